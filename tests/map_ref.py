"""
Test infrastructure (like tests/qscore_ref.py): the CPU restatement of xb_map_templates' contract (include/xna_basecaller.h,
"mapping calls to a template library") in plain numpy / Python -- full matrices, the stated tie orders.  Nothing in the product
imports this module.

  codes      A C G T (either case) 0..3, every other byte 4; the reverse strand aligns the reverse complement of the codes
  score      local alignment, H = max(0, diagonal, E, F); E (deletion: a template letter with nothing opposite) and F
             (insertion) with gap cost open + k * extend; a column with a code 4 scores -ambiguous
  winner     maximum score; ties: lowest template, + before -, first end cell in row-major order
  trace      diagonal, then E, then F; a gap that can be opened or extended at a cell is opened
  second     best score over the other templates
"""
import numpy as np

NEG = -(1 << 28)
DEFAULT_SCORING = (2, 4, 4, 2, 1)          # match, mismatch, gap_open, gap_extend, ambiguous
_CODE = np.full(256, 4, np.int64)
for _i, _c in enumerate("ACGT"):
    _CODE[ord(_c)] = _CODE[ord(_c.lower())] = _i


def codes(seq):
    if isinstance(seq, str):
        seq = seq.encode("ascii")
    return _CODE[np.frombuffer(bytes(seq), np.uint8)]


def revcomp_codes(c):
    c = np.asarray(c)[::-1]
    return np.where(c < 4, 3 - c, 4)


def _sub(qc, tc, scoring):
    match, mismatch, _, _, ambiguous = scoring
    return np.where((qc == 4) | (tc == 4), -ambiguous, np.where(qc == tc, match, -mismatch))


def matrices(q, t, scoring=DEFAULT_SCORING):
    """Full (n + 1, L + 1) H, E, F of the codes q (rows) against t (columns), cell by cell."""
    _, _, go, ge, _ = scoring
    n, L = len(q), len(t)
    H = np.zeros((n + 1, L + 1), np.int64)
    E = np.full((n + 1, L + 1), NEG, np.int64)
    F = np.full((n + 1, L + 1), NEG, np.int64)
    for i in range(1, n + 1):
        sub = _sub(q[i - 1], np.asarray(t), scoring)
        for j in range(1, L + 1):
            E[i, j] = max(E[i, j - 1] - ge, H[i, j - 1] - go - ge)
            F[i, j] = max(F[i - 1, j] - ge, H[i - 1, j] - go - ge)
            H[i, j] = max(0, H[i - 1, j - 1] + sub[j - 1], E[i, j], F[i, j])
    return H, E, F


def _rows(q, tpad, scoring, want_full=False):
    """The same recurrence, one query row at a time over a stack of templates tpad (P, Lmax) (code 5 pads): yields per row
    the H row (P, Lmax + 1).  E of a row is a running maximum: E[j] = max_k<j (H'[k] - open - (j - k) extend) with H' the row
    without its E term, which equals the cell-by-cell recurrence whenever open >= 0."""
    _, _, go, ge, _ = scoring
    P, Lm = tpad.shape
    Hp = np.zeros((P, Lm + 1), np.int64)
    Fp = np.full((P, Lm + 1), NEG, np.int64)
    ramp = np.arange(Lm + 1, dtype=np.int64) * ge
    for i in range(1, q.shape[1] + 1):
        qc = q[:, i - 1][:, None]
        sub = np.where(tpad == 5, -(1 << 20), _sub(qc, tpad, scoring))
        F = np.maximum(Fp - ge, Hp - go - ge)
        F[:, 0] = NEG
        Hn = np.zeros_like(Hp)
        Hn[:, 1:] = np.maximum(np.maximum(Hp[:, :-1] + sub, F[:, 1:]), 0)
        run = np.maximum.accumulate(Hn + ramp, axis=1)            # max_k<=j (H'[k] + k extend)
        E = np.full_like(Hp, NEG)
        E[:, 1:] = run[:, :-1] - go - ramp[1:]
        Hn[:, 1:] = np.maximum(Hn[:, 1:], E[:, 1:])
        yield i, Hn, E, F
        Hp, Fp = Hn, F


def matrices_by_rows(q, t, scoring=DEFAULT_SCORING):
    """matrices() through the row recurrence (the host tests hold the two equal)."""
    n, L = len(q), len(t)
    H = np.zeros((n + 1, L + 1), np.int64)
    E = np.full((n + 1, L + 1), NEG, np.int64)
    F = np.full((n + 1, L + 1), NEG, np.int64)
    for i, h, e, f in _rows(np.asarray(q)[None, :], np.asarray(t)[None, :], scoring):
        H[i], E[i, 1:], F[i, 1:] = h[0], e[0, 1:], f[0, 1:]
    return H, E, F


def map_read(seq, templates, scoring=DEFAULT_SCORING):
    """One read (str / bytes) against the list of templates -> dict with the outputs of xb_map_templates for that row
    (ops as bytes), tmpl = -1 when nothing scores."""
    qf = codes(seq)
    out = dict(tmpl=-1, strand=0, score=0, second=0, q_st=0, q_en=0, r_st=0, r_en=0, ops=b"", n_ops=0)
    n, R = len(qf), len(templates)
    if n == 0 or R == 0:
        return out
    tc = [codes(t) for t in templates]
    lens = np.array([len(t) for t in tc])
    Lm = int(lens.max())
    tpad = np.full((2 * R, Lm), 5, np.int64)                       # pair p = 2 t + strand
    for t, c in enumerate(tc):
        tpad[2 * t, :len(c)] = tpad[2 * t + 1, :len(c)] = c
    q = np.empty((2 * R, n), np.int64)
    q[0::2], q[1::2] = qf, revcomp_codes(qf)
    real = np.arange(1, Lm + 1)[None, :] <= np.repeat(lens, 2)[:, None]
    best = np.zeros(2 * R, np.int64)
    cell = np.zeros((2 * R, 2), np.int64)
    for i, H, _, _ in _rows(q, tpad, scoring):
        h = np.where(real, H[:, 1:], 0)
        j = h.argmax(axis=1)                                       # first maximum of the row
        v = h[np.arange(2 * R), j]
        up = v > best                                              # strictly: the first row keeps a tie
        best[up] = v[up]
        cell[up, 0], cell[up, 1] = i, j[up] + 1
    top = int(best.max())
    if top <= 0:
        return out
    p = int(np.flatnonzero(best == top)[0])                        # lowest template, + before -
    t, s = p // 2, p % 2
    per_t = np.maximum(best[0::2], best[1::2])
    per_t[t] = 0
    bi, bj = int(cell[p, 0]), int(cell[p, 1])
    qa = q[p]
    H, E, F = matrices_by_rows(qa, tc[t], scoring)
    assert H[bi, bj] == top and H.max() == top
    _, _, go, ge, _ = scoring
    i, j, state, ops = bi, bj, 0, []
    while i > 0 and j > 0:
        if state == 0:
            if H[i, j] == 0:
                break
            d = H[i - 1, j - 1] + int(_sub(qa[i - 1], tc[t][j - 1], scoring))
            if H[i, j] == d:
                ops.append("=" if qa[i - 1] < 4 and qa[i - 1] == tc[t][j - 1] else "X")
                i, j = i - 1, j - 1
            elif H[i, j] == E[i, j]:
                state = 1
            else:
                state = 2
        elif state == 1:
            ops.append("D")
            state = 0 if E[i, j] == H[i, j - 1] - go - ge else 1
            j -= 1
        else:
            ops.append("I")
            state = 0 if F[i, j] == H[i - 1, j] - go - ge else 2
            i -= 1
    ops = "".join(reversed(ops)).encode()
    return dict(tmpl=t, strand=-1 if s else 1, score=top, second=int(per_t.max()) if R > 1 else 0, q_st=i, q_en=bi, r_st=j,
                r_en=bj, ops=ops, n_ops=len(ops))


def map_rows(seq, seq_len, templates, scoring=DEFAULT_SCORING):
    """The arrays xb_map_templates writes for rows seq (n, W) int8 / seq_len (n): name -> array, ops (n, W + Lmax)."""
    seq = np.asarray(seq, np.int8)
    n, W = seq.shape
    lmax = max(len(t) for t in templates)
    out = {k: np.zeros((n,), dt) for k, dt in (("tmpl", np.int32), ("strand", np.int8), ("score", np.int32), ("second", np.int32),
                                                ("q_st", np.int32), ("q_en", np.int32), ("r_st", np.int32), ("r_en", np.int32),
                                                ("n_ops", np.int32))}
    out["ops"] = np.zeros((n, W + lmax), np.uint8)
    for r in range(n):
        k = min(max(int(seq_len[r]), 0), W)
        m = map_read(seq[r, :k].astype(np.uint8).tobytes(), templates, scoring)
        for key in out:
            if key == "ops":
                out["ops"][r, :m["n_ops"]] = np.frombuffer(m["ops"], np.uint8)
            else:
                out[key][r] = m[key]
    return out


def mapq(score, second):
    return min(60, max(0, int(60 * (1 - second / score)))) if score > 0 else 0


def pack_rows(seqs, width=None):
    """Strings -> (n, W) int8 left-packed rows and their lengths."""
    W = max(1, max((len(s) for s in seqs), default=1)) if width is None else width
    rows = np.zeros((len(seqs), W), np.int8)
    for r, s in enumerate(seqs):
        rows[r, :len(s)] = np.frombuffer(s.encode("ascii"), np.int8)
    return rows, np.array([len(s) for s in seqs], np.int32)


def to_mapping(m, names, templates, sequence):
    """map_read's dict as the product's host-side Mapping (None when unmapped): the strings are the host formatters'."""
    from xna_basecaller_amd.aligner import Mapping
    if m["tmpl"] < 0:
        return None
    return Mapping(names[m["tmpl"]], templates[m["tmpl"]], sequence, m["strand"], m["r_st"], m["q_st"], m["ops"], m["score"],
                   m["second"])
