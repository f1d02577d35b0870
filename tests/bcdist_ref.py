"""
Test infrastructure (like tests/ubtally_ref.py): the CPU restatement of xb_barcode_dist's contract (include/xna_basecaller.h,
"barcode distance of mapped rows") in plain Python, written from that contract.  Nothing in the product imports this module,
and it imports nothing of the product.

  barcode    template[bc_pos : bc_pos + bc_len], clipped to the template, a-z in upper case, every other byte as it is
  query      strand +1: the row in upper case; strand -1: reversed, A <-> T, C <-> G, X <-> Y, every other byte unchanged
  start      max(q_st + bc_pos - r_st, 0) with q_st clamped to [0, seq_len] and r_st to [0, L]
  windows    i = max(start - relax, 0) .. start + relax, ascending; obs = Q[i : min(i + bc_len, seq_len)]
  distance   unit-cost Levenshtein(barcode, obs); the first strictly smaller one wins
"""
import numpy as np

OUTPUTS = ("bc_dist", "bc_start", "bc_end", "bc_obs_len")
_COMP = {"A": "T", "T": "A", "C": "G", "G": "C", "X": "Y", "Y": "X"}


def _upper(c):
    return c.upper() if "a" <= c <= "z" else c


def levenshtein(a, b):
    """Unit-cost edit distance of two sequences, the textbook row-by-row DP."""
    prev = list(range(len(b) + 1))
    for i, ca in enumerate(a, 1):
        cur = [i]
        for j, cb in enumerate(b, 1):
            cur.append(min(prev[j] + 1, cur[j - 1] + 1, prev[j - 1] + (ca != cb)))
        prev = cur
    return prev[len(b)]


def barcode(template, bc_pos, bc_len):
    return [_upper(c) for c in template[bc_pos:bc_pos + bc_len]]


def query_letters(row, strand):
    """row: str (latin-1, a character per byte) -> the letters on the aligned strand."""
    q = [_upper(c) for c in row]
    if strand < 0:
        q = [_COMP.get(c, c) for c in reversed(q)]
    return q


def row(template, seq, strand, q_st, r_st, bc_pos, bc_len, relax=3):
    """One mapped row (seq: the row's letters as str, already cut to its clamped length) -> (dist, start, end, obs_len)."""
    L = len(template)
    B = barcode(template, bc_pos, bc_len)
    Q = query_letters(seq, strand)
    q_st = min(max(q_st, 0), len(Q))
    r_st = min(max(r_st, 0), L)
    start = max(q_st + bc_pos - r_st, 0)
    best = None
    for i in range(max(start - relax, 0), start + relax + 1):
        obs = Q[i:min(i + bc_len, len(Q))] if i < len(Q) else []
        d = levenshtein(B, obs)
        if best is None or d < best[0]:
            best = (d, i, i + bc_len, len(obs))
    return best


def dist(rows, lens, mapped, templates, bc_pos, bc_len, relax=3):
    """The arrays xb_barcode_dist writes for rows (n, W) int8 / lens (n) and the mapper's outputs `mapped` (name -> array):
    dict of the four (n) int32 arrays named in OUTPUTS."""
    rows = np.asarray(rows, np.int8)
    n, W = rows.shape
    out = {k: np.zeros(n, np.int32) for k in OUTPUTS}
    for r in range(n):
        t = int(mapped["tmpl"][r])
        if t < 0 or t >= len(templates):
            out["bc_dist"][r] = -1
            continue
        sl = min(max(int(lens[r]), 0), W)
        strand = -1 if int(mapped["strand"][r]) < 0 else 1
        seq = rows[r, :sl].astype(np.uint8).tobytes().decode("latin-1")
        got = row(templates[t], seq, strand, int(mapped["q_st"][r]), int(mapped["r_st"][r]), bc_pos, bc_len, relax)
        for k, v in zip(OUTPUTS, got):
            out[k][r] = v
    return out


def demux(dists, read_ids, max_dist):
    """The reference's two-step filter over alignment rows: keep dist <= max_dist (and >= 0), then per read id the rows whose
    distance equals that read's minimum, ties kept.  Returns the kept row indices, ascending."""
    ok = [k for k, d in enumerate(dists) if 0 <= d <= max_dist]
    low = {}
    for k in ok:
        low[read_ids[k]] = min(low.get(read_ids[k], dists[k]), dists[k])
    return [k for k in ok if dists[k] == low[read_ids[k]]]
