"""
Test infrastructure (like tests/savectc_ref.py): the CPU restatement of xb_ub_tally's contract (include/xna_basecaller.h,
"per-position UB accuracy of mapped rows") in plain Python, written from that contract.  Nothing in the product imports this
module, and it imports nothing of the product.

  target     the template letter in upper case when it is one of A C G T, 'X' otherwise
  query      strand +1: the row in upper case; strand -1: reversed, A <-> T, C <-> G, X <-> Y, every other byte unchanged
  called     '-' everywhere, then the columns from (r_st, q_st): '=' / 'X' store the row letter, 'I' / 'D' advance one side;
             a column that needs a letter past seq_len or a position past r_en, or an unknown byte, ends the walk
  polish     per UB site in ascending order, conditions on the called letters, moves on the polished copy
  tallies    errors against the target, the UB / UB-area / outside masks, X / Y letters detected
"""
import numpy as np

COUNTS = ("n_match", "ub_matches", "ub_len", "ub_area_matches", "ub_area_len", "non_ub_area_matches", "non_ub_area_len",
          "ubs_detected")
CM_ROWS = "ATCGXY"
CM_COLS = "ATCGXY-"
AREA = 5
_COMP = {"A": "T", "T": "A", "C": "G", "G": "C", "X": "Y", "Y": "X"}


def target_letters(template):
    return ["X" if c.upper() not in "ACGT" else c.upper() for c in template]


def _upper(c):
    return c.upper() if "a" <= c <= "z" else c


def query_letters(row, strand):
    """row: str (latin-1, a character per byte) -> the letters on the aligned strand."""
    q = [_upper(c) for c in row]
    if strand < 0:
        q = [_COMP.get(c, c) for c in reversed(q)]
    return q


def called_letters(L, query, q_st, r_st, r_en, ops):
    C = ["-"] * L
    qi, ri = q_st, r_st
    for op in ops:
        op = chr(op)
        if op in "=X":
            if qi >= len(query) or ri >= r_en:
                break
            C[ri] = query[qi]
            qi, ri = qi + 1, ri + 1
        elif op == "I":
            if qi >= len(query):
                break
            qi += 1
        elif op == "D":
            if ri >= r_en:
                break
            ri += 1
        else:
            break
    return C


def polish(C, T):
    L = len(T)
    P = list(C)
    for u in range(L):
        if T[u] != "X" or C[u] == "X":
            continue
        if C[u] == "-":
            lo = hi = u
            while lo > 0 and C[lo - 1] == "-":
                lo -= 1
            while hi < L - 1 and C[hi + 1] == "-":
                hi += 1
            if lo > 0 and C[lo - 1] == "X":
                P[lo - 1], P[u] = "-", "X"
            elif hi < L - 1 and C[hi + 1] == "X":
                P[hi + 1], P[u] = "-", "X"
        elif 1 <= u < L - 1 and C[u - 1] == "-" and C[u + 1] == "X":
            P[u - 1] = P[u]
            P[u] = "X"
            P[u + 1] = "-"
        elif 1 <= u < L - 1 and C[u + 1] == "-" and C[u - 1] == "X":
            P[u + 1] = P[u]
            P[u] = "X"
            P[u - 1] = "-"
    return P


def masks(T):
    L = len(T)
    ub = [t == "X" for t in T]
    area = [False] * L
    for u in range(L):
        if ub[u]:
            for j in range(max(0, u - AREA), min(L, u + AREA + 1)):
                area[j] = True
    return ub, [a and not b for a, b in zip(area, ub)]


def row(template, seq, strand, q_st, r_st, r_en, ops):
    """One mapped row (seq: the row's letters as str, already cut to its clamped length; ops: bytes) -> (counts list in the
    order COUNTS, errors list e[0 .. L), T, P)."""
    T = target_letters(template)
    L = len(T)
    r_st = min(max(r_st, 0), L)
    r_en = min(max(r_en, r_st), L)
    q_st = min(max(q_st, 0), len(seq))
    P = polish(called_letters(L, query_letters(seq, strand), q_st, r_st, r_en, bytes(ops)), T)
    e = [int(p != t) for p, t in zip(P, T)]
    ub, area = masks(T)
    n_match = L - sum(e)
    ub_m = sum(1 for j in range(L) if ub[j] and not e[j])
    ar_m = sum(1 for j in range(L) if area[j] and not e[j])
    counts = [n_match, ub_m, sum(ub), ar_m, sum(area), n_match - ub_m - ar_m, L - sum(ub) - sum(area),
              sum(1 for p in P if p in "XY")]
    return counts, e, T, P


def confusion(T, P, strand):
    cm = np.zeros((len(CM_ROWS), len(CM_COLS)), np.int64)
    for t, p in zip(T, P):
        if strand < 0:
            t, p = _COMP.get(t, t), _COMP.get(p, p)
        if p in CM_COLS:
            cm[CM_ROWS.index(t), CM_COLS.index(p)] += 1
    return cm


def new_accumulators(templates):
    total = sum(len(t) for t in templates)
    return {"reads": np.zeros((len(templates), 2), np.int32), "err": np.zeros((2, total), np.int32), "cm": np.zeros((6, 7), np.int64)}


def tally(rows, lens, mapped, templates, acc=None):
    """The arrays xb_ub_tally writes for rows (n, W) int8 / lens (n) and the mapper's outputs `mapped` (name -> array): (counts
    (n, 8) int32, acc) with acc = {"reads", "err", "cm"}, added to when given."""
    rows = np.asarray(rows, np.int8)
    n, W = rows.shape
    cap = W + max(len(t) for t in templates)
    off = np.concatenate([[0], np.cumsum([len(t) for t in templates])]).astype(np.int64)
    acc = new_accumulators(templates) if acc is None else acc
    counts = np.zeros((n, len(COUNTS)), np.int32)
    for r in range(n):
        t = int(mapped["tmpl"][r])
        if t < 0 or t >= len(templates):
            continue
        sl = min(max(int(lens[r]), 0), W)
        nops = min(max(int(mapped["n_ops"][r]), 0), cap)
        strand = -1 if int(mapped["strand"][r]) < 0 else 1
        seq = rows[r, :sl].astype(np.uint8).tobytes().decode("latin-1")
        c, e, T, P = row(templates[t], seq, strand, int(mapped["q_st"][r]), int(mapped["r_st"][r]), int(mapped["r_en"][r]),
                         np.asarray(mapped["ops"][r, :nops], np.uint8).tobytes())
        counts[r] = c
        s = 1 if strand < 0 else 0
        L = len(T)
        acc["reads"][t, s] += 1
        acc["err"][s, off[t]:off[t] + L] += np.asarray(e[::-1] if s else e, np.int32)
        acc["cm"] += confusion(T, P, strand)
    return counts, acc
