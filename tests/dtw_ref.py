"""
Test infrastructure (like tests/map_ref.py): the CPU restatement of xb_dtw_segment's contract (include/xna_basecaller.h,
"DTW signal segmentation"), float64 numpy, one row of the recurrence at a time.  dtw-python is in no image: parity unpinned,
the contract is the header's.

    d(i, j) = |q[i] - r[j]|;  g(0, 0) = d(0, 0);  g(i, j) = d(i, j) + min(g(i-1, j), g(i-1, j-1)), ties to the stay step;
    band |j - i M / N| <= window;  end (N-1, M-1);  failure -> the naive split.
"""
import numpy as np


def naive_breakpoints(N, K):
    """dtw_segmentation.py:186-191: N // K samples per base, the first N % K bases one more."""
    reps = np.full(K, N // K, dtype=np.int64)
    reps[:N % K] += 1
    return np.cumsum(reps)


def allowed_row(i, N, M, window):
    """Boolean (M,) of the cells of row i the slanted band allows; window None / negative: all of them."""
    if window is None or window < 0:
        return np.ones(M, dtype=bool)
    j = np.arange(M, dtype=np.float64)
    return np.abs(j - (i * M) / N) <= window


def dtw(chunk, levels, ref_rep=1, window=None):
    """One chunk -> (breakpoints (K,) int64, ok, cost float64, ties): ties = the reachable cells whose two predecessors are
    finite and equal (where the stay-first rule decides)."""
    q = np.asarray(chunk, dtype=np.float32).astype(np.float64)
    lev = np.asarray(levels, dtype=np.float64)
    N, K = len(q), len(lev)
    r = np.repeat(lev, ref_rep)
    M = len(r)
    if M > N:
        return naive_breakpoints(N, K), False, np.inf, 0
    take = np.zeros((N, M), dtype=bool)                    # True: the diagonal step (i-1, j-1) was taken
    g = np.full(M, np.inf)
    g[0] = np.abs(q[0] - r[0])
    ties = 0
    for i in range(1, N):
        stay = g
        diag = np.concatenate(([np.inf], g[:-1]))
        t = diag < stay                                    # strictly smaller, else stay
        ties += int(np.count_nonzero((diag == stay) & np.isfinite(stay)))
        best = np.where(t, diag, stay)
        g = np.abs(q[i] - r) + best                        # one addition per cell
        g[~allowed_row(i, N, M, window)] = np.inf
        take[i] = t
    cost = g[M - 1]
    if not cost < np.inf:
        return naive_breakpoints(N, K), False, np.inf, ties
    reps = np.zeros(K, dtype=np.int64)
    j = M - 1
    for i in range(N - 1, -1, -1):
        reps[j // ref_rep] += 1
        if i > 0 and take[i, j]:
            j -= 1
    assert j == 0
    return np.cumsum(reps), True, float(cost), ties


def dtw_batch(signal, levels, ref_rep=1, window=None, kmax=None):
    """The arrays xb_dtw_segment writes: (breakpoints (n, kmax) int32 zero-filled, ok (n,) bool, cost (n,) float64) and the
    total tie count."""
    n = len(signal)
    kmax = kmax if kmax is not None else max(len(v) for v in levels)
    bp = np.zeros((n, kmax), np.int32)
    ok = np.zeros(n, bool)
    cost = np.zeros(n, np.float64)
    ties = 0
    for c in range(n):
        b, ok[c], cost[c], t = dtw(signal[c], levels[c], ref_rep, None if window is None else float(window[c]))
        bp[c, :len(b)] = b
        ties += t
    return bp, ok, cost, ties


def device_stand_in(signal, levels, ref_rep=3, window=None, kmax=None):
    """dtw_batch in the shape of Context.dtw_segment (for segment.py driven without a device)."""
    return dtw_batch(signal, levels, ref_rep, window, kmax)[:3]
