"""
Executable restatement of the Viterbi qualities (xb_decode_q, include/xna_basecaller.h) in float32 numpy, built on the
oracle's decode quantities and its contract exp / log (oracle.expf / oracle.logf).  Every float operation is one IEEE
binary32 operation in the specified order, so the result is bit-comparable with the kernel's.  No reference vectors exist
for this decoder (the reference's Viterbi branch writes the placeholder 'O'): parity unpinned.
"""
import numpy as np

import oracle

F32 = np.float32


def path_edges(scores, nb, sl=3, blank_score=None):
    """(T, N, C) scores -> (f (N, T) int64 arg-max flat edge j*E + k per step, the oracle's decode dict).  f_t is rebuilt
    from the oracle's max-marginals: (amax_t[src] + Q) + bmax_{t+1}[j], lowest flat index on ties."""
    ref = oracle.decode(scores, nb, sl, blank_score=blank_score,
                        want=("alpha", "beta", "logz", "qlog", "amax", "bmax"))
    idx = oracle.crf_idx(nb, sl).reshape(-1)                # src of flat edge j*E + k
    E = nb + 1
    amax, qlog, bmax = ref["amax"], ref["qlog"], ref["bmax"]
    T, N, SE = qlog.shape
    f = np.empty((N, T), np.int64)
    for t in range(T):
        sc = (amax[t][:, idx] + qlog[t]) + np.repeat(bmax[t + 1], E, axis=1)
        f[:, t] = np.argmax(sc, axis=1)                     # first maximum = lowest flat index
    return f, ref


def step_probs(f, alpha, beta, logz, nb, sl=3):
    """p_t (N, T) float32: the k-mer posterior of the path state s_t = f_t / E and its 2 nb shifted neighbours at scan
    index t + 1, summed in the beam search's order, clamped to [0, 1] and raised to 0.4."""
    E, hi = nb + 1, nb ** (sl - 1)
    N, T = f.shape
    s = f // E
    cols = [s]
    for b in range(nb):
        cols += [s // nb + hi * b, (s % hi) * nb + b]
    xs = np.stack(cols, axis=-1)                            # (N, T, 2 nb + 1)
    n_ix = np.arange(N)[:, None, None]
    t_ix = np.arange(T)[None, :, None] + 1
    x = (alpha[t_ix, n_ix, xs] + beta[t_ix, n_ix, xs]) - logz.astype(F32)[:, None, None]
    P = oracle.expf(x)
    p = P[..., 0].copy()
    for g in range(1, 2 * nb + 1):
        p = p + P[..., g]
    p = np.where(p > F32(1), F32(1), p)
    p = np.where(p < F32(0), F32(0), p)
    safe = np.where(p > F32(0), p, F32(1))
    return np.where(p > F32(0), oracle.expf(F32(0.4) * oracle.logf(safe)), F32(0)).astype(F32)


def base_qualities(p, moves, nb, qscale=1.0, qoffset=0.0):
    """Per-base quality characters of one chunk: p (T,) float32, moves (T,) bool -> uint8 array, one per emitting step.
    A base's run is t .. u-1 (u = the next emitting step or T); steps before the first move belong to no base."""
    p = np.asarray(p, F32)
    starts = np.flatnonzero(moves)
    T = len(p)
    if len(starts) == 0:
        return np.zeros(0, np.uint8)
    ends = np.append(starts[1:], T)
    runs = ends - starts
    bp = np.zeros(len(starts), F32)
    tot = np.zeros(len(starts), F32)
    nwrong = F32(nb - 1)
    for j in range(int(runs.max())):
        live = runs > j
        pr = p[np.minimum(starts + j, T - 1)]
        wrong = (F32(1) - pr) / nwrong
        one = pr.copy()
        for _ in range(1, nb):
            one = one + wrong
        bp = np.where(live, bp + pr, bp)
        tot = np.where(live, tot + one, tot)
    with np.errstate(over="ignore", divide="ignore", invalid="ignore"):
        e = F32(1) - bp / tot
        safe = np.where(e > F32(0), e, F32(1))
        q = np.where(e > F32(0), oracle.logf(safe) * F32(-4.3429448190325175), F32(3.402823466e+38)).astype(F32)
        q = q * F32(qscale)
        q = q + F32(qoffset)
    q = np.where(q < F32(1), F32(1), q)
    q = np.where(q > F32(50), F32(50), q)
    return (F32(33.5) + q).astype(np.int32).astype(np.uint8)


def decode_q(scores, nb, alphabet, sl=3, blank_score=None, qscale=1.0, qoffset=0.0):
    """The whole operator: (T, N, C) scores -> dict of 'seq', 'qstring' (N, T) int8 left-packed and zero-padded, 'moves'
    (N, T) uint8, 'seq_len' (N,), 'labels' (N, T) and the path edges 'f' (N, T)."""
    f, ref = path_edges(scores, nb, sl, blank_score)
    E = nb + 1
    labels = (f % E).astype(np.int8)
    moves = (labels != 0).astype(np.uint8)
    p = step_probs(f, ref["alpha"], ref["beta"], ref["logz"], nb, sl)
    N, T = f.shape
    ab = np.frombuffer("".join(alphabet).encode(), np.uint8)
    seq = np.zeros((N, T), np.int8)
    qs = np.zeros((N, T), np.int8)
    lens = np.zeros(N, np.int32)
    for n in range(N):
        em = labels[n] != 0
        k = int(em.sum())
        seq[n, :k] = ab[labels[n][em]].view(np.int8)
        qs[n, :k] = base_qualities(p[n], em, nb, qscale, qoffset).view(np.int8)
        lens[n] = k
    return {"seq": seq, "qstring": qs, "moves": moves, "seq_len": lens, "labels": labels, "f": f, "oracle": ref}
