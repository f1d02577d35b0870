"""
Executable restatement of the per-base letter probabilities (xb_decode_ub, include/xna_basecaller.h) in float32 numpy,
built on the oracle's decode quantities (its edge posteriors) and the Viterbi qualities of tests/qscore_ref.py.  Every float
operation is one IEEE binary32 operation in the specified order, so the bytes are bit-comparable with the kernel's.  No
reference vectors exist for this output: parity unpinned.
"""
import numpy as np

import oracle
import qscore_ref

F32 = np.float32


def move_mass(post, nb, sl=3):
    """post (T, N, S*E) edge posteriors -> m (T, N, S): per source state i the posteriors of its nb move edges
    (j = (i % hi) * nb + e - 1, k = i / hi + 1) summed in edge order e = 1..nb, from 0."""
    S, E, hi = nb ** sl, nb + 1, nb ** (sl - 1)
    i = np.arange(S)
    jb, kk = (i % hi) * nb, i // hi + 1
    T, N, _ = post.shape
    m = np.zeros((T, N, S), F32)
    for e in range(1, nb + 1):
        m = m + post[:, :, (jb + e - 1) * E + kk]
    return m


def letter_mass(m, nb, sl=3):
    """m (T, N, S) -> e (T, N, nb): letter b sums the sources b*hi .. b*hi+hi-1.  Lane g = 0..15 sums q = g, g+16, ..
    in increasing order from 0, then four rounds x_g = x_{g-d} + x_g (g >= d; d = 1, 2, 4, 8) and e = x_15."""
    hi = nb ** (sl - 1)
    T, N, _ = m.shape
    mm = m.reshape(T, N, nb, hi)
    x = np.zeros((T, N, nb, 16), F32)
    for q in range(hi):
        x[..., q % 16] = x[..., q % 16] + mm[..., q]
    for d in (1, 2, 4, 8):
        y = x.copy()
        y[..., d:] = x[..., :-d] + x[..., d:]
        x = y
    return x[..., 15].copy()


def base_windows(moves):
    """moves (T,) bool -> [(t_i, lo, hi)]: per emitting step t_i the window lo .. hi-1 = t_{i-1}+1 .. t_{i+1}-1
    (t_0 = -1, t_{L+1} = T)."""
    ts = np.flatnonzero(np.asarray(moves, bool))
    T = len(moves)
    prev = np.concatenate([[-1], ts[:-1]])
    nxt = np.concatenate([ts[1:], [T]])
    return [(int(t), int(p) + 1, int(q)) for t, p, q in zip(ts, prev, nxt)]


def base_probs(e, moves):
    """One chunk: e (T, nb) float32, moves (T,) bool -> (prob (L, nb) float32, bytes (L, nb) uint8) per called base.
    mass = 0 + e_u summed over the window in increasing u, tot = mass summed in letter order, prob = mass / tot,
    byte = min(255, (int)(256 prob)); all 0 where tot = 0."""
    e = np.asarray(e, F32)
    nb = e.shape[1]
    win = base_windows(moves)
    prob = np.zeros((len(win), nb), F32)
    for i, (_, lo, hi) in enumerate(win):
        mass = np.zeros(nb, F32)
        for u in range(lo, hi):
            mass = mass + e[u]
        tot = mass[0]
        for b in range(1, nb):
            tot = F32(tot + mass[b])
        if tot > 0:
            prob[i] = mass / tot
    v = (F32(256) * prob).astype(np.int32)
    return prob, np.minimum(v, 255).astype(np.uint8)


def decode_ub(scores, nb, alphabet, sl=3, blank_score=None, qscale=1.0, qoffset=0.0):
    """The whole operator: (T, N, C) scores -> qscore_ref.decode_q's dict plus 'probs' (N, nb, T) uint8 and 'prob'
    (N, nb, T) float32, left-packed beside 'seq' and zero-padded, 'e' (T, N, nb) and 'post' (T, N, S*E)."""
    out = qscore_ref.decode_q(scores, nb, alphabet, sl, blank_score, qscale, qoffset)
    post = oracle.decode(scores, nb, sl, blank_score=blank_score, want=("post",))["post"]
    e = letter_mass(move_mass(post, nb, sl), nb, sl)
    N, T = out["seq"].shape
    probs = np.zeros((N, nb, T), np.uint8)
    prob = np.zeros((N, nb, T), F32)
    for n in range(N):
        pr, by = base_probs(e[:, n], out["moves"][n] != 0)
        L = len(by)
        probs[n, :, :L] = by.T
        prob[n, :, :L] = pr.T
    out.update(probs=probs, prob=prob, e=e, post=post)
    return out
