"""A plain-Python / numpy restatement of xb_synth_chunks' contract (include/xna_basecaller.h): the reference's fully synthetic
chunks (ub-bonito/bonito/spike_chunks.py: spike_read with fully_synth=True, sim_target, sim_signals with append=True), from
the pieces of tests/spike_ref.py -- the same draws, positions, logarithm, PPND16 and medians.  Test infrastructure only."""
import math

import numpy as np

import splice_ref
from spike_ref import KMER_LEN, Sequential, Stream, kmer_index, letters_with_tail, med_mad, ppnd16


def synth_chunk(signal, target, length, bkp, model, chunk_index, seed, ubs_mask, prop, var_prop, pad, dist_rows, phi, noise_std,
                variable_noise, stats=None):
    """One chunk -> (signal float32, target uint8, spiked, med, mad, status).  model: (mean, stdv) of 7^6 k-mers; phi:
    (dist_rows + 1, 2) float64; stats (a dict) collects 'positions', 'ubs', 'empty' (bases without a sample), 'total' (samples
    synthesised) and 'ppnd' (samples that went through a truncated normal)."""
    out = np.array(signal, dtype=np.float32)
    out_t = np.array(target, dtype=np.uint8)
    length = max(0, min(int(length), len(out_t)))
    N = len(out)
    stats = {} if stats is None else stats
    for key in ("positions", "ubs"):
        stats.setdefault(key, [])
    for key in ("empty", "total", "ppnd"):
        stats.setdefault(key, 0)
    if length == 0:
        return out, out_t, 0, 0.0, 0.0, 0
    mean, stdv = model
    tgt = [min(int(v), 6) for v in np.asarray(target)[:length]]
    b = [min(int(v), N) for v in np.asarray(bkp)[:length]]

    # ---- stream 0, exactly as spike_ref.spike_chunk spends it
    draws = Sequential(seed, chunk_index)
    if var_prop is not None and var_prop > 0:
        lo, hi = prop - var_prop, prop + var_prop
        prop = lo + (hi - lo) * draws.unit()
    ubs_pos = [p for p in range(length) if tgt[p] > 4]
    n_pos = max(splice_ref.rint(float(length) * float(prop)) - len(ubs_pos), 1)
    positions = splice_ref.choose_positions(length, n_pos, pad, ubs_pos, draws)
    n = len(positions)
    if ubs_mask == 3:
        ubs = [5 + (i & 1) for i in range(n + n % 2)]
        for i in range(len(ubs) - 1, 0, -1):
            j = draws.bounded(i + 1)
            ubs[i], ubs[j] = ubs[j], ubs[i]
        ubs = ubs[:n]
    else:
        ubs = [0 if ubs_mask == 0 else 4 + ubs_mask] * n
    stats["positions"].append(positions)
    stats["ubs"].append(ubs)

    # ---- the spiked row and its k-mers, one per base; the first missing one in base order ends the chunk
    spiked = list(tgt)
    for pos, ub in zip(positions, ubs):
        if ub:
            spiked[pos] = ub
    full = letters_with_tail(spiked)
    idx = [kmer_index(full[i:i + KMER_LEN]) for i in range(length)]
    for t in idx:
        if math.isnan(mean[t]):
            return out, out_t, 0, float(t), float("nan"), 2

    med, mad = med_mad(spiked, model, seed, chunk_index)

    # ---- the samples: stream 2 serves the whole chunk
    total = b[length - 1]
    stream = Stream(seed, chunk_index, 2)
    if dist_rows > 0:
        pa, pw = (float(v) for v in phi[stream.bounded(0, dist_rows)])
    sigma = float(noise_std)
    if noise_std > 0 and variable_noise:
        sigma = 0.0 + (float(noise_std) - 0.0) * stream.unit(1)
    na, nw = (float(v) for v in phi[dist_rows])
    start = 0
    for base in range(length):
        end = max(b[base], start)                           # what the host form refuses: a decreasing breakpoint
        stats["empty"] += end == start
        m, s = float(mean[idx[base]]), float(stdv[idx[base]])
        for i in range(start, end):
            u = stream.unit(2 + i)
            if dist_rows == 0:
                lo = -s
                level = lo + (s - lo) * u
            else:
                level = ppnd16(pa + u * pw) * s
            v = m + level
            if noise_std > 0:
                v = v + ppnd16(na + stream.unit(2 + total + i) * nw) * sigma
            out[i] = np.float32((v - med) / mad)
        start = end
    stats["total"] += total
    stats["ppnd"] += total if (dist_rows > 0 or noise_std > 0) else 0
    for pos, ub in zip(positions, ubs):
        if ub:
            out_t[pos] = ub
    return out, out_t, n, med, mad, 0


def synth_batch(model):
    """A stand-in for Context.synth_chunks over `model` (what spike.synth takes as `run=`)."""
    def run(signal, targets, lengths, bkps, first_index, seed, ubs_mask, prop, var_prop=0.0, pad=5, dist_rows=0, phi=None,
            noise_std=0.0, variable_noise=False):
        n = signal.shape[0]
        phi = np.zeros((1, 2)) if phi is None else np.asarray(phi, dtype=np.float64).reshape(-1, 2)
        out, out_t = np.empty(signal.shape, np.float32), np.empty(targets.shape, np.uint8)
        spiked, status = np.zeros(n, np.int32), np.zeros(n, np.int8)
        med, mad = np.zeros(n), np.zeros(n)
        for c in range(n):
            out[c], out_t[c], spiked[c], med[c], mad[c], status[c] = synth_chunk(
                signal[c], targets[c], lengths[c], bkps[c], model, first_index + c, seed, ubs_mask, prop, var_prop, pad, dist_rows,
                phi, noise_std, variable_noise)
        return out, out_t, spiked, med, mad, status
    return run

