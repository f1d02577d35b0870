"""
DTW signal segmentation of ctc-data (the reference's src/tools/dtw_segmentation.py): for every chunk the sample index where
each reference base's signal ends -- `breakpoints.npy`, which the reference's XNA augmentation (here: splice.py) cannot load
a data set without.  The alignment itself runs on the device (xb_dtw_segment, include/xna_basecaller.h: parity unpinned); this module
is the host side: the k-mer pore model, the expected levels of a reference sequence, batching.

Departures from the reference, all stated in INTEGRATION.md: the noise of the level normalisation comes from an explicit
np.random.RandomState(seed) drawn chunk by chunk in file order (the reference draws from the unseeded global np.random, so
its own output is not reproducible; seeding the global generator with the same value gives it the same numbers); a k-mer
the model lacks is an error naming it; the median filtering of the signal (`smooth_val`) is not offered.
"""
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np

BASE_MAP = ("N", "A", "C", "G", "T", "X", "Y")
SHORT_MEAN, SHORT_STDV = 90.2083, 2.0      # dtw_segmentation.py:110-111: a sequence shorter than k
NORM_REP = 100                             # normalize_med_mad_squiggly's norm_rep
MAX_SAMPLES = 65535                        # xb_dtw_segment's limits
MAX_COLUMNS = 65535


def load_kmer_poremodel(path):
    """The tab-separated pore model (columns kmer, level_mean, level_stdv among others; `#` starts a comment) as
    {kmer: (level_mean, level_stdv)} (misc/data_io.py:696-704)."""
    model, cols = {}, None
    with open(path) as fh:
        for line in fh:
            line = line.split("#", 1)[0].rstrip("\r\n")
            if not line.strip():
                continue
            f = line.split("\t")
            if cols is None:
                try:
                    cols = [f.index(c) for c in ("kmer", "level_mean", "level_stdv")]
                except ValueError:
                    raise ValueError("%s: no kmer / level_mean / level_stdv header" % path)
                continue
            model[f[cols[0]]] = (float(f[cols[1]]), float(f[cols[2]]))
    if not model:
        raise ValueError("%s: no k-mer rows" % path)
    return model


def target_string(target, length, ubs_map=None):
    """The first `length` labels of a references.npy row as letters; ubs_map 'AT' reads X as A and Y as T (:134-143)."""
    s = "".join(BASE_MAP[int(v)] for v in np.asarray(target)[:int(length)])
    if ubs_map is not None:
        if len(ubs_map) != 2 or any(c not in BASE_MAP for c in ubs_map):
            raise ValueError("ubs_map takes two letters of %s: the first for X, the second for Y" % "".join(BASE_MAP))
        s = s.replace("X", ubs_map[0]).replace("Y", ubs_map[1])
    return s


def kmer_levels(sequence, poremodel, k=6, chunk=None):
    """get_kmers_model (:90-126): the sequence gets an ATATA / TATAT tail so that every base starts a k-mer; -> (means, stdvs)."""
    if not sequence:
        raise ValueError("chunk %s: empty reference sequence" % chunk)
    sequence += "ATATA" if sequence[-1] != "A" else "TATAT"
    if k < 6:
        sequence = sequence[:k - 6]
    if len(sequence) < k:
        return [SHORT_MEAN] * len(sequence), [SHORT_STDV] * len(sequence)
    means, stdvs = [], []
    for i in range(len(sequence) - k + 1):
        kmer = sequence[i:i + k]
        if kmer not in poremodel:
            raise ValueError("chunk %s: the pore model has no k-mer %s (position %d of %s)" % (chunk, kmer, i, sequence))
        m, s = poremodel[kmer]
        means.append(m)
        stdvs.append(s)
    return means, stdvs


def _squiggle(means, stdvs, rng):
    """The noisy copy normalize_med_mad_squiggly takes its statistics from: every level NORM_REP times plus uniform noise of
    its own stdv.  The ONLY use of the generator."""
    rep = np.repeat(stdvs, NORM_REP)
    return np.repeat(means, NORM_REP) + rng.uniform(-1 * rep, rep)


def _normalise(means, squiggly):
    """normalize_med_mad_squiggly's second half (misc/utils.py:1986-1988): two medians, no randomness."""
    med = np.median(squiggly)
    mad = np.median(np.absolute(squiggly - med)) * 1.4826 + np.finfo(np.float32).eps
    return (np.asarray(means, dtype=np.float64) - med) / mad


def reference_levels(target, length, poremodel, ubs_map=None, k=6, rng=None, chunk=None):
    """The expected normalised levels of one chunk's reference: one float64 per k-mer (= per base for k <= 6)."""
    if rng is None:
        raise ValueError("reference_levels needs an explicit np.random.RandomState")
    means, stdvs = kmer_levels(target_string(target, length, ubs_map), poremodel, k, chunk)
    return _normalise(means, _squiggle(means, stdvs, rng))


def naive_breakpoints(chunksize, length):
    reps = np.full(int(length), chunksize // int(length))
    reps[:chunksize % int(length)] += 1
    return np.cumsum(reps)


def naive_segment(chunksize, targets, lengths):
    """dtw_segmentation.py:268-277: the same repetition for every base."""
    bkps = np.zeros_like(targets, dtype=np.uint16)
    for i, length in enumerate(lengths):
        b = naive_breakpoints(chunksize, length)
        assert b[-1] == chunksize
        bkps[i, :len(b)] = b
    return bkps, np.ones(len(lengths), dtype=bool)


def _device_call(device):
    from . import _lib
    _lib.require_gpu()
    index = int(str(device).split(":")[1]) if ":" in str(device) else 0
    # a context without a model: the smallest encoder geometry, nothing of it is used
    ctx = _lib.Context(index, 6, 3, 64, 19, 5, 5.0, 2.0, 1000, 4)
    return ctx, ctx.dtw_segment


def segment(chunks, targets, lengths, poremodel, ref_rep=3, window_size=None, ubs_map=None, seed=25, k=6, batch=1024,
            workers=4, device="cuda", dtw=None, timings=None):
    """chunks (n, N), targets (n, Lt) labels, lengths (n) -> (breakpoints uint16 shaped like targets, ok (n,) bool).
    `dtw`: the batch aligner, Context.dtw_segment's signature (default: a context on `device`).  The levels of batch b + 1 are
    built by `workers` threads while the device aligns batch b; the random draws stay on ONE generator in file order, so the
    result does not depend on `workers` or `batch`.  `timings` (a dict) receives the seconds spent building levels
    ('levels', summed over the threads), waiting for them ('levels_wait') and in the device calls ('device')."""
    n, N = chunks.shape
    if N < 1 or N > MAX_SAMPLES:
        raise ValueError("chunks of %d samples; 1 .. %d are supported (breakpoints are uint16)" % (N, MAX_SAMPLES))
    if ref_rep < 1:
        raise ValueError("ref_rep must be at least 1")
    ctx = None
    if dtw is None:
        ctx, dtw = _device_call(device)
    rng = np.random.RandomState(seed)
    bkps = np.zeros_like(targets, dtype=np.uint16)
    ok = np.zeros(n, dtype=bool)
    t_levels = [0.0]

    def finish(args):
        t0 = time.perf_counter()
        out = _normalise(*args)
        t_levels[0] += time.perf_counter() - t0
        return out

    def start(b0):
        """Draw batch b0's noise here, in file order; hand the medians to the pool."""
        t0 = time.perf_counter()
        jobs = []
        for c in range(b0, min(b0 + batch, n)):
            length = int(lengths[c])
            means, stdvs = kmer_levels(target_string(targets[c], length, ubs_map), poremodel, k, c)
            if len(means) != length:
                raise ValueError("chunk %d: %d levels for %d bases (a %d-mer model needs sequences of at least %d letters)"
                                 % (c, len(means), length, k, k - 5))
            if len(means) * ref_rep > MAX_COLUMNS:
                raise ValueError("chunk %d: %d bases x ref_rep %d exceeds %d columns" % (c, length, ref_rep, MAX_COLUMNS))
            jobs.append((means, _squiggle(means, stdvs, rng)))
        t_levels[0] += time.perf_counter() - t0
        return [pool.submit(finish, j) for j in jobs]

    t_wait = t_dev = 0.0
    with ThreadPoolExecutor(max(1, int(workers))) as pool:
        pending = start(0) if n else []
        for b0 in range(0, n, batch):
            t0 = time.perf_counter()
            levels = [f.result() for f in pending]
            t_wait += time.perf_counter() - t0
            pending = start(b0 + batch) if b0 + batch < n else []
            b1 = b0 + len(levels)
            window = None
            if window_size is not None:
                window = np.array([(N / int(lengths[c])) * window_size for c in range(b0, b1)], dtype=np.float64)
            t0 = time.perf_counter()
            bp, good, _ = dtw(np.ascontiguousarray(chunks[b0:b1], dtype=np.float32), levels, ref_rep, window,
                              max(len(v) for v in levels))
            t_dev += time.perf_counter() - t0
            for c in range(b0, b1):
                bkps[c, :len(levels[c - b0])] = bp[c - b0, :len(levels[c - b0])]
            ok[b0:b1] = good
    if ctx is not None:
        ctx.close()
    if timings is not None:
        timings.update(levels=t_levels[0], levels_wait=t_wait, device=t_dev)
    return bkps, ok
