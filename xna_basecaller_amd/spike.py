"""
XNA synthetic spiking of ctc-data (the reference's ub-bonito/bonito/spike_chunks.py, `bonito train --spike`, the default of
its training recipe): at chosen bases of a DNA chunk the signal of the six k-mers around the base is replaced by a synthetic
squiggle -- the k-mers' pore-model levels, each held for as many samples as the base had, plus level noise and added noise --
normalised by the med / mad of the whole chunk's synthetic squiggle, and the base is relabelled X or Y.  The reference does
this per read in the data loader, in numpy; here one device pass (xb_spike_chunks, include/xna_basecaller.h) chooses the
positions, selects med and mad exactly, synthesises and pastes.  `synth` is the reference's third recipe, `bonito train
--spike --fully_synth`: the whole chunk is re-synthesised from the spiked labels and the breakpoints (xb_synth_chunks), med and
mad taken from the spiked labels, one shift and one noise std per chunk.  This module is the host side of both: the model
table, the level distribution, validation, batching.

Departures from the reference, all stated in INTEGRATION.md: the random stream is the contract's counter-based one (draws:
parity unpinned; everything else is pinned to the reference through tests/golden/spike.json); the truncated normal is drawn
through AS241's quantile instead of scipy's; the distributions `normal`, `uniform_shift_*` and `truncnorm_prerep`,
equal_kmer_reps and legacy_pos are refused; a fully synthetic chunk keeps its length (the breakpoints must end at it).
"""
import math
import time

import numpy as np

from .segment import load_kmer_poremodel
from .splice import BASE_MAP, FILES, check_ctc  # noqa: F401 (FILES: the ctc-data files, for the command)

KMER_LEN = 6
MODEL_KMERS = 7 ** KMER_LEN
MAX_SHIFT_ROWS = 32                        # xb_spike_chunks' limit on the shift values of a level distribution
NOISE_TRUNC = 3.0                          # sim_signals' std_trunc of the added noise
STATUS_MISSING_KMER = 2
REFUSED_DISTS = ("normal", "uniform_shift_not_shared", "uniform_shift_shared", "truncnorm_prerep")


def kmer_index(kmer):
    """Six letters of NACGTXY -> the table index: base-7 digits, the first letter the most significant."""
    t = 0
    for ch in kmer:
        t = t * 7 + BASE_MAP.index(ch)
    return t


def index_kmer(index):
    index = int(index)
    return "".join(BASE_MAP[index // 7 ** (KMER_LEN - 1 - q) % 7] for q in range(KMER_LEN))


def model_table(poremodel):
    """{kmer: (level_mean, level_stdv)} (segment.load_kmer_poremodel) -> (mean, stdv), (7^6,) float64 each; a k-mer the model
    lacks has mean NaN."""
    mean = np.full(MODEL_KMERS, np.nan)
    stdv = np.zeros(MODEL_KMERS)
    for kmer, (m, s) in poremodel.items():
        if len(kmer) != KMER_LEN or any(ch not in BASE_MAP for ch in kmer):
            raise ValueError("pore model: k-mer %r is not six letters of %s" % (kmer, "".join(BASE_MAP)))
        if not (math.isfinite(m) and math.isfinite(s) and s >= 0):
            raise ValueError("pore model: k-mer %s has level_mean %r, level_stdv %r" % (kmer, m, s))
        t = kmer_index(kmer)
        mean[t], stdv[t] = m, s
    return mean, stdv


def load_model(path):
    return model_table(load_kmer_poremodel(path))


def phi(x):
    """The standard normal distribution function; erfc keeps the lower tail's relative precision."""
    return 0.5 * math.erfc(-x / math.sqrt(2.0))


def parse_std_dist(std_dist):
    """sim_signals' std_dist (:67-110) -> the truncations (a, b) of the level noise, one per shift value; [] for `uniform`."""
    if std_dist == "uniform":
        return []
    if std_dist == "truncnorm":
        return [(-2.0, 2.0)]
    if std_dist.startswith("truncnorm_shift"):
        parts = std_dist.split("_")
        try:
            if len(parts) != 4:
                raise ValueError
            std_len, shift_range = float(parts[2]), float(parts[3])
        except ValueError:
            raise ValueError("std_dist %r: truncnorm_shift_<len>_<range> expected" % std_dist)
        if not (std_len > 0 and shift_range >= 0 and math.isfinite(std_len) and math.isfinite(shift_range)):
            raise ValueError("std_dist %r: a positive length and a range of at least 0 expected" % std_dist)
        shifts = np.arange(-shift_range, shift_range + .01, 0.5)
        if len(shifts) > MAX_SHIFT_ROWS:
            raise ValueError("std_dist %r has %d shift values; the device takes %d" % (std_dist, len(shifts), MAX_SHIFT_ROWS))
        return [(-std_len + float(s), std_len + float(s)) for s in shifts]
    if std_dist in REFUSED_DISTS or std_dist.startswith("uniform_shift"):
        raise ValueError("std_dist %r is not offered: uniform, truncnorm and truncnorm_shift_<len>_<range> run on the device" % std_dist)
    raise ValueError("std_dist %r is not one of the reference's" % std_dist)


def phi_table(std_dist):
    """-> (dist_rows, phi (dist_rows + 1, 2) float64): per shift value Phi(a) and Phi(b) - Phi(a), then the added noise's row."""
    cuts = parse_std_dist(std_dist)
    rows = [(phi(a), phi(b) - phi(a)) for a, b in cuts + [(-NOISE_TRUNC, NOISE_TRUNC)]]
    for (a, b), (pa, pw) in zip(cuts, rows):
        if not (pa >= 1e-300 and pw > 0 and pa + pw < 1):
            raise ValueError("std_dist %r: the truncation %g .. %g leaves no probability the device can draw from" % (std_dist, a, b))
    return len(cuts), np.array(rows, dtype=np.float64)


def ubs_mask(ubs):
    """'X' | 'Y' | 'XY' -> bit 0 for X, bit 1 for Y; 'N' (re-synthesise the DNA, no unnatural base) -> 0."""
    ubs = "".join(ubs)
    if ubs == "N":
        return 0
    if ubs not in ("X", "Y", "XY"):
        raise ValueError("ubs must be X, Y, XY or N, got %r" % ubs)
    return sum(1 << "XY".index(u) for u in ubs)


def check_params(prop_ubs, var_prop_ubs, pad, noise_std):
    if int(pad) < 0:
        raise ValueError("ub_pad %d is negative" % pad)
    var = 0.0 if var_prop_ubs is None else float(var_prop_ubs)
    if not np.isfinite(prop_ubs) or not np.isfinite(var) or prop_ubs < 0 or var < 0 or prop_ubs + var > 1:
        raise ValueError("prop_ubs %r +- var_prop_ubs %r must stay within 0 .. 1" % (prop_ubs, var_prop_ubs))
    if not np.isfinite(noise_std) or noise_std < 0:
        raise ValueError("noise_std %r must be finite and at least 0" % noise_std)
    return var


def _device_call(device, model, call):
    from . import _lib
    _lib.require_gpu()
    index = int(str(device).split(":")[1]) if ":" in str(device) else 0
    ctx = _lib.mapper_context(index)       # no network is needed
    ctx.spike_model(*model)
    return ctx, getattr(ctx, call)


def _batches(call, chunks, targets, lengths, bkps, model, ubs, prop_ubs, var_prop_ubs, pad, std_dist, noise_std, variable_noise, seed,
             batch, device, run, timings):
    """What spike and synth share: validation, the batches over `run` (default: Context.<call> on `device`), the results."""
    mask = ubs_mask(ubs)
    var = check_params(prop_ubs, var_prop_ubs, pad, noise_std)
    dist_rows, table = phi_table(std_dist)
    check_ctc("DNA", chunks, targets, lengths, bkps, empty_bases=True)     # a k-mer without a sample is synthesised as none
    if call == "synth_chunks":             # the reference's sim_target returns breakpoints[-1] samples: a shorter row cannot be batched
        lens = np.asarray(lengths).astype(np.int64)
        last = np.asarray(bkps)[np.arange(len(lens)), np.maximum(lens, 1) - 1].astype(np.int64)
        short = np.flatnonzero((lens > 0) & (last != chunks.shape[1]))
        if short.size:
            raise ValueError("DNA chunk %d: its last breakpoint is %d, the chunk has %d samples; a fully synthetic chunk is as long as "
                             "its breakpoints say (`segment` always ends them at the chunk)" % (short[0], last[short[0]], chunks.shape[1]))
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    n = chunks.shape[0]
    ctx = None
    if run is None:
        ctx, run = _device_call(device, model, call)
    out = np.empty(chunks.shape, np.float32)
    out_t = np.empty(targets.shape, np.uint8)
    spiked = np.zeros(n, np.int32)
    med, mad = np.zeros(n), np.zeros(n)
    t_dev = 0.0
    try:
        for b0 in range(0, n, int(batch)):
            b1 = min(n, b0 + int(batch))
            t0 = time.perf_counter()
            got = run(np.ascontiguousarray(chunks[b0:b1], dtype=np.float32), np.ascontiguousarray(targets[b0:b1], dtype=np.uint8),
                      np.ascontiguousarray(lengths[b0:b1], dtype=np.int32), np.ascontiguousarray(bkps[b0:b1], dtype=np.uint16),
                      b0, int(seed), mask, float(prop_ubs), var, int(pad), dist_rows, table, float(noise_std), bool(variable_noise))
            t_dev += time.perf_counter() - t0
            bad = np.flatnonzero(np.asarray(got[5]) == STATUS_MISSING_KMER)
            if bad.size:
                raise ValueError("DNA chunk %d: the pore model has no k-mer %s" % (b0 + bad[0], index_kmer(got[3][bad[0]])))
            out[b0:b1], out_t[b0:b1], spiked[b0:b1], med[b0:b1], mad[b0:b1] = got[:5]
    finally:
        if ctx is not None:
            ctx.close()
    if timings is not None:
        timings.update(device=t_dev)
    return out, out_t, spiked, med, mad


def spike(chunks, targets, lengths, bkps, model, ubs="XY", prop_ubs=0.0, var_prop_ubs=None, pad=5, std_dist="uniform",
          noise_std=0.0, variable_noise=False, seed=2012, batch=4096, device="cuda", run=None, timings=None):
    """chunks (n, N), targets (n, Lt), lengths (n), bkps (n, Lt) and a model (mean, stdv: model_table) -> (chunks float32,
    targets uint8, spiked (n,) int32, med (n,), mad (n,) float64), rows in the input's order.  `run`: the batch call,
    Context.spike_chunks' signature (default: a context on `device` with the model uploaded once).  A chunk's result depends
    on its global index, never on `batch`.  A chunk that needs a k-mer the model lacks is a ValueError that names both.
    `timings` (a dict) receives the seconds spent in the device calls ('device')."""
    return _batches("spike_chunks", chunks, targets, lengths, bkps, model, ubs, prop_ubs, var_prop_ubs, pad, std_dist, noise_std,
                    variable_noise, seed, batch, device, run, timings)


def synth(chunks, targets, lengths, bkps, model, ubs="XY", prop_ubs=0.0, var_prop_ubs=None, pad=5, std_dist="uniform",
          noise_std=0.0, variable_noise=False, seed=2012, batch=4096, device="cuda", run=None, timings=None):
    """Fully synthetic chunks: spike's arguments and return tuple; `run` has Context.synth_chunks' signature.  Every sample of
    a chunk is synthesised from its spiked labels (`chunks` gives only the shape), `spiked` may be 0 with the chunk still
    synthesised.  A chunk whose last breakpoint is not its number of samples is a ValueError that names it, and so is a chunk
    whose spiked labels need a k-mer the model lacks."""
    return _batches("synth_chunks", chunks, targets, lengths, bkps, model, ubs, prop_ubs, var_prop_ubs, pad, std_dist, noise_std,
                    variable_noise, seed, batch, device, run, timings)
