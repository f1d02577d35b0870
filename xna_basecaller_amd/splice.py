"""
XNA spliced augmentation of ctc-data (the reference's ub-bonito/bonito/stitch_chunks.py, `bonito train -m per_kmer`): the
signal of the six k-mers around an unnatural base is cut out of real XNA chunks and pasted into DNA chunks at chosen
positions, resampled to the length of the signal it replaces, and the base is relabelled X or Y.  The reference does this
per read in the data loader; here one device pass (xb_splice_chunks, include/xna_basecaller.h) chooses the positions, looks
the candidates up, resamples and pastes.  This module is the host side: the candidate library, validation, batching.

Departures from the reference, all stated in INTEGRATION.md: the random stream is the contract's counter-based one (draws:
parity unpinned; everything else is pinned to the reference through tests/golden/splice.json); an XNA read without an
unnatural base is skipped where the reference raises; per_slice / mixed stitching, weighted positions, stitch noise,
window permutation are refused; synthetic spikes are spike.py's.
"""
import time

import numpy as np

BASE_MAP = ("N", "A", "C", "G", "T", "X", "Y")
KMER_LEN = 6
EDGE_LEN = 5
MAX_KMER_CNT = 100                         # slice_xna's max_kmer_cnt: a read with a longer k-mer is discarded
TEMPLATES = 7 ** 5
TABLE_LEN = 2 * TEMPLATES * KMER_LEN       # (ub, the five template labels in base 7, kmer_ub_pos)
MAX_SAMPLES = 65535                        # xb_splice_chunks' limits
MAX_LABELS = 65535
MAX_CANDIDATES = 32
MAX_POOL = 2 ** 31 - 1
FILES = ("chunks.npy", "references.npy", "reference_lengths.npy", "breakpoints.npy")


class Library:
    """The candidates of slice_xna(..., 'per_kmer'): `info`, one tuple (ub, template, kmer_ub_pos, kmer, read_idx, slice_st,
    slice_en) per row in the reference's order, and what the device reads: pool (float16, the kept windows back to back),
    rows (n_rows, 2) int32 pool offset and length, table (TABLE_LEN, 2) int32 first row and count of every group."""
    __slots__ = ("info", "pool", "rows", "table")

    def __init__(self, info, pool, rows, table):
        self.info, self.pool, self.rows, self.table = info, pool, rows, table


def table_index(ub, template, kmer_ub_pos):
    """ub 5 | 6, template: five labels, the first the most significant base-7 digit."""
    t = 0
    for v in template:
        t = t * 7 + int(v)
    return ((int(ub) - 5) * TEMPLATES + t) * KMER_LEN + int(kmer_ub_pos)


def _letters(labels):
    return "".join(BASE_MAP[int(v)] for v in labels)


def check_ctc(name, chunks, targets, lengths, bkps, empty_bases=False):
    """What the kernel relies on, chunk by chunk; a violation is a ValueError that names the chunk.  empty_bases: two equal
    breakpoints (a base without a sample) are let through."""
    if chunks.ndim != 2 or targets.ndim != 2 or bkps.shape != targets.shape or lengths.shape != (chunks.shape[0],) \
            or targets.shape[0] != chunks.shape[0]:
        raise ValueError("%s: chunks (n, N), references (n, Lt), reference_lengths (n) and breakpoints (n, Lt) expected, got %s %s "
                         "%s %s" % (name, chunks.shape, targets.shape, lengths.shape, bkps.shape))
    n, N = chunks.shape
    Lt = targets.shape[1]
    if N < 1 or N > MAX_SAMPLES:
        raise ValueError("%s: chunks of %d samples; 1 .. %d are supported" % (name, N, MAX_SAMPLES))
    if Lt < 1 or Lt > MAX_LABELS:
        raise ValueError("%s: label rows of %d entries; 1 .. %d are supported" % (name, Lt, MAX_LABELS))
    lengths = np.asarray(lengths).astype(np.int64)
    bad = np.flatnonzero((lengths < 0) | (lengths > Lt))
    if bad.size:
        raise ValueError("%s chunk %d: reference length %d outside 0 .. %d" % (name, bad[0], lengths[bad[0]], Lt))
    b = np.asarray(bkps).astype(np.int64)
    live = np.arange(Lt)[None, :] < lengths[:, None]
    if int(np.asarray(targets).max(initial=0)) > 6:
        c = int(np.flatnonzero((np.asarray(targets) > 6).any(axis=1))[0])
        raise ValueError("%s chunk %d: a label above 6" % (name, c))
    prev = np.concatenate([np.zeros((n, 1), np.int64), b[:, :-1]], axis=1)
    bad = np.flatnonzero(((b < prev) & live).any(axis=1))
    if bad.size:
        raise ValueError("%s chunk %d: breakpoints decrease" % (name, bad[0]))
    bad = np.flatnonzero(((b == prev) & live).any(axis=1))
    if bad.size and not empty_bases:
        raise ValueError("%s chunk %d: a base without a sample (two equal breakpoints)" % (name, bad[0]))
    bad = np.flatnonzero(((b > N) & live).any(axis=1))
    if bad.size:
        raise ValueError("%s chunk %d: a breakpoint beyond the chunk's %d samples" % (name, bad[0], N))


def build_library(xna_chunks, targets, lengths, bkps):
    """slice_xna(ctc_dir, 'per_kmer', include_chunks=True) (stitch_chunks.py:127-239) -> Library.  The first UB of a read;
    the read is kept when 5 < ub_pos < length - 5 and none of its six k-mers has more than 100 samples; rows ordered by (ub,
    template, kmer_ub_pos, kmer, read_idx) as pandas orders their letters, grouped by (ub, template, kmer_ub_pos) only."""
    check_ctc("XNA", xna_chunks, targets, lengths, bkps)
    found = []
    for read_idx in range(len(lengths)):
        length = int(lengths[read_idx])
        target = np.asarray(targets[read_idx][:length])
        bkp = np.asarray(bkps[read_idx][:length]).astype(np.int64)
        ubs = np.flatnonzero(target > 4)
        if ubs.size == 0:                  # the reference raises IndexError here
            continue
        ub_pos = int(ubs[0])
        if not EDGE_LEN < ub_pos < length - EDGE_LEN:
            continue
        slice_target = target[ub_pos - KMER_LEN + 1:ub_pos + KMER_LEN]
        slice_bkp = bkp[ub_pos - KMER_LEN:ub_pos + 1]
        if np.diff(slice_bkp).max() > MAX_KMER_CNT:
            continue
        for kmer_idx in range(KMER_LEN):
            found.append((BASE_MAP[int(slice_target[5])], _letters(slice_target[:5]), KMER_LEN - kmer_idx - 1,
                          _letters(slice_target[kmer_idx:kmer_idx + KMER_LEN]), read_idx, int(slice_bkp[kmer_idx]),
                          int(slice_bkp[kmer_idx + 1])))
    found.sort(key=lambda r: r[:5])
    # the pool: per kept read its window of six k-mers once, the rows point into it
    window, pieces, total = {}, [], 0
    rows = np.zeros((len(found), 2), np.int32)
    table = np.zeros((TABLE_LEN, 2), np.int32)
    for r, (ub, template, kpos, _, read_idx, st, en) in enumerate(found):
        if read_idx not in window:
            length = int(lengths[read_idx])
            ub_pos = int(np.flatnonzero(np.asarray(targets[read_idx][:length]) > 4)[0])
            w0, w1 = int(bkps[read_idx][ub_pos - KMER_LEN]), int(bkps[read_idx][ub_pos])
            window[read_idx] = (total, w0)
            pieces.append(np.asarray(xna_chunks[read_idx, w0:w1], dtype=np.float16))
            total += w1 - w0
        base, w0 = window[read_idx]
        rows[r] = (base + st - w0, en - st)
        g = table_index(BASE_MAP.index(ub), [BASE_MAP.index(c) for c in template], kpos)
        if table[g, 1] == 0:
            table[g, 0] = r
        table[g, 1] += 1
    if total > MAX_POOL:
        raise ValueError("XNA: a pool of %d samples; the device takes fewer than 2^31" % total)
    pool = np.concatenate(pieces) if pieces else np.zeros(0, np.float16)
    return Library(found, np.ascontiguousarray(pool, dtype=np.float16), rows, table)


def ubs_mask(ubs):
    """'X' | 'Y' | 'XY' (or a list of the letters) -> bit 0 for X, bit 1 for Y."""
    ubs = list(ubs)
    if not ubs or any(u not in ("X", "Y") for u in ubs) or len(set(ubs)) != len(ubs):
        raise ValueError("ubs must be X, Y or XY, got %r" % "".join(str(u) for u in ubs))
    return sum(1 << ("XY".index(u)) for u in ubs)


def check_params(prop_ubs, var_prop_ubs, cand_sample_size, pad):
    if not 1 <= int(cand_sample_size) <= MAX_CANDIDATES:
        raise ValueError("cand_sample_size %d outside 1 .. %d" % (cand_sample_size, MAX_CANDIDATES))
    if int(pad) < 0:
        raise ValueError("ub_pad %d is negative" % pad)
    var = 0.0 if var_prop_ubs is None else float(var_prop_ubs)
    if not np.isfinite(prop_ubs) or not np.isfinite(var) or prop_ubs < 0 or var < 0 or prop_ubs + var > 1:
        raise ValueError("prop_ubs %r +- var_prop_ubs %r must stay within 0 .. 1" % (prop_ubs, var_prop_ubs))
    return var


def _device_call(device, library):
    from . import _lib
    _lib.require_gpu()
    index = int(str(device).split(":")[1]) if ":" in str(device) else 0
    ctx = _lib.mapper_context(index)       # no model is needed
    ctx.splice_library(library.pool, library.rows, library.table)
    return ctx, ctx.splice_chunks


def splice(chunks, targets, lengths, bkps, library, ubs="XY", prop_ubs=0.0, var_prop_ubs=None, cand_sample_size=10, pad=5,
           seed=2012, batch=4096, device="cuda", run=None, timings=None):
    """chunks (n, N), targets (n, Lt), lengths (n), bkps (n, Lt) and a Library -> (chunks float32, targets uint8, success (n,)
    bool, inserted (n,) int32), rows in the input's order.  `run`: the batch call, Context.splice_chunks' signature (default: a
    context on `device` with the library uploaded once).  A chunk's result depends on its global index, never on `batch`.
    `timings` (a dict) receives the seconds spent in the device calls ('device')."""
    mask = ubs_mask(ubs)
    var = check_params(prop_ubs, var_prop_ubs, cand_sample_size, pad)
    check_ctc("DNA", chunks, targets, lengths, bkps)
    if int(batch) < 1:
        raise ValueError("batch must be at least 1")
    n = chunks.shape[0]
    ctx = None
    if run is None:
        ctx, run = _device_call(device, library)
    out = np.empty(chunks.shape, np.float32)
    out_t = np.empty(targets.shape, np.uint8)
    ok = np.zeros(n, bool)
    inserted = np.zeros(n, np.int32)
    t_dev = 0.0
    try:
        for b0 in range(0, n, int(batch)):
            b1 = min(n, b0 + int(batch))
            t0 = time.perf_counter()
            got = run(np.ascontiguousarray(chunks[b0:b1], dtype=np.float32), np.ascontiguousarray(targets[b0:b1], dtype=np.uint8),
                      np.ascontiguousarray(lengths[b0:b1], dtype=np.int32), np.ascontiguousarray(bkps[b0:b1], dtype=np.uint16),
                      b0, int(seed), mask, float(prop_ubs), var, int(cand_sample_size), int(pad))
            t_dev += time.perf_counter() - t0
            out[b0:b1], out_t[b0:b1], ok[b0:b1], inserted[b0:b1] = got[0], got[1], np.asarray(got[2]).astype(bool), got[3]
    finally:
        if ctx is not None:
            ctx.close()
    if timings is not None:
        timings.update(device=t_dev)
    return out, out_t, ok, inserted
