#!/usr/bin/env python
"""GPU box: time of xb_dtw_segment (the aligner behind `segment`) for a training-set-shaped batch: 4096 chunks of 3600 samples
against about 400 levels each at ref_rep 3, without and with a slanted band (-w 5), after a warm-up call, with HIP events
around the device-pointer form; per case the ms of every repeat, the cells/s over the FEASIBLE cells (j <= i,
M - 1 - j <= N - 1 - i, inside the band), and the bytes of choice scratch the launches are sized for (XB_DTW_SCRATCH_MB bounds
what one launch owns: set it in the environment to see how the time follows the chunks per launch).  Beside it the host: the time
to build the reference levels of the batch (segment.py's two medians per chunk, one thread), and tests/dtw_ref.py -- the numpy
restatement of the contract -- on a sample of the chunks as the stand-in for the reference's host DTW (dtw-python itself is
in no image, so ITS time is not measured here).

The split of a call into kernels comes from a kernel trace: run this script under
`rocprofv3 --kernel-trace --stats --output-format csv -d DIR --` and pass the *kernel_stats.csv with --stats.

    python tools/dtw_time.py [--chunks 4096] [--repeat 5] [--host-sample 8] [--stats kernel_stats.csv]
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from xna_basecaller_amd import _lib  # noqa: E402
from xna_basecaller_amd import segment as seg  # noqa: E402


def feasible_cells(N, M, window):
    """Cells of one chunk a path can use: j <= i, M - 1 - j <= N - 1 - i, and |j - i M / N| <= window when there is one."""
    if M > N:
        return 0
    if window is None or window < 0:
        return (N - M + 1) * M
    i = np.arange(N, dtype=np.float64)[:, None]
    total = 0
    for j0 in range(0, M, 256):                            # in column blocks: the whole lattice is 3600 x 1200 doubles
        j = np.arange(j0, min(M, j0 + 256), dtype=np.float64)[None, :]
        ok = (j <= i) & (M - 1 - j <= N - 1 - i) & (np.abs(j - i * M / N) <= window)
        total += int(ok.sum())
    return total


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=3600)
    ap.add_argument("--levels", type=int, default=400)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=8)
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of an earlier run of this script: prints the kernels' times")
    args = ap.parse_args()
    if args.stats:
        for row in csv.DictReader(open(args.stats)):
            if "dtw_" in row["Name"]:
                print("%-70s calls %4s  average %.3f ms" % (row["Name"][:70], row["Calls"], float(row["AverageNs"]) * 1e-6))
        return
    import torch
    import dtw_ref
    _lib.require_gpu()
    ctx = _lib.Context(0, 4, 3, 32, 19, 5, 5.0, 2.0, 200, 1)
    rng = np.random.RandomState(1)
    n, N, rep = args.chunks, args.samples, 3
    Ks = rng.randint(args.levels - 40, args.levels + 41, n)
    # host: the reference levels of the batch from a seeded 6-mer table, one thread
    import itertools
    model = {"".join(k): (rng.uniform(60.0, 125.0), rng.uniform(0.8, 3.0)) for k in itertools.product("ACGT", repeat=6)}
    targets = [rng.randint(1, 5, K) for K in Ks]
    t0 = time.perf_counter()
    noise = np.random.RandomState(25)
    levels = [seg.reference_levels(t, len(t), model, rng=noise, chunk=c) for c, t in enumerate(targets)]
    t_levels = time.perf_counter() - t0
    print("host: reference levels of %d chunks (mean %.0f bases): %.2f s on one thread, %.3f ms per chunk"
          % (n, Ks.mean(), t_levels, 1e3 * t_levels / n))
    # signal: every level held for a random share of the chunk, plus noise -- what an aligned chunk looks like
    signal = np.empty((n, N), np.float32)
    for c, lev in enumerate(levels):
        cuts = np.sort(rng.choice(np.arange(1, N), len(lev) - 1, replace=False))
        signal[c] = np.repeat(lev, np.diff(np.concatenate(([0], cuts, [N])))) + rng.normal(0.0, 0.15, N)
    flat, off = ctx._dtw_offsets(levels)
    kmax = int(Ks.max())
    dev = torch.device("cuda:0")
    d_sig, d_lev = torch.from_numpy(signal).to(dev), torch.from_numpy(flat).to(dev)
    d_bp = torch.zeros((n, kmax), dtype=torch.int32, device=dev)
    d_ok = torch.zeros(n, dtype=torch.int8, device=dev)
    d_cost = torch.zeros(n, dtype=torch.float64, device=dev)
    results = {}
    for name, wsize in (("no band", None), ("band -w 5", 5)):
        window = None if wsize is None else np.array([(N / K) * wsize for K in Ks])
        d_win = None if window is None else torch.from_numpy(window).to(dev)
        torch.cuda.synchronize()

        def once():
            ctx.dtw_segment_dev(d_sig.data_ptr(), n, N, d_lev.data_ptr(), off, rep, None if d_win is None else d_win.data_ptr(), kmax,
                                d_bp.data_ptr(), d_ok.data_ptr(), d_cost.data_ptr())
        once()
        ctx.synchronize()                                       # warm-up: code objects, the scratch allocation
        stream = torch.cuda.ExternalStream(ctx.result_stream())
        ms = []
        for _ in range(args.repeat):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            once()
            b.record(stream)
            ctx.synchronize()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        sample = rng.choice(n, min(n, 64), replace=False)
        cells = float(np.mean([feasible_cells(N, int(Ks[c]) * rep, None if window is None else window[c]) for c in sample])) * n
        med = float(np.median(ms))
        ok = d_ok.cpu().numpy().astype(bool)
        results[name] = (d_bp.cpu().numpy().copy(), ok, d_cost.cpu().numpy().copy(), window)
        print("%-10s %d chunks x %d samples, %.0f levels x %d: ms per call %s (median %.2f, min %.2f, max %.2f); %.3g feasible cells "
              "(estimated from %d chunks), %.3g cells/s; choice scratch the launches are sized for %.1f MB (all of it written without a "
              "band, fewer rows with one); %d chunks failed"
              % (name, n, N, Ks.mean(), rep, " ".join("%.2f" % v for v in ms), med, min(ms), max(ms), cells, len(sample),
                 cells / (med * 1e-3), ctx.dtw_scratch_bytes() / 1e6, int((~ok).sum())))
    # host stand-in for the reference's DTW: the numpy restatement, one thread, on a sample; it also checks the device bytes
    sample = rng.choice(n, min(n, args.host_sample), replace=False)
    for name, (bp, ok, cost, window) in results.items():
        t0 = time.perf_counter()
        for c in sample:
            want = dtw_ref.dtw(signal[c], levels[c], rep, None if window is None else float(window[c]))
            assert want[1] == ok[c] and np.array_equal(want[0], bp[c, :len(want[0])]), (name, c)
            assert np.float64(want[2]).view(np.uint64) == cost[c:c + 1].view(np.uint64)[0], (name, c)
        t = (time.perf_counter() - t0) / len(sample)
        print("%-10s host restatement (tests/dtw_ref.py, numpy, one thread; dtw-python itself is absent): %.1f ms per chunk over %d "
              "chunks, equal to the device's bytes; %d chunks would take %.0f s on one thread, %.0f s on 16"
              % (name, 1e3 * t, len(sample), n, t * n, t * n / 16))
    ctx.close()


if __name__ == "__main__":
    main()
