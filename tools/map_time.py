#!/usr/bin/env python
"""GPU box: time of xb_map_templates (the mapper behind `basecaller --reference`) for a POC-shaped library (20 templates of
106) and a CPLX-short-shaped one (1024 of 89) at 4096 reads, score pass and trace pass apart, and what mapping 512 reads adds
to a basecall step of 512 chunks.

The wall time of a call is taken around the device-pointer form (warm, xb_synchronize on both sides).  The split between
the two kernels comes from a kernel trace: run this script under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --`
and pass the resulting *kernel_stats.csv with --stats to have the split printed beside the wall times.

    python tools/map_time.py [--reads 4096] [--step-ms MS] [--stats kernel_stats.csv]
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from xna_basecaller_amd import _lib  # noqa: E402


def library(rng, count, length):
    letters = np.array(list("ACGTN"))
    return ["".join(rng.choice(letters, length, p=[0.245, 0.245, 0.245, 0.245, 0.02])) for _ in range(count)]


def reads_of(rng, templates, n):
    """Template-derived reads with a few errors and short flanks, both strands: about as long as a template."""
    comp = str.maketrans("ACGTN", "TGCAN")
    letters = np.array(list("ACGT"))
    out = []
    for _ in range(n):
        t = list(templates[rng.integers(len(templates))])
        for k in rng.integers(0, len(t), 4):
            t[k] = str(rng.choice(letters))
        s = "".join(rng.choice(letters, rng.integers(0, 8))) + "".join(t).replace("N", "X") + "".join(rng.choice(letters, rng.integers(0, 8)))
        out.append(s[::-1].translate(comp) if rng.random() < 0.5 else s)
    return out


def time_library(ctx, name, templates, reads, repeat):
    import torch
    width = -(-max(len(r) for r in reads) // 16) * 16
    rows = np.zeros((len(reads), width), np.int8)
    for r, s in enumerate(reads):
        rows[r, :len(s)] = np.frombuffer(s.encode(), np.int8)
    lens = np.array([len(s) for s in reads], np.int32)
    lib = "".join(templates).encode()
    off = np.zeros(len(templates) + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in templates])
    dev = torch.device("cuda:0")
    d_seq, d_len = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
    lmax = max(len(t) for t in templates)
    d_out = {k: torch.zeros((len(reads), width + lmax) if k == "ops" else (len(reads),), dtype=getattr(torch, np.dtype(dt).name), device=dev)
             for k, dt in ctx.MAP_OUTPUTS}
    torch.cuda.synchronize()
    ptrs = {k: v.data_ptr() for k, v in d_out.items()}

    def once():
        ctx.map_templates_dev(d_seq.data_ptr(), d_len.data_ptr(), len(reads), width, lib, off, (2, 4, 4, 2, 1), ptrs)
        ctx.synchronize()

    once()
    t0 = time.perf_counter()
    for _ in range(repeat):
        once()
    ms = (time.perf_counter() - t0) / repeat * 1e3
    cells = 2.0 * float(lens.sum()) * float(off[-1])
    mapped = int((d_out["tmpl"].cpu().numpy() >= 0).sum())
    print("%-10s %4d templates x %3d, %d reads (mean %.0f letters): %.2f ms per call, %.3g cells, %.3g cells/s; %d mapped"
          % (name, len(templates), lmax, len(reads), lens.mean(), ms, cells, cells / (ms * 1e-3), mapped))
    return ms, cells


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reads", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--step-ms", type=float, default=None, help="ms of a basecall step of 512 chunks (bench.py) to compare with")
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of an earlier run of this script: prints the kernels' times")
    args = ap.parse_args()
    if args.stats:
        for row in csv.DictReader(open(args.stats)):
            if "map_" in row["Name"]:
                print("%-60s calls %4s  average %.3f ms" % (row["Name"][:60], row["Calls"], float(row["AverageNs"]) * 1e-6))
        return
    _lib.require_gpu()
    ctx = _lib.Context(0, 4, 3, 32, 19, 5, 5.0, 2.0, 200, 1)
    rng = np.random.default_rng(1)
    shapes = (("POC", library(rng, 20, 106)), ("CPLX-short", library(rng, 1024, 89)))
    for name, templates in shapes:
        time_library(ctx, name, templates, reads_of(rng, templates, args.reads), args.repeat)
    for name, templates in shapes:
        ms, _ = time_library(ctx, name + "/512", templates, reads_of(rng, templates, 512), args.repeat)
        if args.step_ms:
            print("%-10s mapping 512 reads adds %.2f ms to a basecall step of %.1f ms at batch 512: %.1f %%"
                  % (name, ms, args.step_ms, 100.0 * ms / args.step_ms))
    ctx.close()


if __name__ == "__main__":
    main()
