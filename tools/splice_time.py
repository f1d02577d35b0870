#!/usr/bin/env python
"""GPU box: time of `splice` for a training-set-shaped input: 4096 DNA chunks of 3600 samples (about 400 bases, four letters,
random breakpoints) against a library cut from 2048 XNA reads (template-UB-template over all 1024 five-mers, X and Y), at the
command's defaults but --prop-ubs 0.05.  Three figures, written to --out (default profiles/splice_time.txt):

  device    xb_splice_chunks_dev on resident buffers after a warm-up call, HIP events around it, every repeat's ms;
  command   `python -m xna_basecaller_amd splice` on ctc-data directories in a temporary directory, wall clock, with the
            shares its own stderr reports (library build, device calls including the copies);
  host      tests/splice_ref.py -- the plain-Python restatement of the contract, the stand-in for the reference's per-read
            Python / pandas loop -- on 64 of the chunks, scaled to all of them; its output equals the device's bytes.

Informational: no threshold is attached to any of them.

    python tools/splice_time.py [--chunks 4096] [--repeat 5] [--host-sample 64] [--out profiles/splice_time.txt]
"""
import argparse
import itertools
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from xna_basecaller_amd import _lib  # noqa: E402
from xna_basecaller_amd import splice as sp  # noqa: E402


def random_breakpoints(rng, N, L):
    return np.concatenate([np.sort(rng.choice(np.arange(1, N), L - 1, replace=False)), [N]])


def make_xna(rng, N=400):
    reads = [(list(t), ub) for ub in (5, 6) for t in itertools.product((1, 2, 3, 4), repeat=5)]
    n = len(reads)
    chunks = (rng.standard_normal((n, N)) * 1.5).astype(np.float16)
    targets, bkps = np.zeros((n, 32), np.uint8), np.zeros((n, 32), np.uint16)
    lengths = np.zeros(n, np.uint16)
    for r, (t, ub) in enumerate(reads):
        labels = [int(v) for v in rng.integers(1, 5, 3)] + t + [ub] + t + [int(v) for v in rng.integers(1, 5, 3)]
        L = len(labels)
        targets[r, :L], lengths[r], bkps[r, :L] = labels, L, random_breakpoints(rng, N, L)
    return chunks, targets, lengths, bkps


def make_dna(rng, n, N, bases=400):
    chunks = rng.standard_normal((n, N)).astype(np.float16)
    targets, bkps = np.zeros((n, 512), np.uint8), np.zeros((n, 512), np.uint16)
    lengths = rng.integers(bases - 40, bases + 41, n).astype(np.uint16)
    for c in range(n):
        L = int(lengths[c])
        targets[c, :L], bkps[c, :L] = rng.integers(1, 5, L), random_breakpoints(rng, N, L)
    return chunks, targets, lengths, bkps


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=3600)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--prop-ubs", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "splice_time.txt"))
    args = ap.parse_args()
    import torch
    import splice_ref
    _lib.require_gpu()
    rng = np.random.default_rng(1)
    xna, dna = make_xna(rng), make_dna(rng, args.chunks, args.samples)
    lines = ["python tools/splice_time.py --chunks %d --samples %d --repeat %d --host-sample %d --prop-ubs %g"
             % (args.chunks, args.samples, args.repeat, args.host_sample, args.prop_ubs)]
    t0 = time.perf_counter()
    lib = sp.build_library(*xna)
    lines.append("library: %d reads -> %d rows, %d groups, a pool of %d samples; built on the host in %.2f s"
                 % (len(xna[2]), len(lib.info), int((lib.table[:, 1] > 0).sum()), lib.pool.size, time.perf_counter() - t0))
    kw = dict(ubs_mask=3, prop=args.prop_ubs, var_prop=0.0, cand_sample_size=10, pad=5)
    seed, n, N, Lt = 2012, args.chunks, args.samples, dna[1].shape[1]

    # ---- device: the _dev form on resident buffers
    ctx = _lib.mapper_context(0)
    ctx.splice_library(lib.pool, lib.rows, lib.table)
    dev = torch.device("cuda:0")
    signal = dna[0].astype(np.float32)
    d_in = [torch.from_numpy(a).to(dev) for a in (signal, dna[1], dna[2].astype(np.int32), dna[3].view(np.int16))]
    d_out = [torch.zeros((n, N), dtype=torch.float32, device=dev), torch.zeros((n, Lt), dtype=torch.uint8, device=dev),
             torch.zeros(n, dtype=torch.int8, device=dev), torch.zeros(n, dtype=torch.int32, device=dev)]
    torch.cuda.synchronize()

    def once():
        ctx.splice_chunks_dev(*(t.data_ptr() for t in d_in), n, N, Lt, 0, seed, kw["ubs_mask"], kw["prop"], kw["var_prop"],
                              kw["cand_sample_size"], kw["pad"], *(t.data_ptr() for t in d_out))
    once()
    ctx.synchronize()
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
    got = [t.cpu().numpy() for t in d_out]
    moved = 2.0 * n * N * 4 + 2.0 * n * Lt
    lines.append("device: xb_splice_chunks_dev, %d chunks x %d samples: ms per call %s (median %.3f); %d bases inserted in %d chunks; the "
                 "rows' copy alone moves %.0f MB, %.0f GB/s at the median"
                 % (n, N, " ".join("%.3f" % v for v in ms), float(np.median(ms)), int(got[3].sum()), int(got[2].sum()), moved / 1e6,
                    moved / (float(np.median(ms)) * 1e-3) / 1e9))
    t0 = time.perf_counter()
    host_form = ctx.splice_chunks(signal, dna[1], dna[2].astype(np.int32), dna[3], 0, seed, **kw)
    lines.append("device: xb_splice_chunks (host pointers: the copies both ways included), one call: %.1f ms"
                 % (1e3 * (time.perf_counter() - t0)))
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, host_form))
    ctx.close()

    # ---- host: the restatement on a sample, equal to the device's bytes
    sample = rng.choice(n, min(n, args.host_sample), replace=False)
    t0 = time.perf_counter()
    for c in sample:
        want = splice_ref.splice_chunk(signal[c], dna[1][c], dna[2][c], dna[3][c], lib, int(c), seed, [5, 6], kw["prop"], kw["var_prop"],
                                       kw["cand_sample_size"], kw["pad"])
        assert np.array_equal(want[0].view(np.uint32), got[0][c].view(np.uint32)) and np.array_equal(want[1], got[1][c]), c
    t = (time.perf_counter() - t0) / len(sample)
    lines.append("host: tests/splice_ref.py (plain Python, one thread) %.1f ms per chunk over %d chunks, equal to the device's bytes; %d "
                 "chunks would take %.1f s on one thread, %.1f s on 16" % (1e3 * t, len(sample), n, t * n, t * n / 16))

    # ---- the whole command
    with tempfile.TemporaryDirectory() as tmp:
        for name, data in (("dna", dna), ("xna", xna)):
            os.makedirs(os.path.join(tmp, name))
            for f, a in zip(sp.FILES, data):
                np.save(os.path.join(tmp, name, f), a)
        cmd = [sys.executable, "-m", "xna_basecaller_amd", "splice", os.path.join(tmp, "dna"), os.path.join(tmp, "xna"),
               os.path.join(tmp, "out"), "--ubs", "XY", "--prop-ubs", str(args.prop_ubs)]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode:
            raise SystemExit(r.stderr)
        lines.append("command: python -m xna_basecaller_amd splice DNA XNA OUT --ubs XY --prop-ubs %g: %.2f s wall clock (interpreter "
                     "start, loading, validation, library, device, writing %d chunks as float16)" % (args.prop_ubs, wall, n))
        lines += ["command: " + ln for ln in r.stderr.strip().splitlines()]
        out = np.load(os.path.join(tmp, "out", "chunks.npy"))
        assert np.array_equal(out, got[0].astype(np.float16))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
