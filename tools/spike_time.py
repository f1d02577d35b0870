#!/usr/bin/env python
"""GPU box: time of `spike` for a training-set-shaped input: 4096 DNA chunks of 3600 samples (about 400 bases, four letters,
random breakpoints) against a synthetic model of every k-mer over A C G T X Y, at the reference recipe's settings (--std-dist
truncnorm_shift_1.5_0.5 --noise-std 1.00 --variable-noise) and --prop-ubs 0.05.  Three figures, written to --out (default
profiles/spike_time.txt):

  device    xb_spike_chunks_dev on resident buffers after a warm-up call, HIP events around it, every repeat's ms, and the
            squiggle values the selection regenerates per second (34 passes over 100 values per base);
  command   `python -m xna_basecaller_amd spike` on a ctc-data directory in a temporary directory, wall clock, with the
            shares its own stderr reports (model, device calls including the copies);
  host      tests/spike_ref.py -- the numpy restatement of the contract (vectorised squiggle, np.sort for the medians, scalar
            pastes), the stand-in for the reference's per-read numpy / scipy code -- on 64 of the chunks, scaled to all of
            them; its output equals the device's bytes.

Informational: no threshold is attached to any of them.

    python tools/spike_time.py [--chunks 4096] [--repeat 5] [--host-sample 64] [--out profiles/spike_time.txt]
"""
import argparse
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
from xna_basecaller_amd import spike as sk  # noqa: E402
from splice_time import make_dna  # noqa: E402

STD_DIST, NOISE_STD = "truncnorm_shift_1.5_0.5", 1.0


def make_model(rng):
    """Every k-mer without an N: level means 60 .. 120, stdvs 0.8 .. 3.5."""
    digits = np.stack([np.arange(sk.MODEL_KMERS) // 7 ** q % 7 for q in range(6)])
    have = (digits > 0).all(axis=0)
    mean, stdv = np.full(sk.MODEL_KMERS, np.nan), np.zeros(sk.MODEL_KMERS)
    mean[have] = np.round(rng.uniform(60.0, 120.0, int(have.sum())), 6)
    stdv[have] = np.round(rng.uniform(0.8, 3.5, int(have.sum())), 6)
    return mean, stdv


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=3600)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=64)
    ap.add_argument("--prop-ubs", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "spike_time.txt"))
    args = ap.parse_args()
    import torch
    import spike_ref
    _lib.require_gpu()
    rng = np.random.default_rng(1)
    model, dna = make_model(rng), make_dna(rng, args.chunks, args.samples)
    lines = ["python tools/spike_time.py --chunks %d --samples %d --repeat %d --host-sample %d --prop-ubs %g"
             % (args.chunks, args.samples, args.repeat, args.host_sample, args.prop_ubs)]
    rows, phi = sk.phi_table(STD_DIST)
    kw = dict(ubs_mask=3, prop=args.prop_ubs, var_prop=0.0, pad=5, dist_rows=rows, phi=phi, noise_std=NOISE_STD, variable_noise=True)
    seed, n, N, Lt = 2012, args.chunks, args.samples, dna[1].shape[1]

    # ---- device: the _dev form on resident buffers
    ctx = _lib.mapper_context(0)
    ctx.spike_model(*model)
    dev = torch.device("cuda:0")
    signal = dna[0].astype(np.float32)
    d_in = [torch.from_numpy(a).to(dev) for a in (signal, dna[1], dna[2].astype(np.int32), dna[3].view(np.int16))]
    d_out = [torch.zeros((n, N), dtype=torch.float32, device=dev), torch.zeros((n, Lt), dtype=torch.uint8, device=dev),
             torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.float64, device=dev),
             torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int8, device=dev)]
    torch.cuda.synchronize()

    def once():
        ctx.spike_chunks_dev(*(t.data_ptr() for t in d_in), n, N, Lt, 0, seed, kw["ubs_mask"], kw["prop"], kw["var_prop"], kw["pad"],
                             rows, phi, NOISE_STD, True, *(t.data_ptr() for t in d_out))
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
    assert not got[5].any()
    values = 34.0 * 100 * float(dna[2].astype(np.int64).sum())
    lines.append("device: xb_spike_chunks_dev, %d chunks x %d samples, %d bases: ms per call %s (median %.3f); %d positions spiked in %d "
                 "chunks; the selection regenerates %.3g squiggle values per call, %.3g a second at the median"
                 % (n, N, int(dna[2].sum()), " ".join("%.3f" % v for v in ms), float(np.median(ms)), int(got[2].sum()),
                    int((got[2] > 0).sum()), values, values / (float(np.median(ms)) * 1e-3)))
    t0 = time.perf_counter()
    host_form = ctx.spike_chunks(signal, dna[1], dna[2].astype(np.int32), dna[3], 0, seed, **kw)
    lines.append("device: xb_spike_chunks (host pointers: the copies both ways included), one call: %.1f ms"
                 % (1e3 * (time.perf_counter() - t0)))
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, host_form))
    ctx.close()

    # ---- host: the restatement on a sample, equal to the device's bytes
    sample = rng.choice(n, min(n, args.host_sample), replace=False)
    t0 = time.perf_counter()
    t_med = 0.0
    for c in sample:
        want = spike_ref.spike_chunk(signal[c], dna[1][c], dna[2][c], dna[3][c], model, int(c), seed, 3, kw["prop"], 0.0, 5, rows, phi,
                                     NOISE_STD, True)
        assert np.array_equal(want[0].view(np.uint32), got[0][c].view(np.uint32)) and np.array_equal(want[1], got[1][c]), c
        assert want[3] == got[3][c] and want[4] == got[4][c], c
        t1 = time.perf_counter()
        spike_ref.med_mad([int(v) for v in dna[1][c][:int(dna[2][c])]], model, seed, int(c))
        t_med += time.perf_counter() - t1
    t = (time.perf_counter() - t0 - t_med) / len(sample)
    lines.append("host: tests/spike_ref.py (numpy squiggle and sort, scalar pastes, one thread) %.1f ms per chunk over %d chunks, of "
                 "which med / mad alone (vectorised numpy) %.1f ms, equal to the device's bytes; %d chunks would take %.1f s on one "
                 "thread, %.1f s on 16" % (1e3 * t, len(sample), 1e3 * t_med / len(sample), n, t * n, t * n / 16))

    # ---- the whole command
    with tempfile.TemporaryDirectory() as tmp:
        os.makedirs(os.path.join(tmp, "dna"))
        for f, a in zip(sk.FILES, dna):
            np.save(os.path.join(tmp, "dna", f), a)
        path = os.path.join(tmp, "kmer.model")
        with open(path, "w") as fh:
            fh.write("kmer\tlevel_mean\tlevel_stdv\n")
            for k in np.flatnonzero(~np.isnan(model[0])):
                fh.write("%s\t%r\t%r\n" % (sk.index_kmer(k), float(model[0][k]), float(model[1][k])))
        cmd = [sys.executable, "-m", "xna_basecaller_amd", "spike", os.path.join(tmp, "dna"), os.path.join(tmp, "out"), "-r", path,
               "--ubs", "XY", "--prop-ubs", str(args.prop_ubs), "--std-dist", STD_DIST, "--noise-std", str(NOISE_STD), "--variable-noise"]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode:
            raise SystemExit(r.stderr)
        lines.append("command: python -m xna_basecaller_amd spike DNA OUT -r MODEL --ubs XY --prop-ubs %g --std-dist %s --noise-std %g "
                     "--variable-noise: %.2f s wall clock (interpreter start, loading, validation, model, device, writing %d chunks as "
                     "float16)" % (args.prop_ubs, STD_DIST, NOISE_STD, wall, n))
        lines += ["command: " + ln for ln in r.stderr.strip().splitlines() if ln.startswith(">")]
        out = np.load(os.path.join(tmp, "out", "chunks.npy"))
        assert np.array_equal(out, got[0].astype(np.float16))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
