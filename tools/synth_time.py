#!/usr/bin/env python
"""GPU box: time of `synth` for a training-set-shaped input: 4096 DNA chunks of 3600 samples (about 400 bases, four letters,
random breakpoints) against a synthetic model of every k-mer over A C G T X Y, at the reference recipe's settings (--std-dist
truncnorm_shift_1.5_0.5 --noise-std 1.00 --variable-noise) and --prop-ubs 0.05 -- tools/spike_time.py's workload.  Four
figures, written to --out (default profiles/synth_time.txt):

  device    xb_synth_chunks_dev on resident buffers after a warm-up call, HIP events around it, every repeat's ms;
  spike     xb_spike_chunks_dev on the same buffers, the two calls alternating in one loop, and the ratio of the medians;
  command   `python -m xna_basecaller_amd synth` on a ctc-data directory in a temporary directory, wall clock, with the
            shares its own stderr reports (model, device calls including the copies);
  host      tests/synth_ref.py -- the numpy restatement of the contract (vectorised squiggle, np.sort for the medians, scalar
            samples), the stand-in for the reference's per-read numpy / scipy code -- on a sample of the chunks, scaled to
            all of them; its output equals the device's bytes.

Informational: no threshold is attached to any of them.

    python tools/synth_time.py [--chunks 4096] [--repeat 5] [--host-sample 32] [--out profiles/synth_time.txt]
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
sys.path.insert(0, os.path.join(ROOT, "tools"))
from xna_basecaller_amd import _lib  # noqa: E402
from xna_basecaller_amd import spike as sk  # noqa: E402
from spike_time import NOISE_STD, STD_DIST, make_model  # noqa: E402
from splice_time import make_dna  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--samples", type=int, default=3600)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--host-sample", type=int, default=32)
    ap.add_argument("--prop-ubs", type=float, default=0.05)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "synth_time.txt"))
    args = ap.parse_args()
    import torch
    import synth_ref
    _lib.require_gpu()
    rng = np.random.default_rng(1)
    model, dna = make_model(rng), make_dna(rng, args.chunks, args.samples)
    lines = ["python tools/synth_time.py --chunks %d --samples %d --repeat %d --host-sample %d --prop-ubs %g"
             % (args.chunks, args.samples, args.repeat, args.host_sample, args.prop_ubs)]
    rows, phi = sk.phi_table(STD_DIST)
    kw = dict(ubs_mask=3, prop=args.prop_ubs, var_prop=0.0, pad=5, dist_rows=rows, phi=phi, noise_std=NOISE_STD, variable_noise=True)
    seed, n, N, Lt = 2012, args.chunks, args.samples, dna[1].shape[1]

    # ---- device: the two _dev forms on the same resident buffers, alternating
    ctx = _lib.mapper_context(0)
    ctx.spike_model(*model)
    dev = torch.device("cuda:0")
    signal = dna[0].astype(np.float32)
    d_in = [torch.from_numpy(a).to(dev) for a in (signal, dna[1], dna[2].astype(np.int32), dna[3].view(np.int16))]

    def outputs():
        return [torch.zeros((n, N), dtype=torch.float32, device=dev), torch.zeros((n, Lt), dtype=torch.uint8, device=dev),
                torch.zeros(n, dtype=torch.int32, device=dev), torch.zeros(n, dtype=torch.float64, device=dev),
                torch.zeros(n, dtype=torch.float64, device=dev), torch.zeros(n, dtype=torch.int8, device=dev)]
    d_out = {"synth": outputs(), "spike": outputs()}
    calls = {"synth": ctx.synth_chunks_dev, "spike": ctx.spike_chunks_dev}
    torch.cuda.synchronize()

    def once(which):
        calls[which](*(t.data_ptr() for t in d_in), n, N, Lt, 0, seed, kw["ubs_mask"], kw["prop"], kw["var_prop"], kw["pad"], rows, phi,
                     NOISE_STD, True, *(t.data_ptr() for t in d_out[which]))
    for which in calls:
        once(which)
    ctx.synchronize()
    stream = torch.cuda.ExternalStream(ctx.result_stream())
    ms = {"synth": [], "spike": []}
    for _ in range(args.repeat):
        for which in calls:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            once(which)
            b.record(stream)
            ctx.synchronize()
            b.synchronize()
            ms[which].append(a.elapsed_time(b))
    got = [t.cpu().numpy() for t in d_out["synth"]]
    pasted = [t.cpu().numpy() for t in d_out["spike"]]
    assert not got[5].any() and not pasted[5].any() and np.array_equal(got[1], pasted[1]) and np.array_equal(got[2], pasted[2])
    med = {k: float(np.median(v)) for k, v in ms.items()}
    bases = int(dna[2].astype(np.int64).sum())
    lines.append("device: xb_synth_chunks_dev, %d chunks x %d samples, %d bases: ms per call %s (median %.3f); %d samples synthesised, "
                 "%d positions spiked in %d chunks" % (n, N, bases, " ".join("%.3f" % v for v in ms["synth"]), med["synth"], n * N,
                                                       int(got[2].sum()), int((got[2] > 0).sum())))
    lines.append("spike: xb_spike_chunks_dev on the same buffers, alternating with the above: ms per call %s (median %.3f); synth / spike "
                 "= %.3f" % (" ".join("%.3f" % v for v in ms["spike"]), med["spike"], med["synth"] / med["spike"]))
    t0 = time.perf_counter()
    host_form = ctx.synth_chunks(signal, dna[1], dna[2].astype(np.int32), dna[3], 0, seed, **kw)
    lines.append("device: xb_synth_chunks (host pointers: the copies both ways included), one call: %.1f ms"
                 % (1e3 * (time.perf_counter() - t0)))
    assert all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, host_form))
    ctx.close()

    # ---- host: the restatement on a sample, equal to the device's bytes
    sample = rng.choice(n, min(n, args.host_sample), replace=False)
    t0 = time.perf_counter()
    for c in sample:
        want = synth_ref.synth_chunk(signal[c], dna[1][c], dna[2][c], dna[3][c], model, int(c), seed, 3, kw["prop"], 0.0, 5, rows, phi,
                                     NOISE_STD, True)
        assert np.array_equal(want[0].view(np.uint32), got[0][c].view(np.uint32)) and np.array_equal(want[1], got[1][c]), c
        assert want[3] == got[3][c] and want[4] == got[4][c], c
    t = (time.perf_counter() - t0) / len(sample)
    lines.append("host: tests/synth_ref.py (numpy squiggle and sort, scalar samples, one thread) %.1f ms per chunk over %d chunks, equal "
                 "to the device's bytes; %d chunks would take %.1f s on one thread, %.1f s on 16"
                 % (1e3 * t, len(sample), n, t * n, t * n / 16))

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
        cmd = [sys.executable, "-m", "xna_basecaller_amd", "synth", os.path.join(tmp, "dna"), os.path.join(tmp, "out"), "-r", path,
               "--ubs", "XY", "--prop-ubs", str(args.prop_ubs), "--std-dist", STD_DIST, "--noise-std", str(NOISE_STD), "--variable-noise"]
        t0 = time.perf_counter()
        r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=900)
        wall = time.perf_counter() - t0
        if r.returncode:
            raise SystemExit(r.stderr)
        lines.append("command: python -m xna_basecaller_amd synth DNA OUT -r MODEL --ubs XY --prop-ubs %g --std-dist %s --noise-std %g "
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
