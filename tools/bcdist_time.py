#!/usr/bin/env python
"""GPU box: what the barcode distance costs, written to profiles/bcdist_time.txt.

Two shapes, 65536 rows each: a POC-shaped library (the barcode of 24 letters at 25) and a CPLX-shaped one (30 letters at 23),
32 templates each that share their primers and differ in the barcode.  The rows are seeded calls off the templates
(substitutions and indels inside and outside the barcode, one call in eight with the barcode garbled, both strands), mapped
once by xb_map_templates; then, on those rows and mapper outputs:

  mapper   xb_map_templates_dev on device-resident rows and one xb_synchronize: the call the distance follows, for scale;
  kernel   xb_barcode_dist_dev on device-resident inputs, `--burst` launches back to back on the context's stream and one
           xb_synchronize behind them: the time divided by the number of launches is what one launch costs the stream;
  single   one xb_barcode_dist_dev and one xb_synchronize: a launch and a synchronisation, what a caller waits for;
  host     Context.barcode_dist (xb_barcode_dist: upload, launch, synchronise, copy back);
  python   the plain-Python restatement of the same contract (tests/bcdist_ref.py) on the first `--python-rows` rows, once,
           and that time scaled to all rows.

Every device figure is taken `--repeat` times after one warm-up: mean, smallest, largest.  Nothing here is a threshold; the
file is the record, with the ratio of the kernel and of the single call to the mapper call on the same rows.

    python tools/bcdist_time.py [--rows 65536] [--repeat 10] [--burst 100] [--out profiles/bcdist_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from xna_basecaller_amd import _lib  # noqa: E402

LETTERS = np.array(list("ACGT"))


def library(rng, bc_pos, bc_len, count=32):
    head = "".join(rng.choice(LETTERS, bc_pos))
    tail = "CATGNCAAG" + "".join(rng.choice(LETTERS, 20))
    return [head + "".join(rng.choice(LETTERS, bc_len)) + tail for _ in range(count)]


def calls(templates, count, rng, bc_pos, bc_len):
    comp = str.maketrans("ACGTXY", "TGCAYX")
    out = []
    for k in range(count):
        s = []
        for c in templates[rng.integers(len(templates))]:
            if c not in "ACGT":
                c = str(rng.choice(["X", "Y", "A", ""], p=[0.7, 0.1, 0.1, 0.1]))
            v = rng.random()
            c = str(rng.choice(LETTERS)) if v < 0.04 else "" if v < 0.07 else c + str(rng.choice(LETTERS)) if v < 0.09 else c
            s.append(c)
        s = "".join(s)
        if k % 8 == 0:
            s = s[:bc_pos] + "".join(rng.choice(LETTERS, bc_len)) + s[bc_pos + bc_len:]
        out.append(s[::-1].translate(comp) if rng.random() < 0.5 else s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=65536)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--burst", type=int, default=100, help="back-to-back launches behind one synchronisation")
    ap.add_argument("--python-rows", type=int, default=2048, help="rows the Python restatement is run on")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "bcdist_time.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    import torch
    import bcdist_ref
    rng = np.random.default_rng(0)
    ctx = _lib.mapper_context(0)
    lines = ["bcdist_time: %d rows per shape, %s" % (args.rows, _lib.load().xb_version().decode())]

    def clock(fn, per=1):
        fn()
        t = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        t = np.array(t) * 1e3 / per
        return t.mean(), "%.4f ms (mean of %d; %.4f .. %.4f)" % (t.mean(), len(t), t.min(), t.max())

    dev = torch.device("cuda:0")
    scoring = (2, 4, 4, 2, 1)
    for name, bc_pos, bc_len in (("POC shape", 25, 24), ("CPLX shape", 23, 30)):
        templates = library(rng, bc_pos, bc_len)
        reads = calls(templates, args.rows, rng, bc_pos, bc_len)
        width = -(-max(len(r) for r in reads) // 16) * 16
        rows = np.zeros((len(reads), width), np.int8)
        for k, r in enumerate(reads):
            rows[k, :len(r)] = np.frombuffer(r.encode(), np.int8)
        lens = np.array([len(r) for r in reads], np.int32)
        lib = "".join(templates).encode()
        off = np.zeros(len(templates) + 1, np.int32)
        off[1:] = np.cumsum([len(t) for t in templates])
        got = ctx.map_templates(rows, lens, lib, off, scoring)
        out = ctx.barcode_dist(rows, lens, got, lib, off, bc_pos, bc_len, 3)
        n = len(reads)
        d_rows, d_lens = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
        d_map = {k: torch.zeros(got[k].shape, dtype=getattr(torch, got[k].dtype.name), device=dev) for k, _ in ctx.MAP_OUTPUTS}
        d_out = {k: torch.zeros(n, dtype=torch.int32, device=dev) for k in ctx.BC_OUTPUTS}
        torch.cuda.synchronize()

        def mapper():
            ctx.map_templates_dev(d_rows.data_ptr(), d_lens.data_ptr(), n, width, lib, off, scoring, {k: t.data_ptr() for k, t in d_map.items()})
            ctx.synchronize()

        def launches(count):
            for _ in range(count):
                ctx.barcode_dist_dev(d_rows.data_ptr(), d_lens.data_ptr(), n, width, {k: d_map[k].data_ptr() for k in ctx.BC_INPUTS},
                                     lib, off, bc_pos, bc_len, 3, {k: t.data_ptr() for k, t in d_out.items()})
            ctx.synchronize()

        m_map, t_map = clock(mapper)
        for k in ("tmpl", "strand", "q_st", "r_st"):
            assert np.array_equal(d_map[k].cpu().numpy(), got[k]), k
        m_single, t_single = clock(lambda: launches(1))
        m_kernel, t_kernel = clock(lambda: launches(args.burst), per=args.burst)
        for k in ctx.BC_OUTPUTS:
            assert np.array_equal(d_out[k].cpu().numpy(), out[k]), k
        _, t_host = clock(lambda: ctx.barcode_dist(rows, lens, got, lib, off, bc_pos, bc_len, 3))
        part = min(args.python_rows, n)
        t0 = time.perf_counter()
        want = bcdist_ref.dist(rows[:part], lens[:part], {k: v[:part] for k, v in got.items()}, templates, bc_pos, bc_len, 3)
        t_py = (time.perf_counter() - t0) * 1e3
        for k in ctx.BC_OUTPUTS:
            assert np.array_equal(want[k], out[k][:part]), k
        mapped = got["tmpl"] >= 0
        lines.append("%s: barcode of %d at %d, %d templates, %d letters, rows of %d, %d mapped, %d within 5 edits" %
                     (name, bc_len, bc_pos, len(templates), len(lib), width, int(mapped.sum()), int((out["bc_dist"][mapped] <= 5).sum())))
        lines.append("  mapper   xb_map_templates_dev + synchronise on the same rows: %s" % t_map)
        lines.append("  kernel   xb_barcode_dist_dev, %d launches back to back, per launch: %s  = %.4f of the mapper call" %
                     (args.burst, t_kernel, m_kernel / m_map))
        lines.append("  single   xb_barcode_dist_dev, one launch + synchronise: %s  = %.4f of the mapper call" % (t_single, m_single / m_map))
        lines.append("  host     xb_barcode_dist (upload, launch, synchronise, copy back): %s" % t_host)
        lines.append("  python   tests/bcdist_ref.dist on the first %d rows, once: %.1f ms; scaled to %d rows: %.0f ms" %
                     (part, t_py, n, t_py * n / part))
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
