#!/usr/bin/env python
"""GPU box: what the UB tally costs, written to profiles/ubtally_time.txt.

Two shapes, 4096 rows each: the POC library (tests/golden/poc_refdb_short.fasta) and a library of 1024 templates of 100
letters (one UB site each).  The rows are seeded calls off the templates (substitutions, indels, the UB called X / Y / a
natural letter / dropped, both strands), mapped once by xb_map_templates; then, on those rows and mapper outputs:

  kernel   xb_ub_tally_dev on device-resident inputs, `--burst` launches back to back on the context's stream and one
           xb_synchronize behind them: the time divided by the number of launches is what one launch of the kernel costs
           the stream (the launches queue faster than they run, or the figure is the launch rate -- whichever is larger);
  single   one xb_ub_tally_dev and one xb_synchronize: a launch and a synchronisation, what a caller waits for;
  host     Context.ub_tally (xb_ub_tally: upload, launch, synchronise, copy back);
  python   the plain-Python restatement of the same contract (tests/ubtally_ref.py) on the same rows, once.

Every device figure is taken `--repeat` times after one warm-up: mean, smallest, largest.  Nothing here is a threshold; the
file is the record.

    python tools/ubtally_time.py [--rows 4096] [--repeat 10] [--burst 100] [--out profiles/ubtally_time.txt]
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


def calls(templates, count, rng):
    letters = np.array(list("ACGT"))
    comp = str.maketrans("ACGTXY", "TGCAYX")
    out = []
    for _ in range(count):
        s = []
        for c in templates[rng.integers(len(templates))]:
            if c not in "ACGT":
                c = str(rng.choice(["X", "Y", "A", "", "AX"], p=[0.6, 0.1, 0.1, 0.1, 0.1]))
            v = rng.random()
            c = str(rng.choice(letters)) if v < 0.04 else "" if v < 0.07 else c + str(rng.choice(letters)) if v < 0.09 else c
            s.append(c)
        s = "".join(s)
        out.append(s[::-1].translate(comp) if rng.random() < 0.5 else s)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--burst", type=int, default=100, help="back-to-back launches behind one synchronisation")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ubtally_time.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    import torch
    import ubtally_ref
    from xna_basecaller_amd.aligner import read_fasta
    rng = np.random.default_rng(0)
    poc = [s.upper() for _, s in read_fasta(os.path.join(ROOT, "tests", "golden", "poc_refdb_short.fasta"))]
    big = []
    for _ in range(1024):
        t = list(rng.choice(np.array(list("ACGT")), 100))
        t[int(rng.integers(10, 90))] = "N"
        big.append("".join(t))
    ctx = _lib.mapper_context(0)
    lines = ["ubtally_time: %d rows per shape, %s" % (args.rows, _lib.load().xb_version().decode())]

    def clock(fn, per=1):
        fn()
        t = []
        for _ in range(args.repeat):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
        t = np.array(t) * 1e3 / per
        return "%.4f ms (mean of %d; %.4f .. %.4f)" % (t.mean(), len(t), t.min(), t.max())

    dev = torch.device("cuda:0")
    for name, templates in (("POC library", poc), ("1024 templates of 100 letters", big)):
        reads = calls(templates, args.rows, rng)
        width = -(-max(len(r) for r in reads) // 16) * 16
        rows = np.zeros((len(reads), width), np.int8)
        for k, r in enumerate(reads):
            rows[k, :len(r)] = np.frombuffer(r.encode(), np.int8)
        lens = np.array([len(r) for r in reads], np.int32)
        lib = "".join(templates).encode()
        off = np.zeros(len(templates) + 1, np.int32)
        off[1:] = np.cumsum([len(t) for t in templates])
        got = ctx.map_templates(rows, lens, lib, off)
        counts, acc = ctx.ub_tally(rows, lens, got, lib, off)
        d_rows, d_lens = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
        d_got = {k: torch.from_numpy(got[k]).to(dev) for k in ctx.UB_INPUTS}
        d_counts = torch.zeros(counts.shape, dtype=torch.int32, device=dev)
        d_acc = [torch.zeros(a.shape, dtype=getattr(torch, a.dtype.name), device=dev) for a in (acc.reads, acc.err, acc.cm)]
        torch.cuda.synchronize()

        def launches(count):
            for _ in range(count):
                ctx.ub_tally_dev(d_rows.data_ptr(), d_lens.data_ptr(), len(reads), width, {k: t.data_ptr() for k, t in d_got.items()},
                                 lib, off, d_counts.data_ptr(), *[a.data_ptr() for a in d_acc])
            ctx.synchronize()

        t_single = clock(lambda: launches(1))
        t_kernel = clock(lambda: launches(args.burst), per=args.burst)
        assert np.array_equal(d_counts.cpu().numpy(), counts)
        t_host = clock(lambda: ctx.ub_tally(rows, lens, got, lib, off))
        t0 = time.perf_counter()
        want, want_acc = ubtally_ref.tally(rows, lens, got, templates)
        t_py = (time.perf_counter() - t0) * 1e3
        assert np.array_equal(want, counts) and np.array_equal(want_acc["err"], acc.err) and np.array_equal(want_acc["cm"], acc.cm)
        lines.append("%s: %d templates, %d letters, rows of %d, %d mapped, ops rows of %d bytes" %
                     (name, len(templates), len(lib), width, int((got["tmpl"] >= 0).sum()), got["ops"].shape[1]))
        lines.append("  kernel   xb_ub_tally_dev, %d launches back to back, per launch: %s" % (args.burst, t_kernel))
        lines.append("  single   xb_ub_tally_dev, one launch + synchronise: %s" % t_single)
        lines.append("  host     xb_ub_tally (upload, launch, synchronise, copy back): %s" % t_host)
        lines.append("  python   tests/ubtally_ref.tally on the same rows, once: %.1f ms" % t_py)
    ctx.close()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
