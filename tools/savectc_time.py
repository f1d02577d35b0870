#!/usr/bin/env python
"""GPU box: what `basecaller --save-ctc` costs per chunk, written to profiles/savectc_time.txt.

4096 chunks of 3600 samples (seeded noise through the shipped architecture with synthetic.peaky_weights: the calls follow the
signal but are arbitrary, so few chunks are kept -- the time does not depend on that) against the POC template library, in
batches of 512:

  fused      Context.ctc_chunks per batch (xb_ctc_chunks: basecall, mapper, verdict and label row, one synchronisation);
  separate   the path a user had before the flag: crf.basecall.basecall on the chunks, aligner.align_map, i.e. a Mapping built
             on the host for EVERY chunk, kept or not;
  labels     xb_ctc_targets_dev alone on the device-resident mapper outputs of all 4096 rows: a host clock around each call,
             ended by xb_synchronize, so it holds one launch and one synchronisation, not the kernel alone.

Every figure is a host clock around work that ends in a device synchronise, after one warm-up of the same shape, taken
`--repeat` times (`--label-repeat` for the label kernel): mean, and the smallest and largest of the repeats.  The kernels' own
times come from a kernel trace: run this script under `rocprofv3 --kernel-trace --stats --output-format csv -d DIR --` and pass
the resulting *kernel_stats.csv with --stats to have the label kernel and the mapper's two printed.  Nothing here is a
threshold; the file is the record.

    python tools/savectc_time.py [--chunks 4096] [--batch 512] [--repeat 5] [--out profiles/savectc_time.txt]
    python tools/savectc_time.py --stats DIR/.../*_kernel_stats.csv
"""
import argparse
import csv
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xna_basecaller_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=4096)
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--chunksize", type=int, default=3600)
    ap.add_argument("--features", type=int, default=768)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--label-repeat", type=int, default=20)
    ap.add_argument("--stats", help="rocprofv3 kernel_stats.csv of an earlier run of this script: prints the kernels' times")
    ap.add_argument("--reference", default=os.path.join(ROOT, "tests", "golden", "poc_refdb_short.fasta"))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "savectc_time.txt"))
    args = ap.parse_args()
    if args.stats:
        for row in csv.DictReader(open(args.stats)):
            if "ctc_targets" in row["Name"] or "map_" in row["Name"]:
                print("%-60s calls %4s  average %.4f ms  min %.4f  max %.4f" % (row["Name"][:60], row["Calls"],
                      float(row["AverageNs"]) * 1e-6, float(row.get("MinNs", "nan")) * 1e-6, float(row.get("MaxNs", "nan")) * 1e-6))
        return
    _lib.require_gpu()
    import torch
    from xna_basecaller_amd.aligner import TemplateAligner, align_map
    from xna_basecaller_amd.crf.basecall import basecall, basecall_ctc
    from xna_basecaller_amd.crf.model import Model
    from xna_basecaller_amd.reads import SyntheticRead
    from xna_basecaller_amd.synthetic import peaky_weights

    labels = list("NACGTXY")
    config = {"global_norm": {"state_len": 3}, "input": {"features": 1}, "model": {"package": "bonito.crf"},
              "labels": {"labels": labels},
              "encoder": {"stride": 5, "activation": "swish", "features": args.features, "winlen": 19, "scale": 5.0,
                          "rnn_type": "lstm", "blank_score": 2.0},
              "basecaller": {"batchsize": args.batch, "chunksize": args.chunksize, "overlap": 500}}
    model = Model(config)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in peaky_weights(args.features, len(labels) - 1, 3).items()})
    model.to("cuda")
    aligner = TemplateAligner.from_config(args.reference, config, context=lambda: model._ctx)
    rng = np.random.default_rng(0)
    signal = rng.standard_normal((args.chunks, args.chunksize)).astype(np.float32)
    chunks = [SyntheticRead("chunk-%d" % i, signal[i]) for i in range(args.chunks)]
    lines = ["savectc_time: %d chunks of %d samples, batch %d, features %d, library %s (%d templates, %d letters), %s"
             % (args.chunks, args.chunksize, args.batch, args.features, os.path.basename(args.reference), len(aligner.templates),
                len(aligner.library), _lib.load().xb_version().decode())]

    def clock(fn, repeat=args.repeat):
        """The last result and the seconds of each of `repeat` runs."""
        times = []
        for _ in range(repeat):
            t0 = time.perf_counter()
            out = fn()
            times.append(time.perf_counter() - t0)
        return out, np.array(times)

    def figures(t, per=args.chunks, unit="ms per chunk"):
        return "%.3f s = %.3f %s (mean of %d; %.3f .. %.3f)" % (t.mean(), t.mean() / per * 1e3, unit, len(t), t.min() / per * 1e3,
                                                                 t.max() / per * 1e3)

    # fused: warm one batch, then the whole set
    list(basecall_ctc(model, aligner, chunks[:args.batch], batchsize=args.batch))
    fused, t_fused = clock(lambda: list(basecall_ctc(model, aligner, chunks, batchsize=args.batch)))
    kept = sum(1 for _, r in fused if r["verdict"] == 0)
    mapped = sum(1 for _, r in fused if not r["verdict"] & 3)
    lines.append("fused     basecall_ctc (xb_ctc_chunks per batch; a Mapping for the %d kept of %d mapped chunks): %s"
                 % (kept, mapped, figures(t_fused)))
    ctx = model.context(args.chunksize, args.batch)
    _, t_call = clock(lambda: [ctx.ctc_chunks(signal[a:a + args.batch], labels, aligner.library, aligner.offsets, aligner.scoring)
                               for a in range(0, args.chunks, args.batch)])
    lines.append("fused     Context.ctc_chunks alone, %d calls: %s" % (-(-args.chunks // args.batch), figures(t_call)))

    # the separate path: basecall, then align_map (a Mapping for every chunk)
    def separate(cs):
        return list(align_map(aligner, basecall(model, cs, chunksize=args.chunksize, overlap=500, batchsize=args.batch), batch=args.batch))
    separate(chunks[:args.batch])
    sep, t_sep = clock(lambda: separate(chunks))
    assert [r["sequence"] for _, r in sep] == [r["sequence"] for _, r in fused], "the two paths called different sequences"
    lines.append("separate  basecall + align_map (a Mapping for each of the %d mapped chunks): %s; fused is %.2fx"
                 % (sum(1 for _, r in sep if r["mapping"] is not None), figures(t_sep), t_sep.mean() / t_fused.mean()))
    _, t_base = clock(lambda: list(basecall(model, chunks, chunksize=args.chunksize, overlap=500, batchsize=args.batch)))
    lines.append("          of which basecall alone: %s" % figures(t_base))

    # the label kernel alone, device-resident inputs of all rows
    out = [ctx.ctc_chunks(signal[a:a + args.batch], labels, aligner.library, aligner.offsets, aligner.scoring)
           for a in range(0, args.chunks, args.batch)]
    dev = torch.device("cuda:0")
    cat = {k: np.concatenate([o[k] for o in out]) for k in out[0]}
    d_len = torch.from_numpy(cat["seq_len"]).to(dev)
    d_in = {k: torch.from_numpy(cat[k]).to(dev) for k in ctx.CTC_INPUTS}
    d_out = {k: torch.zeros(cat[k].shape, dtype=getattr(torch, np.dtype(dt).name), device=dev) for k, dt in ctx.CTC_OUTPUTS}
    torch.cuda.synchronize()

    def once():
        ctx.ctc_targets_dev(d_len.data_ptr(), args.chunks, ctx.T, {k: t.data_ptr() for k, t in d_in.items()}, aligner.library,
                            aligner.offsets, {k: t.data_ptr() for k, t in d_out.items()})
        ctx.synchronize()
    once()
    _, t_lab = clock(once, args.label_repeat)
    assert np.array_equal(d_out["verdict"].cpu().numpy(), cat["verdict"])
    moved = cat["ops"].nbytes + cat["target"].nbytes
    lines.append("labels    xb_ctc_targets_dev over %d rows (ops rows of %d bytes, label rows of %d; rows hold %.1f MB), launch + "
                 "synchronise: %.3f ms per call (mean of %d; %.3f .. %.3f)"
                 % (args.chunks, cat["ops"].shape[1], cat["target"].shape[1], moved / 1e6, t_lab.mean() * 1e3, len(t_lab),
                    t_lab.min() * 1e3, t_lab.max() * 1e3))
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    aligner.close()


if __name__ == "__main__":
    main()
