#!/usr/bin/env python
"""GPU box: what the validation loss costs, written to profiles/valloss_time.txt.

One evaluate batch at the shipped config's shape: 512 chunks of 3600 samples, 6 bases, state length 3, 768 features, seeded
weights; label rows 500 wide with ragged lengths (one row full, one of state_len labels).  Three paths, each ending in a
synchronisation, after `--warmup` untimed calls, (a) and (b) alternating `--repeat` times, (c) `--repeat-old` times:

  (a) xb_validate_chunks: encoder, Viterbi decode and the loss from the device-resident scores;
  (b) xb_basecall_chunks alone: what evaluate ran without --loss;
  (c) the parent commit's route to the same three results: xb_encode to the host with the blank column, Model.seqdist.ctc_loss
      (normalise: upload + xb_crf_logz; xb_ctc_logz: upload, host gather columns, per-call allocations), then the decode of
      the host scores.

Then, from the stage times (device events around the launches) of `--repeat` calls each on device-resident blank-less
scores: xb_crf_logz_dev (the Log scan the loss starts with) and xb_ctc_loss_dev (scan + the CTC kernel); their difference is
the CTC kernel's own time, taken per workgroup size (XB_CTC_LOSS_THREADS = 64, 128, 256 and the library's rule).  (a)'s loss
is checked bit for bit against xb_ctc_loss_dev at every workgroup size and against (c)'s.  Nothing here is a threshold; the file
is the record.

    python tools/valloss_time.py [--chunks 512] [--repeat 10] [--repeat-old 2] [--out profiles/valloss_time.txt]
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


def fmt(t):
    t = np.asarray(t) * 1e3
    return "%.2f ms (mean of %d; %.2f .. %.2f)" % (t.mean(), len(t), t.min(), t.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=512)
    ap.add_argument("--chunk-len", type=int, default=3600)
    ap.add_argument("--features", type=int, default=768)
    ap.add_argument("--width", type=int, default=500, help="labels per row of references")
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--repeat-old", type=int, default=2)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "valloss_time.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    import torch
    from conftest import encoder_shapes, make_config, seeded_state_dict
    from xna_basecaller_amd.crf import Model

    labels, sl = list("NACGTXY"), 3
    nb, N, L, Lt = len(labels) - 1, args.chunks, args.chunk_len, args.width
    cfg = make_config(args.features, labels)
    cfg["basecaller"] = {"batchsize": N, "chunksize": L, "overlap": 500}
    model = Model(cfg)
    keys, shapes = encoder_shapes(args.features, nb)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(keys, shapes, 5).items()})
    model = model.to("cuda")
    ctx = model.context(L, N)
    T = ctx.T
    rng = np.random.default_rng(0)
    x = rng.standard_normal((N, L)).astype(np.float32)
    targets = rng.integers(1, nb + 1, (N, Lt)).astype(np.uint8)
    lens = rng.integers(sl, Lt + 1, N).astype(np.int32)
    lens[0], lens[-1] = Lt, sl
    for b in range(N):
        targets[b, lens[b]:] = 0
    lines = ["valloss_time: %d chunks of %d samples, T = %d, %d bases, state length %d, %d features, label rows of %d "
             "(lengths %d .. %d, mean %.0f), %s" % (N, L, T, nb, sl, args.features, Lt, lens.min(), lens.max(), lens.mean(),
                                                    _lib.load().xb_version().decode())]

    def new():
        return ctx.validate_chunks(x, labels, targets, lens)

    def plain():
        return ctx.basecall_chunks(x, labels)

    def old():
        scores = model(x[:, None, :])
        per = model.seqdist.ctc_loss(scores, targets.astype(np.int32), lens, reduction="none")
        return model.decode_batch(scores), per

    for _ in range(args.warmup):
        seq_a, len_a, loss_a = new()
        seq_b, len_b = plain()
    assert np.array_equal(seq_a, seq_b) and np.array_equal(len_a, len_b)
    ta, tb = [], []
    for _ in range(args.repeat):
        for fn, t in ((new, ta), (plain, tb)):
            t0 = time.perf_counter()
            fn()
            t.append(time.perf_counter() - t0)
    calls, per = old()                                          # warm-up of (c): its first call allocates
    assert np.array_equal(per, loss_a), "the fused loss and the host route differ"
    assert calls == [seq_a[i, :len_a[i]].tobytes().decode() for i in range(N)]
    tc = []
    for _ in range(args.repeat_old):
        t0 = time.perf_counter()
        old()
        tc.append(time.perf_counter() - t0)
    a, b, c = np.mean(ta), np.mean(tb), np.mean(tc)
    lines.append("  (a) xb_validate_chunks (calls + loss):            %s" % fmt(ta))
    lines.append("  (b) xb_basecall_chunks (calls alone):             %s" % fmt(tb))
    lines.append("  (c) xb_encode to the host + seqdist.ctc_loss + decode_batch: %s" % fmt(tc))
    lines.append("  (a) - (b), the cost of the loss: %.2f ms = %.4f of (b);  (c) / (a) = %.1f" % ((a - b) * 1e3, (a - b) / b, c / a))
    lines.append("  mean loss of the batch %.6f (bit-equal on both routes)" % float(loss_a.mean(dtype=np.float32)))

    # the kernels' own times: device events around the launches, on scores that already lie on the device
    dev = torch.device("cuda", 0)
    d_sig = torch.from_numpy(x).to(dev)
    d_sc = torch.empty((T, N, ctx.C_noblank), dtype=torch.float32, device=dev)
    d_t, d_l = torch.from_numpy(targets).to(dev), torch.from_numpy(lens).to(dev)
    d_loss = torch.empty((N,), dtype=torch.float32, device=dev)
    d_lz = torch.empty((N,), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()
    ctx.encode_dev(d_sig.data_ptr(), N, False, d_sc.data_ptr())
    ctx.synchronize()

    def stage(fn):
        fn()
        ctx.synchronize()
        ctx.set_profiling(True)
        ctx.reset_stage_times()
        for _ in range(args.repeat):
            fn()
        ctx.synchronize()
        ms = ctx.stage_times()["decode"][0] / args.repeat
        ctx.set_profiling(False)
        return ms

    scan = stage(lambda: ctx.crf_logz_dev(d_sc.data_ptr(), T, N, False, d_lz.data_ptr()))
    lines.append("  stage times, per call (mean of %d), device-resident blank-less scores:" % args.repeat)
    lines.append("    xb_crf_logz_dev (the Log scan for logz_crf):       %.3f ms" % scan)
    for threads in ("", "64", "128", "256"):
        if threads:
            os.environ["XB_CTC_LOSS_THREADS"] = threads
        else:
            os.environ.pop("XB_CTC_LOSS_THREADS", None)
        both = stage(lambda: ctx.ctc_loss_dev(d_sc.data_ptr(), T, N, False, d_t.data_ptr(), Lt, d_l.data_ptr(), d_loss.data_ptr()))
        assert np.array_equal(d_loss.cpu().numpy(), loss_a), "workgroup size %s changes the loss" % (threads or "rule")
        lines.append("    xb_ctc_loss_dev, %-22s %.3f ms; the CTC kernel alone: %.3f ms" %
                     ("%s threads per chunk:" % threads if threads else "the library's rule:", both, both - scan))
    os.environ.pop("XB_CTC_LOSS_THREADS", None)
    d_seq = torch.empty((N, T), dtype=torch.int8, device=dev)
    d_slen = torch.empty((N,), dtype=torch.int32, device=dev)
    torch.cuda.synchronize()
    full = stage(lambda: ctx.decode_dev(d_sc.data_ptr(), T, N, False, labels, None, d_seq.data_ptr(), d_slen.data_ptr()))
    lines.append("    xb_decode_dev (the Viterbi decode, for scale):     %.3f ms" % full)
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
