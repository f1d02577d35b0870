#!/usr/bin/env python
"""GPU box: what the training criterion with its gradient costs, written to profiles/ctcgrad_time.txt.

The reference's training shape: chunks of 3600 samples (T = 720), 6 bases, state length 3; label rows as `basecaller --save-ctc`
writes them for such chunks -- uint8, zero-padded to a width that is a multiple of 16, here 480 wide with 280 .. 470 bases --
at batch 64 and 384, in both score layouts.  Scores 5 tanh(N(0, 1)) on the device.  For each, after `--warmup` untimed
calls, the mean of `--repeat` calls, each timed by the host clock around work that ends in xb_synchronize:

  grad   xb_ctc_loss_grad_dev: the CRF scans (logz, posteriors), the lattice kernel, the fill kernel
  scan   xb_crf_scans_dev with logz and posteriors: the first of these parts alone; grad - scan = the two new kernels
  loss   xb_ctc_loss_dev: the value alone (CRF forward scan + the forward lattice)
  host   the route the device call replaces, with-blank layout only (it has no other): model.seqdist.ctc_loss(numpy scores,
         want_grad=True) -- normalise, xb_ctc_logz with gstay / gmove to the host, np.add.at per time step, the posteriors
         pulled back, numpy arithmetic.  One untimed call at batch 64, then `--repeat-host` timed calls per batch.

The device gradient is checked bit for bit against the host route's at both batches.  The roofline line: the bytes the two new
kernels must move -- the (T, n, C) gradient written once, the (T, n, S (nb + 1)) posteriors read once -- over (grad - scan),
against the 8.0 TB/s HBM3E peak.  The kernels' own times come from a kernel trace in a run of its own (--no-host under
rocprofv3 --kernel-trace --stats).  Nothing here is a threshold; the file is the record.

    python tools/ctcgrad_time.py [--batches 64 384] [--repeat 20] [--repeat-host 1] [--out profiles/ctcgrad_time.txt]
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

HBM_PEAK = 8.0e12           # bytes / s, HBM3E specification of the MI355X


def fmt(t):
    t = np.asarray(t) * 1e3
    return "%9.3f ms (mean of %d; %.3f .. %.3f)" % (t.mean(), len(t), t.min(), t.max())


def timed(fn, sync, warmup, repeat):
    for _ in range(warmup):
        fn()
    sync()
    out = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        sync()
        out.append(time.perf_counter() - t0)
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 384])
    ap.add_argument("--chunk-len", type=int, default=3600)
    ap.add_argument("--width", type=int, default=480, help="labels per row of references")
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeat", type=int, default=20)
    ap.add_argument("--repeat-host", type=int, default=1)
    ap.add_argument("--no-host", action="store_true", help="skip the host route (kernel traces)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ctcgrad_time.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    import torch
    from conftest import make_config
    from xna_basecaller_amd.crf import Model

    labels, sl = list("NACGTXY"), 3
    nb, L, Lt, Nmax = len(labels) - 1, args.chunk_len, args.width, max(args.batches)
    cfg = make_config(32, labels)                               # the encoder is not run: a small one
    cfg["basecaller"] = {"batchsize": Nmax, "chunksize": L, "overlap": 500}
    model = Model(cfg).to("cuda")
    ctx = model.context(L, Nmax)
    T, S, E = ctx.T, ctx.S, nb + 1
    dev = torch.device("cuda", 0)
    rng = np.random.default_rng(0)
    lines = ["ctcgrad_time: chunks of %d samples, T = %d, %d bases, state length %d, label rows of %d (280 .. 470 bases), "
             "XB_CTC_SCRATCH_MB %s, %s" % (L, T, nb, sl, Lt, os.environ.get("XB_CTC_SCRATCH_MB", "unset (1024)"),
                                           _lib.load().xb_version().decode())]
    host_warm = False
    for N in args.batches:
        targets = rng.integers(1, nb + 1, (N, Lt)).astype(np.uint8)
        lens = rng.integers(280, 471, N).astype(np.int32)
        for b in range(N):
            targets[b, lens[b]:] = 0
        d_t, d_l = torch.from_numpy(targets).to(dev), torch.from_numpy(lens).to(dev)
        g = torch.Generator(device=dev).manual_seed(N)
        full = 5.0 * torch.tanh(torch.randn((T, N, S, E), generator=g, device=dev))
        full[..., 0] = ctx.cfg.blank_score
        for hb in (True, False):
            d_sc = (full if hb else full[..., 1:]).reshape(T, N, -1).contiguous()
            C = d_sc.shape[2]
            d_loss = torch.empty((N,), dtype=torch.float32, device=dev)
            d_grad = torch.empty_like(d_sc)
            d_lz = torch.empty((N,), dtype=torch.float32, device=dev)
            d_post = torch.empty((T, N, (S * E + 3) & ~3), dtype=torch.float32, device=dev)
            torch.cuda.synchronize()
            t_grad = timed(lambda: ctx.ctc_loss_grad_dev(d_sc.data_ptr(), T, N, hb, d_t.data_ptr(), Lt, d_l.data_ptr(), d_loss.data_ptr(),
                                                         d_grad.data_ptr()), ctx.synchronize, args.warmup, args.repeat)
            t_scan = timed(lambda: ctx.crf_scans_dev(d_sc.data_ptr(), T, N, hb, d_logz=d_lz.data_ptr(), d_post=d_post.data_ptr()),
                           ctx.synchronize, args.warmup, args.repeat)
            t_loss = timed(lambda: ctx.ctc_loss_dev(d_sc.data_ptr(), T, N, hb, d_t.data_ptr(), Lt, d_l.data_ptr(), d_loss.data_ptr()),
                           ctx.synchronize, args.warmup, args.repeat)
            a, s = np.mean(t_grad), np.mean(t_scan)
            moved = 4.0 * T * N * (C + S * E)
            lines.append("batch %d, %s (C = %d):" % (N, "with blank" if hb else "blank-less", C))
            lines.append("  grad  xb_ctc_loss_grad_dev:                  %s" % fmt(t_grad))
            lines.append("  scan  xb_crf_scans_dev (logz, posteriors):   %s" % fmt(t_scan))
            lines.append("  grad - scan, the lattice and the fill kernel: %8.3f ms" % ((a - s) * 1e3))
            lines.append("  loss  xb_ctc_loss_dev (the value alone):     %s" % fmt(t_loss))
            lines.append("  roofline: %.1f MB of gradient written and posteriors read in grad - scan = %.2f TB/s = %.3f of the "
                         "%.1f TB/s HBM peak" % (moved / 1e6, moved / (a - s) / 1e12, moved / (a - s) / HBM_PEAK, HBM_PEAK / 1e12))
            if hb and not args.no_host:
                sc = d_sc.cpu().numpy()
                t32 = targets.astype(np.int32)
                if not host_warm:
                    model.seqdist.ctc_loss(sc, t32, lens, want_grad=True)
                    host_warm = True
                t_host, got = [], None
                for _ in range(args.repeat_host):
                    t0 = time.perf_counter()
                    got = model.seqdist.ctc_loss(sc, t32, lens, want_grad=True)
                    t_host.append(time.perf_counter() - t0)
                ctx.ctc_loss_grad_dev(d_sc.data_ptr(), T, N, hb, d_t.data_ptr(), Lt, d_l.data_ptr(), d_loss.data_ptr(), d_grad.data_ptr())
                ctx.synchronize()
                assert np.array_equal(d_grad.cpu().numpy(), got[1]), "the device gradient and the host route's differ"
                assert abs(float(d_loss.mean()) - float(got[0])) < 1e-5
                lines.append("  host  seqdist.ctc_loss(numpy, want_grad=True): %s; host / grad = %.0f (gradients bit-equal)"
                             % (fmt(t_host), np.mean(t_host) / a))
                del sc, got
            del d_sc, d_grad, d_post
        del full
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    sys.stdout.write(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)


if __name__ == "__main__":
    main()
