#!/usr/bin/env python
"""GPU box: what one LSTM layer's training recurrence costs, written to profiles/lstmgrad_time.txt.

The reference's training shape: chunks of 3600 samples (T = 720), features 768, at batch 64 and 384, both directions.  For each,
after `--warmup` untimed calls, the mean of `--repeat` calls, each timed by the host clock around work that ends in a
synchronisation:

  forward   xb_lstm_train_forward_dev: 720 launches, y, the activated gates and c written
  backward  xb_lstm_train_backward_dev: the transpose of W_hh and 720 launches
  layer     model.encoder[i](x) and .backward() of sum(y * dy): the two calls above with torch's products around them
            (gin = x W_ih^T + b, dx, dW_ih, db by autograd; dW_hh by one matmul) and the stream hand-overs
  torch     torch.nn.LSTM on the same device, tensors and weights, forward + backward -- if it runs there; if it does not, the
            line says how it failed, and that absence is the finding

Every step is a process of its own under its own time limit (the parent never opens the GPU); the torch steps come last, and
the first step that fails or runs out of time ends the run.  Nothing here is a threshold; the file is the record: the design
pays 2 x 720 launches a layer, and these numbers decide whether a persistent form is worth building.

    python tools/lstmgrad_time.py [--batches 64 384] [--repeat 5] [--out profiles/lstmgrad_time.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

STEP_LIMIT = {"kernels": 180, "layer": 240, "torch": 240}      # seconds a step may take, start of the process included


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


def step(args):
    """One child: prints its lines."""
    import torch
    from xna_basecaller_amd import _lib
    _lib.require_gpu()
    T, F, n, reverse = args.chunk_len // 5, args.features, args.batch, bool(args.reverse)
    dev = torch.device("cuda", 0)
    g = torch.Generator(device=dev).manual_seed(n + reverse)
    k = 1.0 / np.sqrt(F)
    w_ih, w_hh = ((torch.rand((4 * F, F), generator=g, device=dev) * 2 - 1) * k for _ in range(2))
    b = (torch.rand((4 * F,), generator=g, device=dev) * 2 - 1) * k
    x = torch.randn((T, n, F), generator=g, device=dev)
    dy = torch.randn((T, n, F), generator=g, device=dev)
    tag = "batch %d, %s:" % (n, "reverse" if reverse else "forward in time")
    if args.step == "kernels":
        ctx = _lib.Context(0, 4, 2, 32, 19, 5, 5.0, 2.0, 100, 1)
        gin = torch.nn.functional.linear(x, w_ih, b)
        y, c = torch.empty_like(x), torch.empty_like(x)
        gates, dgin = torch.empty_like(gin), torch.empty_like(gin)
        torch.cuda.synchronize()
        t_f = timed(lambda: ctx.lstm_train_forward_dev(gin.data_ptr(), w_hh.data_ptr(), T, n, F, reverse, y.data_ptr(), gates.data_ptr(),
                                                       c.data_ptr()), ctx.synchronize, args.warmup, args.repeat)
        t_b = timed(lambda: ctx.lstm_train_backward_dev(dy.data_ptr(), w_hh.data_ptr(), gates.data_ptr(), c.data_ptr(), T, n, F, reverse,
                                                        dgin.data_ptr()), ctx.synchronize, args.warmup, args.repeat)
        flop_f, flop_b = 2.0 * T * n * 4 * F * F, 2.0 * T * n * 4 * F * F
        print("%s stash %.2f GB" % (tag, 4.0 * T * n * 5 * F / 1e9))
        print("  forward   xb_lstm_train_forward_dev:   %s  = %.1f us a step, %.2f TFLOP/s" % (fmt(t_f), np.mean(t_f) / T * 1e6, flop_f / np.mean(t_f) / 1e12))
        print("  backward  xb_lstm_train_backward_dev:  %s  = %.1f us a step, %.2f TFLOP/s" % (fmt(t_b), np.mean(t_b) / T * 1e6, flop_b / np.mean(t_b) / 1e12))
        ctx.close()
    elif args.step == "layer":
        from conftest import make_config
        from xna_basecaller_amd.crf import Model
        cfg = make_config(F)
        cfg["basecaller"] = {"batchsize": n, "chunksize": args.chunk_len, "overlap": 500}
        model = Model(cfg).to("cuda")
        layer = model.encoder[8 if reverse else 7].to(dev)
        with torch.no_grad():
            layer.rnn.weight_ih_l0.copy_(w_ih), layer.rnn.weight_hh_l0.copy_(w_hh), layer.rnn.bias_ih_l0.copy_(b)
        xt = x.clone().requires_grad_(True)

        def run():
            xt.grad = None
            for p in layer.parameters():
                p.grad = None
            (layer(xt) * dy).sum().backward()
        t_l = timed(run, torch.cuda.synchronize, args.warmup, args.repeat)
        print("%s\n  layer     encoder[i](x), .backward():     %s" % (tag, fmt(t_l)))
        model._drop_context()
    else:
        try:
            rnn = torch.nn.LSTM(F, F).to(dev)
            with torch.no_grad():
                rnn.weight_ih_l0.copy_(w_ih), rnn.weight_hh_l0.copy_(w_hh), rnn.bias_ih_l0.copy_(b), rnn.bias_hh_l0.zero_()
            xt = x.clone().requires_grad_(True)

            def run():
                xt.grad = None
                rnn.zero_grad(set_to_none=True)
                xin = xt.flip(0) if reverse else xt
                y = rnn(xin)[0]
                ((y.flip(0) if reverse else y) * dy).sum().backward()
            t_t = timed(run, torch.cuda.synchronize, args.warmup, args.repeat)
            print("%s\n  torch     torch.nn.LSTM (torch %s), forward + backward: %s" % (tag, torch.__version__, fmt(t_t)))
        except Exception as e:                                        # the finding: it does not run here
            print("%s\n  torch     torch.nn.LSTM (torch %s) does not run on this device: %s: %s"
                  % (tag, torch.__version__, type(e).__name__, str(e).splitlines()[0][:200] if str(e) else ""))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 384])
    ap.add_argument("--chunk-len", type=int, default=3600)
    ap.add_argument("--features", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--no-torch", action="store_true", help="skip the torch.nn.LSTM steps")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lstmgrad_time.txt"))
    ap.add_argument("--step", choices=sorted(STEP_LIMIT), help=argparse.SUPPRESS)
    ap.add_argument("--batch", type=int, help=argparse.SUPPRESS)
    ap.add_argument("--reverse", type=int, default=0, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.step:
        return step(args)
    lines = ["lstmgrad_time: T = %d, features %d, fp32; the mean of %d calls after %d untimed ones"
             % (args.chunk_len // 5, args.features, args.repeat, args.warmup)]
    ok = True
    for what in ("kernels", "layer") + (() if args.no_torch else ("torch",)):
        for n in args.batches:
            for reverse in (0, 1):
                if not ok:
                    break
                cmd = [sys.executable, os.path.abspath(__file__), "--step", what, "--batch", str(n), "--reverse", str(reverse),
                       "--chunk-len", str(args.chunk_len), "--features", str(args.features), "--warmup", str(args.warmup),
                       "--repeat", str(args.repeat)]
                try:
                    out = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT[what])
                    lines += out.stdout.rstrip().splitlines()
                    if out.returncode:
                        ok = False
                        lines.append("step %s, batch %d, reverse %d ended with status %d; nothing further was run: %s"
                                     % (what, n, reverse, out.returncode, out.stderr.strip().splitlines()[-1:] or ""))
                except subprocess.TimeoutExpired:
                    ok = False
                    lines.append("step %s, batch %d, reverse %d did not end within %d s; nothing further was run"
                                 % (what, n, reverse, STEP_LIMIT[what]))
                sys.stdout.write("\n".join(lines[-4:]) + "\n")
                sys.stdout.flush()
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    sys.stdout.write("\n" + text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
