#!/usr/bin/env python
"""GPU box: what one head-training step costs, and its parts, written to profiles/headtrain_time.txt.

The reference's training shape: chunks of 3600 samples (T = 720), 6 bases, state length 3, features 768, label rows 480 wide
with 280 .. 470 bases, batch 64 and 384, precision mixed.  After `--warmup` untimed calls, the mean of `--repeat` calls, each
timed by the host clock around work that ends in xb_synchronize:

  step      xb_head_train_step: signal and labels from the host, everything else on the device
  encode    xb_encode_dev, blank-less
  lossgrad  xb_ctc_loss_grad_dev, reduction mean
  headgrad  xb_head_grad_dev on the encoder's own layer output (X = NULL): max |dY|, the slabs' partial products, their sum
  norm      xb_grad_norm_dev over dW and db
  adamw     xb_adamw_step_dev on W, then on b
  repack    xb_head_repack_dev

For headgrad: the share of the fp16 MFMA peak (3 products x 2 M O F flops over 2.5e15 dense fp16 flop/s) and of the HBM peak
(Y and dY read once, X's two planes read once, dW written, over 8.0e12 B/s).

For comparison the route that exists without these entry points, timed the same way: xb_encode to the host (which leaves the
layer output in the context), xb_debug_layer_output to the host, X = hi + lo to the device, torch.nn.functional.linear and
scale * tanh on the device, model.seqdist.ctc_loss on the device tensor, .backward(), clip_grad_norm_(2.0),
torch.optim.AdamW.step.  Nothing here is a threshold; the file is the record.

    python tools/headtrain_time.py [--batches 64 384] [--repeat 10] [--repeat-torch 3] [--out profiles/headtrain_time.txt]
"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from xna_basecaller_amd import _lib  # noqa: E402
from xna_basecaller_amd.crf import Model  # noqa: E402
from xna_basecaller_amd.synthetic import peaky_weights  # noqa: E402

MFMA_PEAK, HBM_PEAK = 2.5e15, 8.0e12
W_KEY, B_KEY = "encoder.9.linear.weight", "encoder.9.linear.bias"


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
    return np.asarray(out)


def fmt(t):
    t = t * 1e3
    return "%9.3f ms (mean of %d; %.3f .. %.3f)" % (t.mean(), len(t), t.min(), t.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 384])
    ap.add_argument("--chunk-len", type=int, default=3600)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--features", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=10)
    ap.add_argument("--repeat-torch", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "headtrain_time.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    nb, sl, F, L = 6, 3, args.features, args.chunk_len
    labels = list("NACGTXY")
    cfg = {"global_norm": {"state_len": sl}, "input": {"features": 1}, "model": {"package": "bonito.crf"},
           "labels": {"labels": labels},
           "encoder": {"stride": 5, "activation": "swish", "features": F, "winlen": 19, "scale": 5.0, "rnn_type": "lstm",
                       "blank_score": 2.0},
           "basecaller": {"batchsize": max(args.batches), "chunksize": L, "overlap": 500}}
    sd = peaky_weights(F, nb, seed=25)
    lines = ["head-training step on %s, T = %d, %d bases, state length %d, features %d, label rows %d wide, precision mixed"
             % (torch.cuda.get_device_name(0), L // 5, nb, sl, F, args.width),
             "library %s, sources %s" % (_lib.load().xb_version().decode(), _lib.source_digest()), ""]
    for n in args.batches:
        rng = np.random.default_rng(n)
        model = Model(cfg)
        model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
        model.to("cuda")
        ctx = model.context(L, n)
        T, O = ctx.T, ctx.C_noblank
        M = T * n
        signal = rng.standard_normal((n, L)).astype(np.float32)
        lens = rng.integers(280, 471, n).astype(np.int32)
        targets = np.zeros((n, args.width), np.uint8)
        for i in range(n):
            targets[i, :lens[i]] = rng.integers(1, nb + 1, lens[i])
        sync = ctx.synchronize

        # ---- the route without the new entry points, first: it needs the context as load_state_dict left it
        lin = torch.nn.Linear(F, O).to(dev)
        with torch.no_grad():
            lin.weight.copy_(torch.from_numpy(sd[W_KEY]))
            lin.bias.copy_(torch.from_numpy(sd[B_KEY]))
        opt = torch.optim.AdamW(lin.parameters(), lr=2e-3)

        def torch_step():
            ctx.encode(signal, expand_blanks=False)
            hi, lo = ctx.debug_layer_output(1, n)
            x = torch.from_numpy(hi.view(np.float16)).to(dev).float() + torch.from_numpy(lo.view(np.float16)).to(dev).float()
            opt.zero_grad()
            scores = (5.0 * torch.tanh(torch.nn.functional.linear(x, lin.weight, lin.bias))).contiguous()
            loss = model.seqdist.ctc_loss(scores, targets, lens)
            loss.backward()
            torch.nn.utils.clip_grad_norm_(lin.parameters(), max_norm=2.0)
            opt.step()
            torch.cuda.synchronize()

        t_torch = timed(torch_step, sync, 1, args.repeat_torch)

        # ---- the parts, on device buffers
        d_sig = torch.from_numpy(signal).to(dev)
        d_y = torch.empty((T, n, O), dtype=torch.float32, device=dev)
        d_dy = torch.empty_like(d_y)
        d_t, d_l = torch.from_numpy(targets).to(dev), torch.from_numpy(lens).to(dev)
        d_loss = torch.empty((n,), dtype=torch.float32, device=dev)
        d_p = torch.from_numpy(np.concatenate([sd[W_KEY].ravel(), sd[B_KEY]])).to(dev)
        d_g, d_m, d_v = torch.zeros_like(d_p), torch.zeros_like(d_p), torch.zeros_like(d_p)
        d_norm = torch.zeros(1, dtype=torch.float32, device=dev)
        torch.cuda.synchronize()
        OF = O * F
        off = lambda t, k: t.data_ptr() + 4 * k                                               # noqa: E731
        parts = [
            ("encode", lambda: ctx._check(ctx.lib.xb_encode_dev(ctx.h, d_sig.data_ptr(), n, 0, d_y.data_ptr()))),
            ("lossgrad", lambda: ctx.ctc_loss_grad_dev(d_y.data_ptr(), T, n, 0, d_t.data_ptr(), args.width, d_l.data_ptr(),
                                                       d_loss.data_ptr(), d_dy.data_ptr())),
            ("headgrad", lambda: ctx.head_grad_dev(d_y.data_ptr(), d_dy.data_ptr(), None, None, M, d_g.data_ptr(), off(d_g, OF))),
            ("norm", lambda: ctx.grad_norm_dev(d_g.data_ptr(), OF, off(d_g, OF), O, d_norm.data_ptr())),
            ("adamw", lambda: (ctx.adamw_step_dev(d_p.data_ptr(), d_g.data_ptr(), d_m.data_ptr(), d_v.data_ptr(), OF, 1.0, 0.99998,
                                                  0.02, 0.0316),
                               ctx.adamw_step_dev(off(d_p, OF), off(d_g, OF), off(d_m, OF), off(d_v, OF), O, 1.0, 0.99998, 0.02,
                                                  0.0316))),
            ("repack", lambda: ctx.head_repack_dev(d_p.data_ptr(), off(d_p, OF))),
        ]
        t_parts = {name: timed(fn, sync, args.warmup, args.repeat) for name, fn in parts}

        # ---- the step
        ctx.head_train_begin(sd[W_KEY], sd[B_KEY])
        t_step = timed(lambda: ctx.head_train_step(signal, targets, lens, 2e-3), sync, args.warmup, args.repeat)
        ctx.head_train_end()

        hg = t_parts["headgrad"].mean()
        flops = 3 * 2.0 * M * O * F
        moved = M * (2 * 4 * O + 2 * 2 * F) + 4 * (OF + O)
        lines.append("batch %d (M = T n = %d rows, head %d x %d)" % (n, M, O, F))
        lines.append("  step      %s" % fmt(t_step))
        for name, _ in parts:
            lines.append("  %-9s %s" % (name, fmt(t_parts[name])))
        lines.append("  headgrad: %.3g flop in the three products -> %.1f %% of the fp16 MFMA peak (%.2g flop/s); %.3g bytes that must move "
                     "-> %.1f %% of the HBM peak (%.2g B/s)" % (flops, 100 * flops / hg / MFMA_PEAK, MFMA_PEAK, moved,
                                                               100 * moved / hg / HBM_PEAK, HBM_PEAK))
        lines.append("  without the new entry points (layer output to the host, torch linear + tanh, autograd loss, torch AdamW):")
        lines.append("  torch     %s" % fmt(t_torch))
        lines.append("")
        model._drop_context()
        del d_y, d_dy, lin, opt
        torch.cuda.empty_cache()
    text = "\n".join(lines)
    print(text)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text + "\n")


if __name__ == "__main__":
    main()
