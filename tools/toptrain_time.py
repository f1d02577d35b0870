#!/usr/bin/env python
"""GPU box: what one step of `train -F --num-unfreeze-top K --no-amp` costs for K = 2, 3, 6 (the head and the top L = K - 1 LSTM
layers), and its parts, written to profiles/toptrain_time.txt.

The reference's training shape: chunks of 3600 samples (T = 720), 6 bases, state length 3, features 768, label rows 480 wide with
280 .. 470 bases, batch 64 and 98, precision mixed.  After `--warmup` untimed calls, the mean of `--repeat` calls, each timed by the
host clock around work that ends in xb_synchronize:

  step      xb_top_train_step: signal and labels from the host, everything else on the device
  bottom    the frozen bottom pass of 5 - L LSTM layers (what xb_encode_bottom_dev runs before its join)
  join      the two fp16 planes into fp32 x0
  forward   per unfrozen layer the bias sum's place (torch adds the biases once, outside the clock), xb_linear_f32_dev for gin,
            xb_lstm_train_forward_dev; then the scores
  lossgrad  xb_ctc_loss_grad_dev, reduction mean
  backward  xb_head_dz_dev, the head's xb_wgrad_f32_dev, transpose and xb_linear_f32_dev for dX; per layer downwards the backward
            recurrence, the two weight gradients, transpose and xb_linear_f32_dev for dx
  norm      xb_grad_norm_dev over all parameters
  adamw     xb_adamw_step_dev over all parameters
  publish   TopTrainer.publish(): the masters to the host, into the model's parameters and through the host packer into the
            context (once per epoch, not per step)

With --full, per batch, the step that trains every layer (`train --no-amp` without -F: xb_full_train_begin, Model.full_trainer) and
the stages it adds to the K = 6 step: the three xb_conv_train_forward_dev in place of bottom and join, the lowest LSTM layer's dx
(transpose and xb_linear_f32_dev), the three xb_conv_train_backward_dev; for scale, the products of the five LSTM layers that
carry no recurrence (gin, dW_ih, dW_hh, dx per layer), and the torch route with nn.Conv1d + SiLU under autograd feeding it.
--append adds to the file instead of replacing it.

Beside them the route that exists without the trainer, timed the same way: the bottom's output on the device
(xb_encode_bottom_dev: the parent has no entry point for it below LSTM layer 3, so this flatters that route), the crf/lstm.py
autograd layers, torch linear + tanh, model.seqdist.ctc_loss, .backward(), clip_grad_norm_(2.0), torch.optim.AdamW.step.  Nothing
here is a threshold; the file is the record.

    python tools/toptrain_time.py [--batches 64 98] [--unfreeze 2 3 6] [--full] [--append] [--repeat 5] [--out profiles/toptrain_time.txt]
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
from xna_basecaller_amd.crf.trainer import CONV_KEYS, top_keys  # noqa: E402
from xna_basecaller_amd.synthetic import peaky_weights  # noqa: E402


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


def full_section(args, cfg, sd, n, signal, targets, lens, dev):
    """The step of every layer at batch n, the conv stages on buffers of their own, and the torch route: the lines of the report."""
    F, L_chunk, scale = args.features, args.chunk_len, 5.0
    model = Model(cfg)
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model.to("cuda")
    ctx = model.context(L_chunk, n)
    T, rows = ctx.T, ctx.T * n
    new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)                 # noqa: E731
    P = lambda t: t.data_ptr()                                                                # noqa: E731
    d_sig = torch.from_numpy(signal).to(dev)

    # ---- the torch route: Conv1d + SiLU under autograd, the crf/lstm.py autograd layers, torch linear + tanh, the autograd loss
    convs = []
    for i, (cin, cout, k, stride) in enumerate(((1, 4, 5, 1), (4, 16, 5, 1), (16, F, 19, 5))):
        conv = torch.nn.Conv1d(cin, cout, k, stride=stride, padding=k // 2).to(dev)
        with torch.no_grad():
            conv.weight.copy_(torch.from_numpy(sd[CONV_KEYS[2 * i]]))
            conv.bias.copy_(torch.from_numpy(sd[CONV_KEYS[2 * i + 1]]))
        convs.append(conv)
    layers = [model.encoder[4 + i].to(dev) for i in range(5)]
    head = model.encoder[9].to(dev)
    params = [p for m in convs + layers + [head] for p in m.parameters() if p.requires_grad]
    opt = torch.optim.AdamW(params, lr=2e-3)

    def torch_step():
        opt.zero_grad()
        x = d_sig[:, None, :]
        for conv in convs:
            x = torch.nn.functional.silu(conv(x))
        x = x.permute(2, 0, 1).contiguous()
        for layer in layers:
            x = layer(x)
        scores = (scale * torch.tanh(torch.nn.functional.linear(x, head.linear.weight, head.linear.bias))).contiguous()
        loss = model.seqdist.ctc_loss(scores, targets, lens)
        loss.backward()
        torch.nn.utils.clip_grad_norm_(params, max_norm=2.0)
        opt.step()
        torch.cuda.synchronize()

    t_torch = timed(torch_step, ctx.synchronize, args.warmup, args.repeat)
    del opt, params, convs
    model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    model.to("cuda")
    ctx = model.context(L_chunk, n)
    sync = ctx.synchronize
    torch.cuda.empty_cache()

    # ---- the conv stages, on device buffers of their own
    cw = [torch.from_numpy(sd[k].copy()).to(dev) for k in CONV_KEYS]
    cg = [torch.zeros_like(t) for t in cw]
    z1, y1, dy1 = new(n, 4, L_chunk), new(n, 4, L_chunk), new(n, 4, L_chunk)
    z2, y2, dy2 = new(n, 16, L_chunk), new(n, 16, L_chunk), new(n, 16, L_chunk)
    z3, x0, dy0 = new(T, n, F), new(T, n, F), torch.randn(T, n, F, device=dev)
    w_ih, w_hh = torch.from_numpy(sd["encoder.4.rnn.weight_ih_l0"].copy()).to(dev), torch.from_numpy(sd["encoder.4.rnn.weight_hh_l0"].copy()).to(dev)
    gin, dgin, turned, gw = new(T, n, 4 * F), torch.randn(T, n, 4 * F, device=dev), new(4 * F * F), new(4 * F, F)
    torch.cuda.synchronize()

    def lstm_products():                                    # the five layers' products that carry no recurrence
        for _ in range(5):
            ctx.linear_f32_dev(P(x0), P(w_ih), None, rows, 4 * F, F, 0, 1.0, P(gin))
            ctx.wgrad_f32_dev(P(dgin), P(x0), rows, 4 * F, F, P(gw), None)
            ctx.wgrad_f32_dev(P(dgin) + 4 * n * 4 * F, P(x0), (T - 1) * n, 4 * F, F, P(gw), None)
            ctx.transpose_f32_dev(P(w_ih), 4 * F, F, P(turned))
            ctx.linear_f32_dev(P(dgin), P(turned), None, rows, F, 4 * F, 0, 1.0, P(z3))

    def dx0():
        ctx.transpose_f32_dev(P(w_ih), 4 * F, F, P(turned))
        ctx.linear_f32_dev(P(dgin), P(turned), None, rows, F, 4 * F, 0, 1.0, P(z3))

    parts = [
        ("conv1 fwd", lambda: ctx.conv_train_forward_dev(P(d_sig), P(cw[0]), P(cw[1]), n, 1, L_chunk, 4, 5, 1, 0, P(z1), P(y1))),
        ("conv2 fwd", lambda: ctx.conv_train_forward_dev(P(y1), P(cw[2]), P(cw[3]), n, 4, L_chunk, 16, 5, 1, 0, P(z2), P(y2))),
        ("conv3 fwd", lambda: ctx.conv_train_forward_dev(P(y2), P(cw[4]), P(cw[5]), n, 16, L_chunk, F, 19, 5, 1, P(z3), P(x0))),
        ("layer0 dx", dx0),
        ("conv3 bwd", lambda: ctx.conv_train_backward_dev(P(dy0), P(y2), P(z3), P(cw[4]), n, 16, L_chunk, F, 19, 5, 1, P(dy2), P(cg[4]), P(cg[5]))),
        ("conv2 bwd", lambda: ctx.conv_train_backward_dev(P(dy2), P(y1), P(z2), P(cw[2]), n, 4, L_chunk, 16, 5, 1, 0, P(dy1), P(cg[2]), P(cg[3]))),
        ("conv1 bwd", lambda: ctx.conv_train_backward_dev(P(dy1), P(d_sig), P(z1), P(cw[0]), n, 1, L_chunk, 4, 5, 1, 0, None, P(cg[0]), P(cg[1]))),
        ("LSTM products", lstm_products),
    ]
    t_parts = {}
    for name, fn in parts:                                  # in order: each stage reads what the one before it wrote
        t_parts[name] = timed(fn, sync, args.warmup, args.repeat)
    del cw, cg, z1, y1, dy1, z2, y2, dy2, z3, x0, dy0, gin, dgin, turned, gw
    torch.cuda.empty_cache()

    trainer = model.full_trainer(L_chunk, n)
    t_step = timed(lambda: trainer.step(signal[:, None, :], targets, lens, 2e-3), sync, args.warmup, args.repeat)
    t_publish = timed(trainer.publish, sync, 1, 2)
    trainer.close()
    conv_ms = 1e3 * sum(t_parts[name].mean() for name, _ in parts[:7])
    lines = ["batch %d, every layer (`train --no-amp` without -F: 3 convolutions, 5 LSTM layers, head; %d rows, %d parameters)" % (n, rows, ctx.full_params()),
             "  step          %s" % fmt(t_step)]
    lines += ["  %-13s %s" % (name, fmt(t_parts[name])) for name, _ in parts]
    lines += ["  (conv stages and layer0 dx %9.3f ms summed: %.1f %% of the step; the LSTM layers' products without a recurrence %.3f ms)"
              % (conv_ms, 100.0 * conv_ms / (1e3 * t_step.mean()), 1e3 * t_parts["LSTM products"].mean()),
              "  publish       %s" % fmt(t_publish),
              "  without the trainer (nn.Conv1d + SiLU under autograd, crf/lstm.py autograd layers, torch linear + tanh, autograd loss, clip_grad_norm_, "
              "torch AdamW):",
              "  torch         %s" % fmt(t_torch), ""]
    print("\n".join(lines), flush=True)
    model._drop_context()
    del layers, head, model, trainer
    torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 98])
    ap.add_argument("--unfreeze", type=int, nargs="*", default=[2, 3, 6])
    ap.add_argument("--full", action="store_true", help="also the step that trains every layer, with its conv stages")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it")
    ap.add_argument("--chunk-len", type=int, default=3600)
    ap.add_argument("--width", type=int, default=480)
    ap.add_argument("--features", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "toptrain_time.txt"))
    args = ap.parse_args()
    _lib.require_gpu()
    dev = torch.device("cuda", 0)
    nb, sl, F, L_chunk = 6, 3, args.features, args.chunk_len
    cfg = {"global_norm": {"state_len": sl}, "input": {"features": 1}, "model": {"package": "bonito.crf"},
           "labels": {"labels": list("NACGTXY")},
           "encoder": {"stride": 5, "activation": "swish", "features": F, "winlen": 19, "scale": 5.0, "rnn_type": "lstm",
                       "blank_score": 2.0},
           "basecaller": {"batchsize": max(args.batches), "chunksize": L_chunk, "overlap": 500}}
    sd = peaky_weights(F, nb, seed=25)
    scale = 5.0
    lines = ["top-layer training step on %s, T = %d, %d bases, state length %d, features %d, label rows %d wide, precision mixed"
             % (torch.cuda.get_device_name(0), L_chunk // 5, nb, sl, F, args.width),
             "library %s, sources %s" % (_lib.load().xb_version().decode(), _lib.source_digest()), ""]
    for n in args.batches:
        rng = np.random.default_rng(n)
        signal = rng.standard_normal((n, L_chunk)).astype(np.float32)
        lens = rng.integers(280, 471, n).astype(np.int32)
        targets = np.zeros((n, args.width), np.uint8)
        for i in range(n):
            targets[i, :lens[i]] = rng.integers(1, nb + 1, lens[i])
        for K in args.unfreeze:
            L = K - 1
            model = Model(cfg)
            model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
            model.to("cuda")
            ctx = model.context(L_chunk, n)
            T, C = ctx.T, ctx.C_noblank
            rows = T * n
            sync = ctx.synchronize
            new = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)         # noqa: E731
            d_sig, d_x0 = torch.from_numpy(signal).to(dev), new(T, n, F)
            torch.cuda.synchronize()

            # ---- the route without the trainer, first: it moves the layers' parameters to the device
            layers = [model.encoder[9 - L + i].to(dev) for i in range(L)]
            head = model.encoder[9].to(dev)
            params = [p for m in layers + [head] for p in m.parameters() if p.requires_grad]
            opt = torch.optim.AdamW(params, lr=2e-3)

            def torch_step():
                ctx.encode_bottom_dev(d_sig.data_ptr(), n, 5 - L, d_x0.data_ptr())
                ctx.synchronize()
                opt.zero_grad()
                x = d_x0
                for layer in layers:
                    x = layer(x)
                scores = (scale * torch.tanh(torch.nn.functional.linear(x, head.linear.weight, head.linear.bias))).contiguous()
                loss = model.seqdist.ctc_loss(scores, targets, lens)
                loss.backward()
                torch.nn.utils.clip_grad_norm_(params, max_norm=2.0)
                opt.step()
                torch.cuda.synchronize()

            t_torch = timed(torch_step, sync, args.warmup, args.repeat)
            del opt, params
            model.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})        # the pretrained floats again
            model.to("cuda")
            ctx = model.context(L_chunk, n)
            sync = ctx.synchronize
            torch.cuda.empty_cache()

            # ---- the parts, on device buffers of their own
            w = [torch.from_numpy(sd[k].copy()).to(dev) for k in top_keys(L)]
            bias = [w[4 * i + 2] + w[4 * i + 3] for i in range(L)]
            gin, dgin, dy = new(T, n, 4 * F), new(T, n, 4 * F), new(T, n, F)
            ys, gates, cs = [new(T, n, F) for _ in range(L)], [new(T, n, 4 * F) for _ in range(L)], [new(T, n, F) for _ in range(L)]
            scores, dscores, dz = new(T, n, C), new(T, n, C), new(T, n, C)
            grads = [torch.zeros_like(t) for t in w]
            turned = new(4 * F * F)
            d_t, d_l, d_loss = torch.from_numpy(targets).to(dev), torch.from_numpy(lens).to(dev), new(n)
            flat = torch.cat([t.reshape(-1) for t in w])
            d_g, d_m, d_v, d_norm = torch.zeros_like(flat), torch.zeros_like(flat), torch.zeros_like(flat), new(1)
            torch.cuda.synchronize()
            P = lambda t: t.data_ptr()                                                        # noqa: E731
            rev = [(9 - L + i - 4) % 2 == 0 for i in range(L)]

            def forward():
                x = d_x0
                for i in range(L):
                    ctx.linear_f32_dev(P(x), P(w[4 * i]), P(bias[i]), rows, 4 * F, F, 0, 1.0, P(gin))
                    ctx.lstm_train_forward_dev(P(gin), P(w[4 * i + 1]), T, n, F, rev[i], P(ys[i]), P(gates[i]), P(cs[i]))
                    x = ys[i]
                ctx.linear_f32_dev(P(x), P(w[-2]), P(w[-1]), rows, C, F, 1, scale, P(scores))

            def backward():
                top = ys[-1]
                ctx.head_dz_dev(P(scores), P(dscores), rows * C, scale, P(dz))
                ctx.wgrad_f32_dev(P(dz), P(top), rows, C, F, P(grads[-2]), P(grads[-1]))
                ctx.transpose_f32_dev(P(w[-2]), C, F, P(turned))
                ctx.linear_f32_dev(P(dz), P(turned), None, rows, F, C, 0, 1.0, P(dy))
                for i in range(L - 1, -1, -1):
                    xin = ys[i - 1] if i else d_x0
                    ctx.lstm_train_backward_dev(P(dy), P(w[4 * i + 1]), P(gates[i]), P(cs[i]), T, n, F, rev[i], P(dgin))
                    ctx.wgrad_f32_dev(P(dgin), P(xin), rows, 4 * F, F, P(grads[4 * i]), P(grads[4 * i + 2]))
                    a = P(dgin) + (0 if rev[i] else 4 * n * 4 * F)
                    b = P(ys[i]) + (4 * n * F if rev[i] else 0)
                    ctx.wgrad_f32_dev(a, b, (T - 1) * n, 4 * F, F, P(grads[4 * i + 1]), None)
                    if i:
                        ctx.transpose_f32_dev(P(w[4 * i]), 4 * F, F, P(turned))
                        ctx.linear_f32_dev(P(dgin), P(turned), None, rows, F, 4 * F, 0, 1.0, P(dy))

            parts = [
                ("bottom", lambda: ctx.bottom_part_dev(P(d_sig), n, 5 - L, P(d_x0), 1)),
                ("join", lambda: ctx.bottom_part_dev(P(d_sig), n, 5 - L, P(d_x0), 2)),
                ("forward", forward),
                ("lossgrad", lambda: ctx.ctc_loss_grad_dev(P(scores), T, n, 0, P(d_t), args.width, P(d_l), P(d_loss), P(dscores))),
                ("backward", backward),
                ("norm", lambda: ctx.grad_norm_dev(P(d_g), flat.numel(), None, 0, P(d_norm))),
                ("adamw", lambda: ctx.adamw_step_dev(P(flat), P(d_g), P(d_m), P(d_v), flat.numel(), 1.0, 0.99998, 0.02, 0.0316)),
            ]
            t_parts = {name: timed(fn, sync, args.warmup, args.repeat) for name, fn in parts}
            del w, bias, gin, dgin, dy, ys, gates, cs, scores, dscores, dz, grads, turned, flat, d_g, d_m, d_v
            torch.cuda.empty_cache()

            # ---- the step
            trainer = model.top_trainer(L, L_chunk, n)
            t_step = timed(lambda: trainer.step(signal[:, None, :], targets, lens, 2e-3), sync, args.warmup, args.repeat)
            t_publish = timed(trainer.publish, sync, 1, 2)
            trainer.close()

            lines.append("batch %d, --num-unfreeze-top %d (head + %d LSTM layer%s, %d rows, %d parameters)"
                         % (n, K, L, "" if L == 1 else "s", rows, ctx.top_params(L)))
            lines.append("  step      %s" % fmt(t_step))
            for name, _ in parts:
                lines.append("  %-9s %s" % (name, fmt(t_parts[name])))
            lines.append("  (parts    %9.3f ms summed)" % (1e3 * sum(t_parts[name].mean() for name, _ in parts)))
            lines.append("  publish   %s" % fmt(t_publish))
            lines.append("  without the trainer (bottom output on the device, crf/lstm.py autograd layers, torch linear + tanh, autograd loss, "
                         "clip_grad_norm_, torch AdamW):")
            lines.append("  torch     %s" % fmt(t_torch))
            lines.append("")
            print("\n".join(lines[-14:]), flush=True)
            model._drop_context()
            del layers, head, model, trainer
            torch.cuda.empty_cache()
        if args.full:
            lines += full_section(args, cfg, sd, n, signal, targets, lens, dev)
    text = "\n".join(lines)
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "a" if args.append else "w") as f:
        f.write(text + "\n")
    print("wrote", args.out)


if __name__ == "__main__":
    main()
