#!/usr/bin/env python
"""GPU box: what the fp32 products of training (csrc/xb_train_gemm.hip) reach, written to profiles/traingemm_time.txt.

The shapes a fine-tuning step of the head and the top LSTM layers would give them at the reference's training shape: chunks of
3600 samples (T = 720), features 768, 6 bases (C = 1296), batch 64 and 98, on random tensors.  After `--warmup` untimed calls, the
mean of `--repeat` calls, each timed by the host clock around work that ends in a synchronisation:

  linear   xb_linear_f32_dev: gin = x W_ih^T + b, the head's scores (tanh), dx = dgin W_ih, the head's dX = dZ W
  wgrad    xb_wgrad_f32_dev: dW_ih + db, dW_hh (operands offset by one time step), the head's dW + db
  dz       xb_head_dz_dev
  error    a 256 x 768 block of a real-shape dW_ih against float64 on the CPU, relative to the block's maximum; and the M = 20000
           shape of the tests with one running sum and with the blocks of 1024 rows that shipped, each beside torch float32 on the
           CPU -- the measurement that chose the blocked sum

with each product's TFLOP/s against the f32-input MFMA's peak (PEAK below).  A batch is a process of its own under its own time
limit (the parent never opens the GPU); the first that fails or runs out of time ends the run.  No encoder runs here: the
context gives the stream only.  Nothing here is a threshold; the file is the record.

    python tools/traingemm_time.py [--batches 64 98] [--repeat 5] [--out profiles/traingemm_time.txt]
"""
import argparse
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PEAK = 157.0                     # TFLOP/s of v_mfma_f32_16x16x4_f32 on the MI355X
STEP_LIMIT = 300                 # seconds a child may take, start of the process included
C = 1296


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
    import torch
    from xna_basecaller_amd import _lib
    _lib.require_gpu()
    F, n, T = args.features, args.batch, args.chunk_len // 5
    rows, G = T * n, 4 * F
    dev = torch.device("cuda", 0)
    ctx = _lib.Context(0, 4, 2, 32, 19, 5, 5.0, 2.0, 100, 1)
    W, R = args.warmup, args.repeat
    gen = torch.Generator(device=dev).manual_seed(n)
    rnd = lambda *s: torch.randn(s, generator=gen, device=dev)      # noqa: E731
    k = 1.0 / np.sqrt(F)
    x, w_ih, b = rnd(T, n, F), rnd(G, F) * k, rnd(G) * k
    w_l, b_l, w_iht, w_lt = rnd(C, F) * k, rnd(C) * k, rnd(F, G) * k, rnd(F, C) * k
    gin, dgin, y = torch.empty((T, n, G), device=dev), rnd(T, n, G) * 1e-3, torch.empty((T, n, F), device=dev)
    scores, dscores, dz = torch.empty((T, n, C), device=dev), rnd(T, n, C) * 1e-3, rnd(T, n, C) * 1e-3
    dw, dcol = torch.empty(G * F, device=dev), torch.empty(G, device=dev)
    torch.cuda.synchronize()
    P = lambda a: a.data_ptr()                                       # noqa: E731
    print("batch %d (T n = %d rows):" % (n, rows))

    def product(name, fn, M, N, K):
        t = timed(fn, ctx.synchronize, W, R)
        tf = 2.0 * M * N * K / np.mean(t) / 1e12
        print("  %-52s %s  %6.2f TFLOP/s = %4.1f %% of %.0f" % (name, fmt(t), tf, 100.0 * tf / PEAK, PEAK))
    product("linear gin = x W_ih^T + b     (M %d, N %d, K %d):" % (rows, G, F), lambda: ctx.linear_f32_dev(P(x), P(w_ih), P(b), rows, G, F, 0, 0.0, P(gin)), rows, G, F)
    product("linear scores, tanh           (M %d, N %d, K %d):" % (rows, C, F), lambda: ctx.linear_f32_dev(P(x), P(w_l), P(b_l), rows, C, F, 1, 5.0, P(scores)), rows, C, F)
    product("linear dx = dgin W_ih         (M %d, N %d, K %d):" % (rows, F, G), lambda: ctx.linear_f32_dev(P(dgin), P(w_iht), None, rows, F, G, 0, 0.0, P(y)), rows, F, G)
    product("linear dX = dZ W              (M %d, N %d, K %d):" % (rows, F, C), lambda: ctx.linear_f32_dev(P(dz), P(w_lt), None, rows, F, C, 0, 0.0, P(y)), rows, F, C)
    product("wgrad dW_ih, db               (M %d, N %d, K %d):" % (rows, G, F), lambda: ctx.wgrad_f32_dev(P(dgin), P(x), rows, G, F, P(dw), P(dcol)), rows, G, F)
    product("wgrad dW_hh                   (M %d, N %d, K %d):" % (rows - n, G, F), lambda: ctx.wgrad_f32_dev(P(dgin) + 4 * n * G, P(x), rows - n, G, F, P(dw), None), rows - n, G, F)
    product("wgrad head dW, db             (M %d, N %d, K %d):" % (rows, C, F), lambda: ctx.wgrad_f32_dev(P(dz), P(x), rows, C, F, P(dw), P(dcol)), rows, C, F)
    t = timed(lambda: ctx.head_dz_dev(P(scores), P(dscores), rows * C, 5.0, P(dz)), ctx.synchronize, W, R)
    print("  dz     xb_head_dz_dev (%d elements):                %s" % (rows * C, fmt(t)))
    ctx.wgrad_f32_dev(P(dgin), P(x), rows, G, F, P(dw), P(dcol))
    ctx.synchronize()
    a64 = dgin.reshape(rows, G)[:, :256].cpu().numpy().astype(np.float64)
    ref = a64.T @ x.reshape(rows, F).cpu().numpy().astype(np.float64)
    got = dw.reshape(G, F)[:256].cpu().numpy().astype(np.float64)
    t32 = (dgin.reshape(rows, G)[:, :256].t() @ x.reshape(rows, F)).cpu().numpy().astype(np.float64)
    print("  error  dW_ih[:256] at M = %d against float64: %.3g of the block's maximum (torch float32 on this device: %.3g)"
          % (rows, np.abs(got - ref).max() / np.abs(ref).max(), np.abs(t32 - ref).max() / np.abs(ref).max()))
    rng = np.random.default_rng(0)
    a, bb = rng.standard_normal((20000, 125)).astype(np.float32), rng.standard_normal((20000, 48)).astype(np.float32)
    ref = a.astype(np.float64).T @ bb.astype(np.float64)
    yard = np.abs((torch.from_numpy(a).t() @ torch.from_numpy(bb)).numpy() - ref).max() / np.abs(ref).max()
    da, db_, out = torch.tensor(a, device=dev), torch.tensor(bb, device=dev), torch.empty((125, 48), device=dev)
    torch.cuda.synchronize()
    err = []
    for name, blk in (("one running sum", 1 << 20), ("blocks of 1024 rows", None)):
        ctx.wgrad_f32_dev(P(da), P(db_), 20000, 125, 48, P(out), None, block_rows=blk)
        ctx.synchronize()
        e = np.abs(out.cpu().numpy() - ref).max() / np.abs(ref).max()
        err.append("%s %.3g (%.2f x torch float32 on the CPU)" % (name, e, e / yard))
    print("  error  wgrad M 20000, N 125, K 48: " + "; ".join(err))
    ctx.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batches", type=int, nargs="+", default=[64, 98])
    ap.add_argument("--chunk-len", type=int, default=3600)
    ap.add_argument("--features", type=int, default=768)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--repeat", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "traingemm_time.txt"))
    ap.add_argument("--batch", type=int, help=argparse.SUPPRESS)
    args = ap.parse_args()
    if args.batch:
        return step(args)
    lines = ["traingemm_time: T = %d, features %d, C = %d, fp32 on random tensors; the mean of %d calls after %d untimed ones"
             % (args.chunk_len // 5, args.features, C, args.repeat, args.warmup)]
    ok = True
    for n in args.batches:
        cmd = [sys.executable, os.path.abspath(__file__), "--batch", str(n), "--chunk-len", str(args.chunk_len), "--features", str(args.features),
               "--warmup", str(args.warmup), "--repeat", str(args.repeat)]
        try:
            out = subprocess.run(cmd, capture_output=True, text=True, timeout=STEP_LIMIT)
            lines += out.stdout.rstrip().splitlines()
            if out.returncode:
                ok = False
                lines.append("batch %d ended with status %d; nothing further was run: %s" % (n, out.returncode, out.stderr.strip().splitlines()[-1:] or ""))
        except subprocess.TimeoutExpired:
            ok = False
            lines.append("batch %d did not end within %d s; nothing further was run" % (n, STEP_LIMIT))
        if not ok:
            break
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write(text)
    sys.stdout.write(text)
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
