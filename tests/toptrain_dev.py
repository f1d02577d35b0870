"""The device's training kernels composed into one step of the head and the top L LSTM layers, by the recipe of the public header
(include/xna_basecaller.h: xb_lstm_train_*_dev, xb_linear_f32_dev, xb_wgrad_f32_dev, xb_head_dz_dev) -- what a trainer built on
them will chain, and what tests/toptrain_ref.py restates in float64.  Only those five entry points compute; torch allocates, adds
the two biases of a layer (float32, one rounding) and transposes weights (.t().contiguous(): a copy, exact).

  forward(ctx, x0, tensors, scale)          -> the stages of the forward, `scores` (T, n, C) among them
  backward(ctx, stages, dscores)            -> the gradients, one device tensor per tensor, in the tensors' order; adds its stages
  composed_step(ctx, x0, tensors, scale, dscores) -> dict(scores, grads: numpy, the order of toptrain_ref.run; stages: every
                                               intermediate as a device tensor, so that a failure can be traced to its stage)

x0 (T, n, F), tensors (toptrain_ref's 4 L + 2) and dscores (T, n, C) are float32 torch tensors on the context's device.  Layer i
runs in direction toptrain_ref.reverse_of(L, i).  The stream hand-over is crf/lstm.py's: torch's stream is synchronised before a
call of the context, the context after it.  Every output starts as NaN: an element a kernel does not write fails the comparison."""
import torch

import toptrain_ref as TR


def _new(like, *shape):
    return torch.full(shape, float("nan"), dtype=torch.float32, device=like.device)


def _call(ctx, fn, *args):
    torch.cuda.current_stream().synchronize()         # the inputs are written; the context's stream may read them
    fn(*args)
    ctx.synchronize()                                 # ... and torch's stream the outputs


def _linear(ctx, a, w, bias, M, N, K, act, scale, out):
    """out (M, N) = act(a (M, K) w (N, K)^T + bias)"""
    assert a.numel() == M * K and tuple(w.shape) == (N, K) and out.numel() == M * N and w.is_contiguous()
    _call(ctx, ctx.linear_f32_dev, a.data_ptr(), w.data_ptr(), None if bias is None else bias.data_ptr(), M, N, K, act, scale, out.data_ptr())


def forward(ctx, x0, tensors, scale):
    L = (len(tensors) - 2) // 4
    T, n, F = x0.shape
    rows = T * n
    layers, x = [], x0
    for i in range(L):
        w_ih, w_hh, b_ih, b_hh = tensors[4 * i:4 * i + 4]
        rev = TR.reverse_of(L, i)
        bias = b_ih + b_hh                                                        # gin[t] = x_t W_ih^T + b_ih + b_hh
        gin = _new(x0, T, n, 4 * F)
        _linear(ctx, x, w_ih, bias, rows, 4 * F, F, 0, 1.0, gin)
        y, gates, c = _new(x0, T, n, F), _new(x0, T, n, 4 * F), _new(x0, T, n, F)
        _call(ctx, ctx.lstm_train_forward_dev, gin.data_ptr(), w_hh.data_ptr(), T, n, F, rev, y.data_ptr(), gates.data_ptr(), c.data_ptr())
        layers.append(dict(x=x, bias=bias, gin=gin, y=y, gates=gates, c=c, reverse=rev))
        x = y
    W, b = tensors[-2], tensors[-1]
    scores = _new(x0, T, n, W.shape[0])
    _linear(ctx, x, W, b, rows, W.shape[0], F, 1, scale, scores)                  # scale * tanh(y W^T + b)
    return dict(x0=x0, tensors=list(tensors), scale=scale, layers=layers, scores=scores)


def backward(ctx, stages, dscores):
    tensors, layers, scores, scale = stages["tensors"], stages["layers"], stages["scores"], stages["scale"]
    L = len(layers)
    T, n, F = stages["x0"].shape
    C = scores.shape[2]
    rows = T * n
    grads = [None] * len(tensors)
    top = layers[-1]["y"] if L else stages["x0"]
    dz = _new(scores, T, n, C)
    _call(ctx, ctx.head_dz_dev, scores.data_ptr(), dscores.data_ptr(), rows * C, scale, dz.data_ptr())
    grads[-2], grads[-1] = _new(scores, C, F), _new(scores, C)
    _call(ctx, ctx.wgrad_f32_dev, dz.data_ptr(), top.data_ptr(), rows, C, F, grads[-2].data_ptr(), grads[-1].data_ptr())    # the head's dW, db
    wt = tensors[-2].t().contiguous()                                             # (F, C)
    dy = _new(scores, T, n, F)
    _linear(ctx, dz, wt, None, rows, F, C, 0, 1.0, dy)                            # the head's dX = dZ W
    stages.update(dscores=dscores, dz=dz, head_wt=wt, head_dx=dy)
    for i in range(L - 1, -1, -1):
        w_ih, w_hh = tensors[4 * i], tensors[4 * i + 1]
        k = layers[i]
        rev = k["reverse"]
        dgin = _new(scores, T, n, 4 * F)
        _call(ctx, ctx.lstm_train_backward_dev, dy.data_ptr(), w_hh.data_ptr(), k["gates"].data_ptr(), k["c"].data_ptr(), T, n, F, rev, dgin.data_ptr())
        dw_ih, db, dw_hh = _new(scores, 4 * F, F), _new(scores, 4 * F), _new(scores, 4 * F, F)
        _call(ctx, ctx.wgrad_f32_dev, dgin.data_ptr(), k["x"].data_ptr(), rows, 4 * F, F, dw_ih.data_ptr(), db.data_ptr())   # dW_ih and db
        # dW_hh = sum_t dgin[t]^T y[the step processed before t]: a = dgin + n 4F, b = y forward in time; a = dgin, b = y + n F
        # in a reverse layer; M = (T - 1) n (floats of 4 bytes)
        a = dgin.data_ptr() + (0 if rev else 4 * n * 4 * F)
        b = k["y"].data_ptr() + (4 * n * F if rev else 0)
        _call(ctx, ctx.wgrad_f32_dev, a, b, (T - 1) * n, 4 * F, F, dw_hh.data_ptr(), None)
        grads[4 * i:4 * i + 4] = [dw_ih, dw_hh, db, db.clone()]                   # both biases receive dcol
        w_iht = w_ih.t().contiguous()                                             # (F, 4F)
        dx = _new(scores, T, n, F)
        _linear(ctx, dgin, w_iht, None, rows, F, 4 * F, 0, 1.0, dx)               # dx = dgin W_ih: the dy of the layer below
        k.update(dy=dy, dgin=dgin, w_iht=w_iht, dx=dx)
        dy = dx
    stages["grads"] = grads
    return grads


def composed_step(ctx, x0, tensors, scale, dscores):
    stages = forward(ctx, x0, tensors, scale)
    grads = backward(ctx, stages, dscores)
    torch.cuda.current_stream().synchronize()
    return dict(scores=stages["scores"].cpu().numpy(), grads=[g.cpu().numpy() for g in grads], stages=stages)
