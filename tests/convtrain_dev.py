"""The device's conv training entry points (include/xna_basecaller.h: xb_conv_train_forward_dev, xb_conv_train_backward_dev) on
float32 torch tensors of the context's device, and the three layers of rnn_encoder chained around tests/toptrain_dev.py by the
public header's recipe for xb_full_train_begin.  Only the entry points compute; torch allocates.  The stream hand-over is
toptrain_dev's.  Every output starts as NaN: an element a kernel does not write fails the comparison.

  layer_forward(ctx, x, w, b, stride, tnc)            -> z, y
  layer_backward(ctx, dy, x, z, w, stride, tnc, want_dx=True) -> dx (or None), dw, db
  stack_forward(ctx, signal, conv)                    -> the stages of the three layers; x0 (T, n, F) is stages[2]["y"]
  stack_backward(ctx, stages, dy)                     -> the six gradients, in the tensors' order"""
import torch

import convtrain_ref as CR
from toptrain_dev import _call, _new


def layer_forward(ctx, x, w, b, stride, tnc):
    n, Cin, Lin = x.shape
    Cout, _, K = w.shape
    Lout = CR.out_len(Lin, K, stride)
    shape = (Lout, n, Cout) if tnc else (n, Cout, Lout)
    z, y = _new(x, *shape), _new(x, *shape)
    _call(ctx, ctx.conv_train_forward_dev, x.data_ptr(), w.data_ptr(), b.data_ptr(), n, Cin, Lin, Cout, K, stride, tnc, z.data_ptr(), y.data_ptr())
    return z, y


def layer_backward(ctx, dy, x, z, w, stride, tnc, want_dx=True):
    n, Cin, Lin = x.shape
    Cout, _, K = w.shape
    dx = _new(x, n, Cin, Lin) if want_dx else None
    dw, db = _new(x, Cout, Cin, K), _new(x, Cout)
    _call(ctx, ctx.conv_train_backward_dev, dy.data_ptr(), x.data_ptr(), z.data_ptr(), w.data_ptr(), n, Cin, Lin, Cout, K, stride, tnc,
          None if dx is None else dx.data_ptr(), dw.data_ptr(), db.data_ptr())
    return dx, dw, db


def stack_forward(ctx, signal, conv, stride=5):
    """signal (n, chunk) and conv = [w1, b1, w2, b2, w3, b3] on the device."""
    stages, x = [], signal.reshape(signal.shape[0], 1, signal.shape[1])
    for i in range(3):
        w, b = conv[2 * i], conv[2 * i + 1]
        s, tnc = (stride, 1) if i == 2 else (1, 0)
        z, y = layer_forward(ctx, x, w, b, s, tnc)
        stages.append(dict(x=x, w=w, z=z, y=y, stride=s, tnc=tnc))
        x = y
    return stages


def stack_backward(ctx, stages, dy):
    grads = [None] * 6
    for i in (2, 1, 0):
        k = stages[i]
        dx, dw, db = layer_backward(ctx, dy, k["x"], k["z"], k["w"], k["stride"], k["tnc"], want_dx=i > 0)
        grads[2 * i], grads[2 * i + 1] = dw, db
        k.update(dy=dy, dx=dx)
        dy = dx
    torch.cuda.current_stream().synchronize()
    return grads
