"""Float64 numpy restatements of xb_lstm_train_forward_dev / xb_lstm_train_backward_dev (include/xna_basecaller.h): one
unidirectional LSTM layer's recurrence with torch's semantics (gates i, f, g, o; h_-1 = c_-1 = 0; reverse processes the time
axis downwards and stores at each step's own t), the same inputs and outputs as the entry points, and the layer composed around
them as crf/lstm.py composes it (gin by a linear map, dW_hh by a product on the shifted y).

  forward(gin, w_hh, reverse)               -> y (T, n, F), gates (T, n, 4F), c (T, n, F)
  backward(dy, w_hh, gates, c, reverse)     -> dgin (T, n, 4F)
  h_prev(y, reverse)                        -> y shifted by one processed step, zeros at the first
  layer(x, w_ih, w_hh, b, dy, reverse)      -> dict(y, dx, dw_ih, dw_hh, db)
  rel(got, ref)                             -> max |got - ref| / max |ref|: the error measure of the tests
  torch_layer(..., dtype)                   -> the same dict from torch.nn.LSTM on the CPU with torch.autograd: in float64 what the
                                               restatement is checked against, in float32 the yardstick of the device tests
"""
import numpy as np


def _order(T, reverse):
    return range(T - 1, -1, -1) if reverse else range(T)


def _sigmoid(x):
    e = np.exp(-np.abs(x))
    return np.where(x >= 0, 1.0 / (1.0 + e), e / (1.0 + e))


def forward(gin, w_hh, reverse):
    gin, w_hh = np.asarray(gin, np.float64), np.asarray(w_hh, np.float64)
    T, n, G = gin.shape
    F = G // 4
    y, gates, c = np.zeros((T, n, F)), np.zeros((T, n, G)), np.zeros((T, n, F))
    h, cc = np.zeros((n, F)), np.zeros((n, F))
    for t in _order(T, reverse):
        pre = gin[t] + h @ w_hh.T
        i, f, o = _sigmoid(pre[:, :F]), _sigmoid(pre[:, F:2 * F]), _sigmoid(pre[:, 3 * F:])
        g = np.tanh(pre[:, 2 * F:3 * F])
        cc = f * cc + i * g
        h = o * np.tanh(cc)
        gates[t], c[t], y[t] = np.concatenate([i, f, g, o], axis=1), cc, h
    return y, gates, c


def backward(dy, w_hh, gates, c, reverse):
    dy, w_hh, gates, c = (np.asarray(a, np.float64) for a in (dy, w_hh, gates, c))
    T, n, F = dy.shape
    dgin = np.zeros((T, n, 4 * F))
    order = list(_order(T, reverse))
    carry, later = np.zeros((n, F)), None
    for k in range(T - 1, -1, -1):
        t = order[k]
        i, f, g, o = (gates[t][:, a * F:(a + 1) * F] for a in range(4))
        c_prev = c[order[k - 1]] if k else np.zeros((n, F))
        dh = dy[t] + (dgin[later] @ w_hh if later is not None else 0.0)
        th = np.tanh(c[t])
        do = dh * th
        dc = dh * o * (1.0 - th * th) + carry
        di, df, dg = dc * g, dc * c_prev, dc * i
        carry = dc * f
        dgin[t] = np.concatenate([di * i * (1 - i), df * f * (1 - f), dg * (1 - g * g), do * o * (1 - o)], axis=1)
        later = t
    return dgin


def h_prev(y, reverse):
    out = np.zeros_like(y)
    if reverse:
        out[:-1] = y[1:]
    else:
        out[1:] = y[:-1]
    return out


def layer(x, w_ih, w_hh, b, dy, reverse):
    """The layer around the recurrence: gin = x W_ih^T + b; the gradients of a loss whose d loss / d y is dy."""
    x, w_ih, w_hh, b, dy = (np.asarray(a, np.float64) for a in (x, w_ih, w_hh, b, dy))
    T, n, _ = x.shape
    gin = x @ w_ih.T + b
    y, gates, c = forward(gin, w_hh, reverse)
    dgin = backward(dy, w_hh, gates, c, reverse)
    d2 = dgin.reshape(T * n, -1)
    return dict(y=y, dx=dgin @ w_ih, dw_ih=d2.T @ x.reshape(T * n, -1), dw_hh=d2.T @ h_prev(y, reverse).reshape(T * n, -1),
                db=d2.sum(axis=0))


def rel(got, ref):
    ref = np.asarray(ref, np.float64)
    m = np.abs(ref).max()
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (m if m > 0 else 1.0))


def torch_layer(x, w_ih, w_hh, b, dy, reverse, dtype):
    """torch.nn.LSTM on the CPU in `dtype`, the bias in bias_ih alone, flip / rnn / flip when reverse (nn.py:189-193), the loss
    sum(y * dy).  With x = gin, w_ih = the identity and b = 0 the input projection is exact and dx is dgin."""
    import torch
    F = np.asarray(w_hh).shape[1]
    rnn = torch.nn.LSTM(np.asarray(x).shape[2], F).to(dtype)
    with torch.no_grad():
        rnn.weight_ih_l0.copy_(torch.from_numpy(np.asarray(w_ih)))
        rnn.weight_hh_l0.copy_(torch.from_numpy(np.asarray(w_hh)))
        rnn.bias_ih_l0.copy_(torch.from_numpy(np.asarray(b)))
        rnn.bias_hh_l0.zero_()
    xt = torch.from_numpy(np.asarray(x)).to(dtype).requires_grad_(True)
    y = rnn(xt.flip(0) if reverse else xt)[0]
    y = y.flip(0) if reverse else y
    (y * torch.from_numpy(np.asarray(dy)).to(dtype)).sum().backward()
    return dict(y=y.detach().numpy(), dx=xt.grad.numpy(), dw_ih=rnn.weight_ih_l0.grad.numpy(), dw_hh=rnn.weight_hh_l0.grad.numpy(),
                db=rnn.bias_ih_l0.grad.numpy())
