"""Float64 numpy restatement of the arithmetic a fine-tuning step of the head and the top L LSTM layers has between the frozen
bottom and the optimiser (groundwork: the device has its products, xb_linear_f32 / xb_wgrad_f32 / xb_head_dz, and its
recurrences, but no trainer chains them yet), built on tests/lstm_train_ref.py: the unfrozen LSTM layers, the head
scores = scale * tanh(y W^T + b), and the gradients of every tensor from a given d loss / d scores.  x0 (the bottom's output) and
dscores are inputs: the bottom and the loss have their own references.

  reverse_of(L, i)                          -> whether unfrozen layer i (0 = lowest, encoder.(9 - L + i)) runs backwards in time
  run(x0, tensors, scale, dscores)          -> dict(scores (T, n, C), grads: one array per tensor, in the tensors' order, dx0:
                                               d loss / d x0 (T, n, F), what the layers below the unfrozen ones receive)
  torch_run(x0, tensors, scale, dscores, dtype) -> the same from torch.nn.LSTM / Linear and torch.autograd on the CPU: in float64
                                               what the restatement is held to, in float32 the yardstick of the device tests
  table(L, F, C, rows)                      -> csrc/xb_top_plan.h restated: offsets, lengths, floats of a buffer, its stride, bytes
  CASES, draw(case)                         -> the steps the device's kernels are composed at (tests/test_gpu_toptrain.py) and their
                                               float32 numpy stand-in is run at (tests/test_toptrain_host.py), and their inputs

tensors: per unfrozen layer weight_ih_l0 (4F, F), weight_hh_l0 (4F, F), bias_ih_l0 (4F), bias_hh_l0 (4F), lowest layer first; then
the head's weight (C, F) and bias (C) -- 4 L + 2 arrays, the order of csrc/xb_top_plan.h."""
import collections

import numpy as np

import lstm_train_ref as R

# A composed step: L unfrozen layers, (T, n, F) activations, C score columns; d loss / d scores is N(0, 1), times 10^U(-9, -4)
# per element where `small` (a mean loss's gradients), or None: the test supplies it (the device's own loss).
Case = collections.namedtuple("Case", "L T n F C small")
CASES = [Case(1, 7, 5, 48, 125, False),       # a ragged last column tile, score rows that are not 16-byte aligned
         Case(2, 7, 17, 48, 125, False),
         Case(3, 7, 5, 48, 125, True),
         Case(2, 4, 65, 96, 64, False),       # the recurrence's launch with four row tiles a workgroup
         Case(1, 3, 5, 768, 125, False),      # the real K
         Case(5, 6, 5, 32, 64, True),         # every layer csrc/xb_top_plan.h lays out
         Case(2, 1, 5, 48, 125, False),       # one time step: dW_hh sums over no rows
         # appended (TR.CASES[1] stays what it was): the head widths of the other (n_base, state_len) pairs a context takes
         Case(1, 7, 5, 48, 216, False),       # (6, 2)
         Case(1, 7, 5, 48, 625, True),        # (5, 3): score rows that are not 16-byte aligned
         Case(2, 5, 17, 32, 1024, False),     # (4, 4)
         Case(1, 7, 5, 48, 3125, False),      # (5, 4): not 16-byte aligned, 49 column tiles
         Case(2, 5, 5, 32, 4096, False)]      # (4, 5)
LOSS_CASE = Case(2, 40, 6, 48, 125, None)     # d loss / d scores from xb_ctc_loss_grad on the device's scores (n_base 5, state_len 2)


def case_id(c):
    return "L%d-T%d-n%d-F%d-C%d%s" % (c[:5] + ({False: "", True: "-small", None: "-loss"}[c.small],))


def draw(c):
    """(x0, tensors, dscores) of a case in float32, drawn as tests/test_toptrain_host.py draws them; dscores None for LOSS_CASE."""
    rng = np.random.default_rng(1000 * c.L + c.T + c.n + c.F + c.C)
    k = 2.0 / np.sqrt(c.F)
    tensors = []
    for _ in range(c.L):
        tensors += [rng.uniform(-k, k, (4 * c.F, c.F)), rng.uniform(-k, k, (4 * c.F, c.F)), rng.uniform(-k, k, 4 * c.F), rng.uniform(-k, k, 4 * c.F)]
    tensors += [rng.uniform(-k, k, (c.C, c.F)), rng.uniform(-k, k, c.C)]
    x0, dscores = rng.standard_normal((c.T, c.n, c.F)), rng.standard_normal((c.T, c.n, c.C))
    if c.small:
        dscores = dscores * 10.0 ** rng.uniform(-9, -4, dscores.shape)
    return x0.astype(np.float32), [a.astype(np.float32) for a in tensors], None if c.small is None else dscores.astype(np.float32)


def reverse_of(L, i):
    return (9 - L + i - 4) % 2 == 0


def run(x0, tensors, scale, dscores):
    t = [np.asarray(a, np.float64) for a in tensors]
    L = (len(t) - 2) // 4
    x = np.asarray(x0, np.float64)
    T, n, F = x.shape
    rows = T * n
    keep = []
    for i in range(L):
        w_ih, w_hh, b_ih, b_hh = t[4 * i:4 * i + 4]
        rev = reverse_of(L, i)
        y, gates, c = R.forward(x @ w_ih.T + (b_ih + b_hh), w_hh, rev)
        keep.append((x, y, gates, c, rev))
        x = y
    W, b = t[-2], t[-1]
    scores = scale * np.tanh(x @ W.T + b)
    dz = np.asarray(dscores, np.float64) * ((scale - scores) * (scale + scores) / scale)
    d2 = dz.reshape(rows, -1)
    grads = [None] * len(t)
    grads[-2], grads[-1] = d2.T @ x.reshape(rows, F), d2.sum(axis=0)
    dy = dz @ W
    for i in range(L - 1, -1, -1):
        w_ih, w_hh = t[4 * i], t[4 * i + 1]
        xin, y, gates, c, rev = keep[i]
        dgin = R.backward(dy, w_hh, gates, c, rev)
        g2 = dgin.reshape(rows, 4 * F)
        db = g2.sum(axis=0)
        grads[4 * i:4 * i + 4] = [g2.T @ xin.reshape(rows, F), g2.T @ R.h_prev(y, rev).reshape(rows, F), db, db.copy()]
        dy = dgin @ w_ih
    return dict(scores=scores, grads=grads, dx0=dy)


def torch_run(x0, tensors, scale, dscores, dtype):
    import torch
    L = (len(tensors) - 2) // 4
    F = np.asarray(x0).shape[2]
    params = [torch.from_numpy(np.asarray(a)).to(dtype).clone().requires_grad_(True) for a in tensors]
    x = torch.from_numpy(np.asarray(x0)).to(dtype)
    for i in range(L):
        rnn = torch.nn.LSTM(F, F).to(dtype)
        flat = dict(zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"), params[4 * i:4 * i + 4]))
        rev = reverse_of(L, i)
        y = torch.func.functional_call(rnn, flat, (x.flip(0) if rev else x,))[0]
        x = y.flip(0) if rev else y
    scores = scale * torch.tanh(torch.nn.functional.linear(x, params[-2], params[-1]))
    (scores * torch.from_numpy(np.asarray(dscores)).to(dtype)).sum().backward()
    return dict(scores=scores.detach().numpy(), grads=[p.grad.numpy() for p in params])


def table(L, F, C, rows):
    lens = [n for _ in range(L) for n in (4 * F * F, 4 * F * F, 4 * F, 4 * F)] + [C * F, C]
    offs = [int(v) for v in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    params = sum(lens)
    stride = (params + 3) // 4 * 4
    act = rows * (L * 6 * F + 9 * F + 3 * C)
    return dict(off=offs, len=lens, params=params, stride=stride, bytes=4 * (act + 4 * stride + L * 4 * F + max(4 * F * F, C * F)))
