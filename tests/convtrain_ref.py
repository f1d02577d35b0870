"""Float64 numpy restatement of one `Convolution` layer of rnn_encoder in training -- Conv1d(Cin, Cout, K, stride, padding = K // 2,
bias) followed by swish -- as csrc/xb_conv_train.hip computes it on the device (include/xna_basecaller.h: xb_conv_train_*_dev), and
of the layout header csrc/xb_conv_plan.h.

  CASES, case_id, draw(case)        -> the layers the device is held to (tests/test_gpu_convtrain.py) and their float32 numpy
                                       stand-in is run at (tests/test_convtrain_host.py), and their float32 inputs (x, w, b, dy)
  out_len(Lin, K, stride)
  forward(x, w, b, stride)          -> z, y: (n, Cout, Lout)
  backward(dy, x, z, w, stride)     -> dx, dw, db
  torch_run(x, w, b, dy, stride, dtype) -> dict(z, y, dx, dw, db) from torch.nn.functional.conv1d + silu and autograd on the CPU: in
                                       float64 what the restatement is held to, in float32 the yardstick of the device tests
  tnc(a), untnc(a)                  -> (n, Cout, Lout) <-> (Lout, n, Cout), the layout conv3 writes for the LSTM layers
  is_narrow(Cin, Cout, K, stride), narrow_blocks(...), table(chunk, F, W, S, n) -> csrc/xb_conv_plan.h restated"""
import collections

import numpy as np

# (n, Cin, Cout, K, stride, Lin); small: dy is N(0, 1) times 10^U(-9, -4) per element (a mean loss's gradients)
Case = collections.namedtuple("Case", "n Cin Cout K stride Lin small")
CASES = [Case(1, 1, 4, 5, 1, 23, False), Case(3, 4, 16, 5, 1, 23, False),             # the narrow route, edges
         Case(6, 1, 4, 5, 1, 1000, False), Case(6, 4, 16, 5, 1, 1000, False),         # dw summed over several workgroups' partials
         Case(2, 16, 32, 19, 5, 23, False),                                          # the wide route, Lin no multiple of the stride
         Case(1, 16, 48, 19, 5, 7, False),                                           # Lin < K: every window padded, Lout = 2
         Case(5, 16, 80, 9, 3, 50, False),                                           # another window and stride, a ragged Cout
         Case(2, 16, 768, 19, 5, 40, False),                                         # the real Cout
         Case(6, 16, 32, 19, 5, 1000, False), Case(3, 16, 32, 19, 5, 1001, False),   # 1200 rows: past xb_wgrad_f32's 1024-row block
         Case(3, 4, 16, 5, 1, 23, True),                                             # gradients of 1e-9 .. 1e-4
         # appended (the tests that index this list keep their cases) -- the narrow route's three templates (CO = 4, 8, 16) and a
         # Cout below its template's CO: 8 of 8, 5 of 8, 1 of 4, 12 of 16 at window 1
         Case(2, 4, 8, 5, 1, 300, False), Case(3, 3, 5, 3, 1, 23, False), Case(2, 1, 1, 7, 1, 40, False), Case(2, 8, 12, 1, 1, 300, False),
         # the narrow route at even windows, Lout = Lin + 1: the backward's tile count comes from Lout (257: 2 tiles a chunk where
         # Lin gives 1; 513: 3 against 2)
         Case(2, 2, 6, 6, 1, 256, False), Case(2, 4, 16, 4, 1, 512, False),
         Case(2, 16, 32, 8, 2, 41, False),                                           # the wide route at an even window
         Case(2, 16, 32, 3, 8, 50, False), Case(3, 16, 32, 1, 3, 40, False),         # stride above the window: 60 % and 65 % of dx are exact zeros
         Case(2, 16, 32, 31, 8, 100, False), Case(2, 16, 32, 31, 8, 8, False),       # the widest window; Lout 1
         Case(2, 16, 32, 31, 1, 33, False), Case(2, 16, 32, 1, 1, 40, False),        # window 31 and window 1 at stride 1 (16 channels in: wide)
         Case(2, 16, 32, 9, 6, 383, False)]


def case_id(c):
    return "n%d-%dto%d-K%d-s%d-L%d%s" % (c[:6] + ("-small" if c.small else "",))


def out_len(Lin, K, stride):
    return (Lin + 2 * (K // 2) - K) // stride + 1


def draw(c):
    rng = np.random.default_rng(100000 * c.n + 1000 * c.Cin + 100 * c.Cout + 10 * c.K + c.stride + c.Lin)
    k = 1.0 / np.sqrt(c.Cin * c.K)                                  # torch's Conv1d initialisation
    x = rng.standard_normal((c.n, c.Cin, c.Lin))
    w, b = rng.uniform(-k, k, (c.Cout, c.Cin, c.K)), rng.uniform(-k, k, c.Cout)
    dy = rng.standard_normal((c.n, c.Cout, out_len(c.Lin, c.K, c.stride)))
    if c.small:
        dy = dy * 10.0 ** rng.uniform(-9, -4, dy.shape)
    return tuple(a.astype(np.float32) for a in (x, w, b, dy))


def windows(x, K, stride):
    """(n, Lout, Cin, K): x[b, ci, t stride + k - K // 2], zero outside."""
    n, Cin, Lin = x.shape
    pad, Lout = K // 2, out_len(Lin, K, stride)
    xp = np.zeros((n, Cin, Lin + 2 * pad + stride), x.dtype)
    xp[:, :, pad:pad + Lin] = x
    idx = np.arange(Lout)[:, None] * stride + np.arange(K)[None, :]
    return xp[:, :, idx].transpose(0, 2, 1, 3)


def sigmoid(z):
    return 1.0 / (1.0 + np.exp(-z))


def forward(x, w, b, stride):
    x, w, b = (np.asarray(a, np.float64) for a in (x, w, b))
    Cout, Cin, K = w.shape
    col = windows(x, K, stride)
    z = np.einsum("btck,ock->bot", col, w) + b[None, :, None]
    return z, z * sigmoid(z)


def backward(dy, x, z, w, stride):
    dy, x, z, w = (np.asarray(a, np.float64) for a in (dy, x, z, w))
    Cout, Cin, K = w.shape
    n, _, Lin = x.shape
    pad, Lout = K // 2, z.shape[2]
    s = sigmoid(z)
    dz = dy * (s * (1.0 + z * (1.0 - s)))
    col = windows(x, K, stride)
    dw, db = np.einsum("bot,btck->ock", dz, col), dz.sum(axis=(0, 2))
    dcol = np.einsum("bot,ock->btck", dz, w)
    dxp = np.zeros((n, Cin, Lin + 2 * pad + stride))
    for t in range(Lout):
        dxp[:, :, t * stride:t * stride + K] += dcol[:, t]
    return dxp[:, :, pad:pad + Lin], dw, db


def torch_run(x, w, b, dy, stride, dtype):
    import torch
    xs, ws, bs = (torch.from_numpy(np.asarray(a)).to(dtype).clone().requires_grad_(True) for a in (x, w, b))
    z = torch.nn.functional.conv1d(xs, ws, bs, stride=stride, padding=ws.shape[2] // 2)
    y = torch.nn.functional.silu(z)
    (y * torch.from_numpy(np.asarray(dy)).to(dtype)).sum().backward()
    return dict(z=z.detach().numpy(), y=y.detach().numpy(), dx=xs.grad.numpy(), dw=ws.grad.numpy(), db=bs.grad.numpy())


def tnc(a):
    return np.ascontiguousarray(np.transpose(a, (2, 0, 1)))


def untnc(a):
    return np.ascontiguousarray(np.transpose(a, (1, 2, 0)))


# ---- csrc/xb_conv_plan.h ---------------------------------------------------------------------------------------------------------
def is_narrow(Cin, Cout, K, stride):
    return stride == 1 and Cin <= 16 and Cout <= 16 and Cin * K <= 64


def narrow_blocks(n, Lin, K):
    return n * -(-max(Lin, out_len(Lin, K, 1)) // 256)


def table(chunk, F, W, S, n):
    lens = [20, 4, 320, 16, F * 16 * W, F]
    offs = [int(v) for v in np.concatenate([[0], np.cumsum(lens)[:-1]])]
    L1 = out_len(chunk, 5, 1)
    L2 = out_len(L1, 5, 1)
    T = out_len(L2, W, S)
    r4 = lambda v: (v + 3) // 4 * 4
    pieces = [n * 4 * L1, n * 4 * L1, n * 16 * L2, n * 16 * L2, n * T * 16 * W, n * T * F, n * 16 * L2, n * 4 * L1]     # z1 y1 z2 y2 col z3 dy2 dy1
    at, act = 0, []
    for p in pieces:
        act.append(at)
        at += r4(p)
    return dict(off=offs, len=lens, params=sum(lens), L1=L1, L2=L2, T=T, act=act, act_floats=at)
