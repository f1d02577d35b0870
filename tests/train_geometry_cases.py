"""The trainers at geometries other than the shipped one's: the table of cases, their weights and batches, and the float64 reference
of a whole step (no device; tests/test_train_geometry_host.py is the CPU tier, tests/test_gpu_train_geometry.py the GPU tier).

A case is a context: (n_base, state_len, window, stride, chunk, features, n).  The five head widths no trainer has run at -- 216,
625, 1024, 3125, 4096 -- each under another window and stride of conv3: stride above the window (positions of conv2's output no
window covers: exact zeros in conv3's dx), window 1 (no padding), window 31 at stride 8 (the widest window a context takes), a chunk
shorter than the window (T = 1: no recurrent product, dW_hh is zero bytes); features 96 with 17 chunks (a ragged row tile of the
recurrence) at the shipped window and stride.

  CASES, case_id(c), steps(c), columns(c), label_width(c)
  weights(c, seed)                  -> the 28 tensors as a state dict (xna_basecaller_amd.synthetic), conv3 at the case's window
  batch(c, seed, n = c.n)           -> signal (n, chunk), targets (n, Lt) uint8, lengths (n) int32: ctc_wide_cases.label_rows, every
                                       length <= T + state_len, so that every row has a path
  torch_chain(signal, tensors, dscores, dtype, stride, scale) -> dict(scores (T, n, C), grads: 28 arrays) from conv1d + silu, LSTM and
                                       Linear with autograd on the CPU: tests/test_gpu_fulltrain.py's chain at any window (the
                                       weights' own), stride and scale.  In float64 the reference, in float32 the yardstick.
  restated_chain(signal, tensors, dscores, stride, scale) -> the same from the restatements the kernels' own tests are held to:
                                       convtrain_ref.forward / backward three times around toptrain_ref.run"""
import collections

import numpy as np

import convtrain_ref as CR
import toptrain_ref as TR
from ctc_wide_cases import label_rows
from xna_basecaller_amd.synthetic import STATE_DICT_ORDER, encoder_shapes, seeded_state_dict

Case = collections.namedtuple("Case", "nb sl W S chunk F n")
KEYS = list(STATE_DICT_ORDER)          # crf/trainer.py's full_keys(): the order of csrc/xb_conv_plan.h, then csrc/xb_top_plan.h
SCALE = 5.0

# case: (T, C) it must give
EXPECTED = collections.OrderedDict([
    (Case(6, 2, 9, 6, 383, 32, 3), (64, 216)),
    (Case(5, 3, 5, 3, 98, 32, 4), (33, 625)),
    (Case(4, 4, 3, 8, 200, 32, 3), (25, 1024)),        # stride above the window
    (Case(5, 4, 31, 8, 120, 64, 3), (15, 3125)),
    (Case(4, 5, 1, 1, 40, 32, 3), (40, 4096)),         # window 1, no padding
    (Case(4, 2, 19, 5, 200, 96, 17), (40, 64)),        # features 96 and a ragged row tile
    (Case(4, 5, 31, 8, 8, 32, 2), (1, 4096)),          # the chunk is shorter than the window
])
CASES = list(EXPECTED)


def case_id(c):
    return "nb%d-sl%d-w%d-s%d-L%d-F%d-n%d" % c


def steps(c):
    """(L1, L2, T): samples behind conv1 and conv2, time steps behind conv3."""
    L1 = CR.out_len(c.chunk, 5, 1)
    L2 = CR.out_len(L1, 5, 1)
    return L1, L2, CR.out_len(L2, c.W, c.S)


def columns(c):
    return c.nb ** (c.sl + 1)


def label_width(c):
    """Lt: up to 20 labels, and no more than a row of T steps has a path for."""
    return min(steps(c)[2] + c.sl, 20)


for _c, _tc in EXPECTED.items():
    assert (steps(_c)[2], columns(_c)) == _tc, (_c, steps(_c), columns(_c))


def weights(c, seed=3):
    keys, shapes = encoder_shapes(c.F, c.nb, c.sl, c.W)
    assert keys == KEYS
    return seeded_state_dict(keys, shapes, seed=seed)


def batch(c, seed, n=None):
    n = c.n if n is None else n
    rng = np.random.default_rng(seed)
    signal = rng.standard_normal((n, c.chunk)).astype(np.float32)
    targets, lens = label_rows(rng, n, label_width(c), c.nb, c.sl, dtype=np.uint8)
    assert (lens.astype(np.int64) <= steps(c)[2] + c.sl).all() and (lens >= c.sl).all()      # every row has a path
    return signal, targets, lens.astype(np.int32)


def torch_chain(signal, tensors, dscores, dtype, stride=5, scale=SCALE):
    """The whole encoder from the signal to the scores and the gradients of all 28 tensors for a given d loss / d scores."""
    import torch
    params = [torch.from_numpy(np.asarray(a)).to(dtype).clone().requires_grad_(True) for a in tensors]
    F = params[4].shape[0]
    x = torch.from_numpy(np.asarray(signal)).to(dtype)[:, None, :]
    for i, s in enumerate((1, 1, stride)):
        w, b = params[2 * i], params[2 * i + 1]
        x = torch.nn.functional.silu(torch.nn.functional.conv1d(x, w, b, stride=s, padding=w.shape[2] // 2))
    x = x.permute(2, 0, 1)
    for i in range(5):
        rnn = torch.nn.LSTM(F, F).to(dtype)
        named = dict(zip(("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"), params[6 + 4 * i:10 + 4 * i]))
        rev = TR.reverse_of(5, i)
        y = torch.func.functional_call(rnn, named, (x.flip(0) if rev else x,))[0]
        x = y.flip(0) if rev else y
    scores = scale * torch.tanh(torch.nn.functional.linear(x, params[-2], params[-1]))
    (scores * torch.from_numpy(np.asarray(dscores)).to(dtype)).sum().backward()
    return dict(scores=scores.detach().numpy(), grads=[p.grad.numpy() for p in params])


def restated_chain(signal, tensors, dscores, stride=5, scale=SCALE):
    x = np.asarray(signal, np.float64)[:, None, :]
    stages = []
    for i, s in enumerate((1, 1, stride)):
        w, b = tensors[2 * i], tensors[2 * i + 1]
        z, y = CR.forward(x, w, b, s)
        stages.append((x, z, w, s))
        x = y
    top = TR.run(CR.tnc(x), tensors[6:], scale, dscores)
    dy, grads = CR.untnc(top["dx0"]), [None] * 6
    for i in (2, 1, 0):
        x, z, w, s = stages[i]
        dy, grads[2 * i], grads[2 * i + 1] = CR.backward(dy, x, z, w, s)
    return dict(scores=top["scores"], grads=grads + top["grads"])
