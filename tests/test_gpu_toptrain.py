"""GPU: the training kernels as one composed step -- tests/toptrain_dev.py chains xb_linear_f32_dev, xb_lstm_train_forward_dev,
xb_head_dz_dev, xb_wgrad_f32_dev and xb_lstm_train_backward_dev by the public header's recipe, and the scores and all 4 L + 2
gradients are held to the float64 restatement tests/toptrain_ref.py.  The tolerance is the rule of tests/test_gpu_lstm_train.py:
per tensor, the error relative to the tensor's maximum stays within MARGIN = 8 times that of torch.nn.LSTM / Linear with autograd in
float32 on the CPU (toptrain_ref.torch_run) on the same float32 inputs.  What a composition gets wrong -- a layer's direction, the
side of dW_hh's shift, one bias where two are summed, a weight not transposed -- is off by orders of magnitude in one tensor.
tests/test_toptrain_host.py runs a float32 numpy stand-in through the same cases and the same rule on the CPU.

  cases      toptrain_ref.CASES: L in {1, 2, 3, 5}, a ragged C = 125, n = 65 (the recurrence's four-tile launch), F = 768,
             gradients of 1e-9 .. 1e-4, and T = 1, where dW_hh sums over no rows and is zero bytes
  loss       toptrain_ref.LOSS_CASE: d loss / d scores is what xb_ctc_loss_grad_dev (mean, blank-less) writes for the device's own
             scores; the reference chain is fed the same dscores (the loss has its own tests)
  bytes      a repeated step gives the same bytes in every output"""
import functools

import numpy as np
import pytest
import torch

import lstm_train_ref as R
import toptrain_dev as D
import toptrain_ref as TR
from ctc_wide_cases import label_rows
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MARGIN = 8.0
SCALE = 5.0
RATIOS = []


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0, 5, 2, 32, 19, 5, SCALE, 2.0, TR.LOSS_CASE.T * 5, TR.LOSS_CASE.n)   # n_base 5, state_len 2: 125 blank-less columns
    assert c.T >= TR.LOSS_CASE.T and c.C_noblank == TR.LOSS_CASE.C
    yield c
    c.close()
    if RATIOS:
        print("largest ratio to torch float32: %.2f (%s)" % max(RATIOS))


def names(L):
    return ["layer%d %s" % (i, k) for i in range(L) for k in ("weight_ih", "weight_hh", "bias_ih", "bias_hh")] + ["head weight", "head bias"]


def held(what, got, ref, yard):
    err = R.rel(got, ref)
    ratio = err / yard if yard else (0.0 if err == 0.0 else float("inf"))
    RATIOS.append((ratio, what))
    print("%-40s device %.3g  torch float32 %.3g  ratio %.2f" % (what, err, yard, ratio))
    assert np.isfinite(got).all(), what
    assert err <= MARGIN * yard, (what, err, yard)


def held_step(tag, got, x0, tensors, dscores):
    """Every tensor of a step against the restatement, with torch float32 as the yardstick; all are printed before any fails."""
    ref = TR.run(x0, tensors, SCALE, dscores)
    t32 = TR.torch_run(x0, tensors, SCALE, dscores, torch.float32)
    failed = []
    for what, g, r, t in [("scores", got["scores"], ref["scores"], t32["scores"])] + list(zip(names(len(tensors) // 4), got["grads"], ref["grads"], t32["grads"])):
        assert g.shape == r.shape, (what, g.shape, r.shape)
        try:
            held("%s %s" % (tag, what), g, r, R.rel(t, r))
        except AssertionError as e:
            failed.append(str(e))
    assert not failed, failed


def _dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)


@functools.lru_cache(maxsize=None)
def inputs(case):
    return TR.draw(case)


@pytest.mark.parametrize("case", TR.CASES, ids=TR.case_id)
def test_composed_step_against_the_restatement(ctx, case):
    x0, tensors, dscores = inputs(case)
    got = D.composed_step(ctx, _dev(x0), [_dev(a) for a in tensors], SCALE, _dev(dscores))
    held_step(TR.case_id(case), got, x0, tensors, dscores)
    if case.T == 1:                                                   # h_-1 = 0: no step has a recurrent product
        for i in range(case.L):
            assert got["grads"][4 * i + 1].tobytes() == bytes(got["grads"][4 * i + 1].nbytes), i
    for i in range(case.L):                                           # both biases of a layer receive the same gradient
        assert got["grads"][4 * i + 2].tobytes() == got["grads"][4 * i + 3].tobytes()


def test_composed_step_from_the_device_loss(ctx):
    case = TR.LOSS_CASE
    x0, tensors, _ = inputs(case)
    Lt = 20
    targets, lens = label_rows(np.random.default_rng(8), case.n, Lt, 5, 2, dtype=np.uint8)
    assert (case.T >= lens - 2).all() and lens.max() == Lt and lens.min() == 2          # every row has a path
    stages = D.forward(ctx, _dev(x0), [_dev(a) for a in tensors], SCALE)
    d_t, d_l = torch.from_numpy(targets).to(DEV), torch.from_numpy(lens).to(DEV)
    d_loss = torch.full((case.n,), float("nan"), dtype=torch.float32, device=DEV)
    d_grad = torch.full(tuple(stages["scores"].shape), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.ctc_loss_grad_dev(stages["scores"].data_ptr(), case.T, case.n, False, d_t.data_ptr(), Lt, d_l.data_ptr(), d_loss.data_ptr(), d_grad.data_ptr())
    ctx.synchronize()
    loss, dscores = d_loss.cpu().numpy(), d_grad.cpu().numpy()
    print("losses", " ".join("%.4f" % v for v in loss), " largest |d loss / d scores| %.3g" % np.abs(dscores).max())
    assert np.isfinite(loss).all() and (loss > 0).all() and np.isfinite(dscores).all() and np.abs(dscores).max() > 0
    grads = D.backward(ctx, stages, d_grad)
    got = dict(scores=stages["scores"].cpu().numpy(), grads=[g.cpu().numpy() for g in grads])
    held_step(TR.case_id(case), got, x0, tensors, dscores)


def test_a_repeated_step_gives_the_same_bytes(ctx):
    x0, tensors, dscores = inputs(TR.CASES[1])
    args = (_dev(x0), [_dev(a) for a in tensors], SCALE, _dev(dscores))
    a, b = D.composed_step(ctx, *args), D.composed_step(ctx, *args)
    assert a["scores"].tobytes() == b["scores"].tobytes()
    assert len(a["grads"]) == len(b["grads"]) == 10
    for what, p, q in zip(names(2), a["grads"], b["grads"]):
        assert np.isfinite(p).all() and p.tobytes() == q.tobytes(), what
