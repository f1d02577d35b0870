"""CPU: the restatements of xb_head_grad (tests/headgrad_ref.py) and its split plan (csrc/xb_head_split.h).

  - the float64 form is the gradient torch's autograd gives, in float64 on the CPU, for scale * tanh(linear(X, W, b)) under a
    linear functional of the output (whose gradient with respect to the output is dY), to 1e-12 relative;
  - the form with the kernel's operand rounding stays within K_BOUND of the elementwise yardstick, with and only with the
    power-of-two prescale;
  - the single-product form -- fp16 dZ against x_hi alone -- breaks that bound on the same inputs, so the bound cannot hide a
    dropped residual product;
  - the split plan: slabs that are never empty and cover the rows once, a workspace within the bound, for M = 1 .. 4097 and the
    two training shapes."""
import ctypes as C

import numpy as np
import pytest
import torch

import headgrad_ref as H
from xna_basecaller_amd import _lib

SCALE = 5.0
CASES = [(4099, 64, 32), (257, 125, 96), (21, 64, 32)]


@pytest.mark.parametrize("M,O,F", [(37, 25, 32), (300, 64, 96)])
def test_float64_form_is_autograd(M, O, F):
    rng = np.random.default_rng(M)
    x = rng.uniform(-1, 1, (M, F))
    x_hi = x.astype(np.float16)                          # the planes carry hi + lo: the model reads that value
    x_lo = (x - x_hi.astype(np.float64)).astype(np.float16)
    xs = torch.from_numpy(x_hi.astype(np.float64) + x_lo.astype(np.float64))
    w2 = torch.from_numpy(rng.standard_normal((O, F)) * 0.3).requires_grad_()
    b2 = torch.from_numpy(rng.standard_normal(O) * 0.1).requires_grad_()
    c = torch.from_numpy(rng.standard_normal((M, O)) * 1e-4)
    y2 = SCALE * torch.tanh(torch.nn.functional.linear(xs, w2, b2))
    (y2 * c).sum().backward()
    dw, db = H.head_grad_f64(y2.detach().numpy(), c.numpy(), x_hi.view(np.uint16), x_lo.view(np.uint16), SCALE)
    for got, ref in ((dw, w2.grad.numpy()), (db, b2.grad.numpy())):
        assert np.abs(got - ref).max() <= 1e-12 * np.abs(ref).max()


@pytest.mark.parametrize("M,O,F", CASES)
def test_kernel_arithmetic_holds_the_bound_and_one_product_does_not(M, O, F):
    a = H.inputs(M, O, F, seed=M)
    ref, bnd = H.head_grad_f64(*a, SCALE), H.bound(*a, SCALE)
    kern = H.ratios(H.head_grad_kernel(*a, SCALE), ref, bnd)
    single = H.ratios(H.head_grad_single(*a, SCALE), ref, bnd)
    print("M=%d O=%d F=%d: |err| / bound  kernel arithmetic dW %.3g db %.3g, single product dW %.3g db %.3g; K_BOUND %.3g"
          % (M, O, F, *kern, *single, H.K_BOUND))
    assert max(kern) <= H.K_BOUND
    assert single[0] > H.K_BOUND


def test_small_gradients_need_the_prescale():
    """Every |dY| below 2^-20: fp16 without the power-of-two scale loses them to its subnormals."""
    a = H.inputs(257, 64, 32, seed=5, lo=1e-9, hi=2.0 ** -21)
    assert np.abs(a[1]).max() < 2.0 ** -20
    ref, bnd = H.head_grad_f64(*a, SCALE), H.bound(*a, SCALE)
    assert max(H.ratios(H.head_grad_kernel(*a, SCALE), ref, bnd)) <= H.K_BOUND
    assert H.ratios(H.head_grad_kernel(*a, SCALE, prescale=False), ref, bnd)[0] > H.K_BOUND


# ---- the split plan ---------------------------------------------------------------------------------------------------------
FIELDS = ("error", "ksteps", "nslabs", "o_tiles", "f_tiles", "o_tiles_per_launch", "launches", "row_bytes", "bytes", "order_kept")
KT, TO, TF = 32, 64, 128


def plan(M, O, F, mb=None, cu=256):
    out = (C.c_int64 * 10)()
    _lib.load().xb_internal_head_plan(M, O, F, cu, None if mb is None else str(mb).encode(), out)
    return dict(zip(FIELDS, out))


def check_plan(M, O, F, mb):
    p = plan(M, O, F, mb)
    bound = (256 if mb is None else mb) << 20
    assert p["error"] == 0
    assert p["ksteps"] == -(-M // KT) and p["o_tiles"] == -(-O // TO) and p["f_tiles"] == -(-F // TF)
    ns = p["nslabs"]
    assert 1 <= ns <= p["ksteps"]
    begin = [min(p["ksteps"] * s // ns * KT, M) for s in range(ns + 1)]
    assert begin[0] == 0 and begin[-1] == M and all(a < b for a, b in zip(begin, begin[1:])), (M, begin)
    assert p["row_bytes"] == TO * (4 * F + 8)
    assert 1 <= p["o_tiles_per_launch"] <= p["o_tiles"]
    assert p["launches"] == -(-p["o_tiles"] // p["o_tiles_per_launch"])
    assert p["bytes"] == p["o_tiles_per_launch"] * ns * p["row_bytes"] <= bound
    return p


@pytest.mark.parametrize("O,F", [(64, 32), (125, 96), (1296, 384), (1296, 768)])
def test_split_plan_for_every_small_M(O, F):
    for M in range(1, 4098):
        for mb in (None, 1):
            check_plan(M, O, F, mb)


def test_split_plan_of_the_training_shapes():
    for M in (720 * 64, 720 * 384):
        p = check_plan(M, 1296, 768, None)
        assert p["launches"] == 1 and p["order_kept"] and p["nslabs"] * p["o_tiles"] * p["f_tiles"] >= 8 * 256
        q = check_plan(M, 1296, 768, 1)
        assert q["launches"] > 1


def test_a_bound_that_only_splits_the_call_keeps_the_slabs():
    """M = 1000 at O = 1296, F = 384 (tests/test_gpu_headgrad.py's split case): four slabs either way, the 1 MB bound serves two
    blocks of output rows per launch."""
    p, q = check_plan(1000, 1296, 384, None), check_plan(1000, 1296, 384, 1)
    assert p["nslabs"] == q["nslabs"] == 4 and p["launches"] == 1 and q["launches"] == 11 and q["order_kept"] == 1
    r = check_plan(4099, 1296, 384, 1)
    assert r["order_kept"] == 0 and r["nslabs"] < check_plan(4099, 1296, 384, None)["nslabs"]
