"""CPU: the reference the trainers are held to at other geometries (tests/train_geometry_cases.py), before the device is held to it
(tests/test_gpu_train_geometry.py).

  chain       the torch chain in float64 -- conv1d + silu three times, five LSTM layers, the head, autograd -- agrees to 1e-10 of
              each tensor's maximum with the composition of the restatements the kernels' own tests use: convtrain_ref.forward /
              backward around toptrain_ref.run, on a drawn d loss / d scores.  Two derivations of the same 29 tensors that share no
              code: this is what makes the reference trustworthy at a stride above the window, at window 1 and at T = 1
  yardsticks  the device test's rule is MARGIN times the error of the same chain in torch float32: that error is non-zero for every
              case and tensor -- but for dW_hh at T = 1, which is exactly zero on both sides"""
import functools

import numpy as np
import pytest
import torch

import train_geometry_cases as G
from lstm_train_ref import rel


@functools.lru_cache(maxsize=None)
def chains(c):
    sd = G.weights(c)
    tensors = [sd[k] for k in G.KEYS]
    signal = G.batch(c, seed=7)[0]
    T = G.steps(c)[2]
    dscores = np.random.default_rng(c.chunk + c.W).standard_normal((T, c.n, G.columns(c))).astype(np.float32)
    return (G.torch_chain(signal, tensors, dscores, torch.float64, c.S), G.restated_chain(signal, tensors, dscores, c.S),
            G.torch_chain(signal, tensors, dscores, torch.float32, c.S))


def rows(a, b):
    return [("scores", a["scores"], b["scores"])] + list(zip(G.KEYS, a["grads"], b["grads"]))


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_torch_chain_is_the_composed_restatements(c):
    ref, restated, _ = chains(c)
    T = G.steps(c)[2]
    assert ref["scores"].shape == (T, c.n, G.columns(c)) and len(ref["grads"]) == len(restated["grads"]) == 28
    for what, r, g in rows(ref, restated):
        assert g.shape == r.shape and np.isfinite(r).all(), what
        if T == 1 and what.endswith("weight_hh_l0"):
            assert not r.any() and not g.any(), what
            continue
        assert np.abs(r).max() > 0, what
        assert rel(g, r) <= 1e-10, (what, rel(g, r))


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_no_yardstick_is_zero(c):
    ref, _, t32 = chains(c)
    T = G.steps(c)[2]
    for what, r, t in rows(ref, t32):
        assert t.dtype == np.float32 and t.shape == r.shape, what
        yard = rel(t, r)
        print("%-32s torch float32 %.3g" % (what, yard))
        if T == 1 and what.endswith("weight_hh_l0"):
            assert not r.any() and not t.any(), what
        else:
            assert yard > 0, what                          # torch float32 bit-equal to float64 would make the rule empty
