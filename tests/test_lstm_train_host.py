"""CPU: what the reference of the LSTM training tests is worth.  tests/lstm_train_ref.py (the float64 restatement the device's
xb_lstm_train_forward_dev / _backward_dev are held to) against torch.nn.LSTM in float64 with torch.autograd, through the same
composition as crf/lstm.py (linear, then the recurrence): y, dx, dW_ih, dW_hh and db agree to 1e-10 of each tensor's maximum --
both sides are float64 and T is short, only rounding differs.  A gradient of zeros gives exactly zero; LSTM.forward refuses what
it cannot run."""
import numpy as np
import pytest
import torch

import lstm_train_ref as R
from conftest import make_config
from xna_basecaller_amd.crf.model import LSTM, Model


def case(T, n, F, I=None, seed=0):
    """x, W_ih, W_hh, b, dy in float64: weights of torch's own scale (uniform +-1/sqrt(F)) times 2, so that gates move."""
    rng = np.random.default_rng(seed + 1000 * T + 10 * n + F)
    I = I or F
    k = 2.0 / np.sqrt(F)
    return (rng.standard_normal((T, n, I)), rng.uniform(-k, k, (4 * F, I)), rng.uniform(-k, k, (4 * F, F)),
            rng.uniform(-k, k, 4 * F), rng.standard_normal((T, n, F)))


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("F", [16, 48])
@pytest.mark.parametrize("n", [1, 3])
@pytest.mark.parametrize("T", [1, 2, 7])
def test_restatement_is_torch_lstm_in_float64(T, n, F, reverse):
    a = case(T, n, F, I=F + 8)
    ref = R.layer(*a, reverse)
    got = R.torch_layer(*a, reverse, torch.float64)
    for k in ("y", "dx", "dw_ih", "dw_hh", "db"):
        assert ref[k].shape == got[k].shape, k
        assert R.rel(ref[k], got[k]) <= 1e-10, (k, R.rel(ref[k], got[k]))


@pytest.mark.parametrize("reverse", [False, True])
def test_zero_dy_gives_exactly_zero_dgin(reverse):
    x, w_ih, w_hh, b, dy = case(5, 3, 16)
    y, gates, c = R.forward(x @ w_ih.T + b, w_hh, reverse)
    dgin = R.backward(np.zeros_like(dy), w_hh, gates, c, reverse)
    assert dgin.shape == (5, 3, 64) and not dgin.any()
    assert R.backward(dy, w_hh, gates, c, reverse).any()


def test_h_prev_is_y_of_the_step_processed_before():
    y = np.arange(24.0).reshape(4, 2, 3) + 1
    assert np.array_equal(R.h_prev(y, False)[1:], y[:-1]) and not R.h_prev(y, False)[0].any()
    assert np.array_equal(R.h_prev(y, True)[:-1], y[1:]) and not R.h_prev(y, True)[-1].any()


def test_forward_refuses_what_it_cannot_run():
    model = Model(make_config(32))
    x = torch.zeros(3, 2, 32)
    with pytest.raises(ValueError, match="on the model's device"):
        model.encoder[8](x)                                      # a CPU tensor
    with pytest.raises(ValueError, match="on the model's device"):
        model.encoder[8](x.numpy())
    with pytest.raises(RuntimeError, match=r"model\.encoder\[i\]\(x\)"):
        LSTM(32, 32, reverse=True)(x)                            # a layer without a model
    assert sorted(model.state_dict()) == sorted(Model(make_config(32)).state_dict()) and len(model.state_dict()) == 28
    assert all(k.startswith("encoder.") for k in model.state_dict())
