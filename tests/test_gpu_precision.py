"""GPU: every encoder precision (xb_precision, and the int8-limb recurrence XB_LSTM_I8 = 1 / 2 under f16f8) in both LSTM
launch modes against the float64 reference (tests/encoder_f64.py) on signal-sensitive weights with non-zero bias_hh, and
on outlier weights, at the shapes of tests/encoder_cases.py: scores within the table's (max, rms) bound per precision on
the first and last chunk and at the group seams, the outputs of LSTM layers 3 and 4 within LAYER_BOUNDS.  The table's
bounds are at least 5x below every defect a precision claims not to have (tests/test_encoder_f64.py checks that)."""
import functools

import numpy as np
import pytest

import encoder_cases as EC
from encoder_f64 import WEIGHTS, Reference
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    F, nb, L, N, weights = EC.CASES[name]
    sd = WEIGHTS[weights](F, nb, EC.seed_of(name))
    x = np.random.default_rng(L + N).standard_normal((N, L)).astype(np.float32)
    pk = EC.picks(N)
    ref = Reference(x[pk], sd, nb).run()
    return sd, x, pk, ref


def _layer(hi, second, residual):
    h = hi.view(np.float16).astype(np.float64)
    return h + second.view(np.float16).astype(np.float64) if residual else h


@pytest.mark.parametrize("prec", list(EC.PRECISIONS))
@pytest.mark.parametrize("name", list(EC.CASES))
def test_precision_against_float64(name, prec, monkeypatch):
    F, nb, L, N, _ = EC.CASES[name]
    sd, x, pk, ref = _case(name)
    pname, i8 = EC.PRECISIONS[prec]
    monkeypatch.setenv("XB_LSTM_I8", i8)
    # the consumers of layers 3 and 4 (input projection of layer 4, the linear layer) read an fp16 residual in f16x3 and
    # mixed, a q8 image in the f16f8 family, nothing in f16
    residual = pname in ("f16x3", "mixed")
    outs = []
    for mode in (1, 2):
        ctx = _lib.Context(0, nb, 3, F, 19, 5, 5.0, 2.0, L, N, precision=_lib.PRECISIONS[pname], lstm_mode=mode)
        ctx.load_state_dict(sd)
        got = ctx.encode(x, expand_blanks=False)
        layers = [_layer(*ctx.debug_layer_output(w, N), residual)[:, pk] for w in (0, 1)]
        ctx.close()
        outs.append(got)
        err = got[:, pk].astype(np.float64) - ref["scores"]
        emax, erms = float(np.abs(err).max()), float(np.sqrt((err ** 2).mean()))
        lerr = max(float(np.abs(layers[0] - ref["lstm3"]).max()), float(np.abs(layers[1] - ref["lstm4"]).max()))
        print("PRECISION %s %s mode %d max %.3e rms %.3e layer %.3e" % (name, prec, mode, emax, erms, lerr))
        bmax, brms = EC.BOUNDS[name][prec]
        assert emax <= bmax and erms <= brms, (mode, emax, erms, bmax, brms)
        assert lerr <= EC.LAYER_BOUNDS[prec], (mode, lerr)
    assert np.array_equal(outs[0], outs[1])               # one launch per step == persistent, bit for bit
