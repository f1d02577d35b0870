"""GPU: the encoder at state lengths, windows and strides other than the shipped model's (tests/geometry_cases.py) in the
precisions f16x3 (the tightest bound), mixed (the default) and f16f8 (the q8 im2col image), in both LSTM launch modes,
against the float64 reference (tests/encoder_f64.py): every column of the picked chunks within the table's (max, rms)
bound, the two modes and the two GEMM kernels bit for bit the same, the expanded blank layout, and the time-step count
xb_geometry reports.  The bounds are at least 5x below every defect of geometry_cases.catalogue
(tests/test_encoder_f64.py checks that)."""
import functools

import numpy as np
import pytest

import encoder_cases as EC
import geometry_cases as GC
from encoder_f64 import WEIGHTS, Reference, blank_layout
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu


@functools.lru_cache(maxsize=None)
def _case(name):
    F, nb, sl, W, ST, L, N, weights = GC.GEOMETRY_CASES[name]
    sd = WEIGHTS[weights](F, nb, GC.seed_of(name), state_len=sl, winlen=W)
    x = np.random.default_rng(L + N + W).standard_normal((N, L)).astype(np.float32)
    pk = EC.picks(N)
    ref = Reference(x[pk], sd, nb, winlen=W, stride=ST).run()["scores"]
    ref.setflags(write=False)
    return sd, x, pk, ref


@pytest.mark.parametrize("prec", GC.PRECISIONS)
@pytest.mark.parametrize("name", list(GC.GEOMETRY_CASES))
def test_geometry_against_float64(name, prec, monkeypatch):
    F, nb, sl, W, ST, L, N, _ = GC.GEOMETRY_CASES[name]
    sd, x, pk, ref = _case(name)
    T, S = GC.steps(L, W, ST), nb ** sl
    assert ref.shape == (T, len(pk), S * nb)

    def encode(mode, expand=False):
        ctx = _lib.Context(0, nb, sl, F, W, ST, 5.0, 2.0, L, N, precision=_lib.PRECISIONS[prec], lstm_mode=mode)
        assert (ctx.T, ctx.S, ctx.C_blank, ctx.C_noblank) == (T, S, S * (nb + 1), S * nb)
        ctx.load_state_dict(sd)
        out = [ctx.encode(x, expand_blanks=False)]
        if expand:
            out.append(ctx.encode(x, expand_blanks=True))
        ctx.close()
        return out

    outs, worst = [], (0.0, 0.0)
    for mode in (1, 2):
        got = encode(mode, expand=mode == 1)
        outs.append(got[0])
        assert got[0].shape == (T, N, S * nb) and np.isfinite(got[0]).all()
        if mode == 1:
            assert np.array_equal(got[1], blank_layout(got[0], nb, np.float32(2.0), True))
        err = got[0][:, pk].astype(np.float64) - ref
        emax, erms = float(np.abs(err).max()), float(np.sqrt((err ** 2).mean()))
        print("PRECISION %s %s mode %d max %.3e rms %.3e" % (name, prec, mode, emax, erms))
        worst = (max(worst[0], emax), max(worst[1], erms))
    assert np.array_equal(outs[0], outs[1])               # one launch per step == persistent, bit for bit
    monkeypatch.setenv("XB_GEMM4", "0")
    assert np.array_equal(encode(0)[0], outs[0])          # the two GEMM kernels add the same products in the same order
    bmax, brms = GC.BOUNDS[name][prec]
    assert worst[0] <= bmax and worst[1] <= brms, (worst, bmax, brms)
