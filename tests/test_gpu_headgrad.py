"""GPU: xb_head_grad, the gradient of the CRF head's weight and bias from the gradient of its output (csrc/xb_head.hip).

The contract is elementwise: |device - float64| <= K_BOUND * 2^-24 * (|dZ|^T |X|) for dW and K_BOUND * 2^-24 * sum |dZ| for db,
against tests/headgrad_ref.py's float64 form.  K_BOUND = 4 x the largest ratio measured on the MI355X over the cases of this
file (headgrad_ref.K_MEASURED; every test prints its ratios), and tests/test_headgrad_host.py shows that a single fp16 product
exceeds it on the CPU.  Shapes: features 32 / 96 / 384 (one, three, twelve k-tiles of the forward; a quarter, three quarters and
three whole feature tiles here), heads of 64, 125 (ragged in both MFMA tile dimensions) and 1296 columns, rows 1, 21, 255, 256,
257 (one k-tile short of, at and past two slabs) and 4099 (17 slabs); the heads of the other (n_base, state_len) pairs -- 216, 625,
1024, 3125 and 4096 columns -- at features 32 and 96 and rows 1, 21, 257 and 1000 (four slabs), under the same K_BOUND; gradients of the magnitude a mean loss gives (1e-6 .. 1e-3),
one case with every |dY| < 2^-20, which fails without the prescale.  Also: columns of zeros in dY give exact zeros, two calls give
the same bytes, a workspace bound that splits the call over output rows gives the same bytes and one that shortens the slab list
stays within the bound, the context's own X is the explicit one bit for bit, and the refusals."""
import ctypes

import numpy as np
import pytest

import headgrad_ref as H
from conftest import encoder_shapes, seeded_state_dict
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu
SCALE = 5.0
HEADS = {64: (4, 2), 125: (5, 2), 1296: (6, 3)}            # columns -> (n_base, state_len)
ROWS = (1, 21, 255, 256, 257, 4099)
# the widths of the other pairs a context takes: 4, 10, 16, 49 and 64 blocks of 64 output rows (3125: a ragged last block, and
# rows of Y and dY that are not 16-byte aligned); at 1000 rows head_plan cuts the sum into four slabs at every width
NEW_HEADS = {216: (6, 2), 625: (5, 3), 1024: (4, 4), 3125: (5, 4), 4096: (4, 5)}
HEADS.update(NEW_HEADS)
NEW_ROWS = (1, 21, 257, 1000)
SHAPES = [(F, O) for O in (64, 125, 1296) for F in (32, 96, 384)] + [(F, O) for O in sorted(NEW_HEADS) for F in (32, 96)]


def _context(F, O, chunk_len=100, n=1, precision=_lib.XB_PREC_MIXED, seed=3):
    nb, sl = HEADS[O]
    ctx = _lib.Context(0, nb, sl, F, 19, 5, SCALE, 2.0, chunk_len, n, precision=precision)
    assert ctx.C_noblank == O
    keys, shapes = encoder_shapes(F, nb, sl)
    ctx.load_state_dict(seeded_state_dict(keys, shapes, seed=seed))
    return ctx


def _measure(ctx, a, what):
    got = ctx.head_grad(*a)
    ref, bnd = H.head_grad_f64(*a, SCALE), H.bound(*a, SCALE)
    r = H.ratios(got, ref, bnd)
    print("%s: |err| / bound dW %.3g db %.3g (restatement with float64 sums: %s)"
          % (what, r[0], r[1], "dW %.3g db %.3g" % H.ratios(H.head_grad_kernel(*a, SCALE), ref, bnd)))
    return got, max(r)


def _slabs(M, O, F, cu=256):
    """nslabs of xb::head_plan (csrc/xb_head_split.h) under the default workspace bound."""
    out = (ctypes.c_int64 * 10)()
    _lib.load().xb_internal_head_plan(M, O, F, cu, None, out)
    assert out[0] == 0
    return out[2]


@pytest.mark.parametrize("F,O", SHAPES, ids=["%d-%d" % s for s in SHAPES])
def test_gradient_within_the_bound(F, O):
    ctx = _context(F, O)
    worst = {}
    if O in NEW_HEADS:                                                  # several slabs from 32 CUs up: 1000 rows are 32 k-tiles
        assert _slabs(1000, O, F, cu=32) == _slabs(1000, O, F) == 4 and _slabs(257, O, F) == 2
    for M in NEW_ROWS if O in NEW_HEADS else ROWS:
        a = H.inputs(M, O, F, seed=M + O + F, zero_cols=(0, O - 1) if M > 1 else ())
        (dw, db), worst["M=%d" % M] = _measure(ctx, a, "F=%d O=%d M=%d" % (F, O, M))
        if M > 1:
            assert not dw[0].any() and not dw[O - 1].any() and db[0] == 0 and db[O - 1] == 0
        dw2, db2 = ctx.head_grad(*a)
        assert dw.tobytes() == dw2.tobytes() and db.tobytes() == db2.tobytes()
    a = H.inputs(257, O, F, seed=7, lo=1e-9, hi=2.0 ** -21)
    assert np.abs(a[1]).max() < 2.0 ** -20
    _, worst["small"] = _measure(ctx, a, "F=%d O=%d M=257, every |dY| < 2^-20" % (F, O))
    dw, db = ctx.head_grad(a[0], np.zeros_like(a[1]), a[2], a[3])
    assert not dw.any() and not db.any()
    ctx.close()
    print("F=%d O=%d: largest |err| / bound %.3g, K_BOUND %.3g" % (F, O, max(worst.values()), H.K_BOUND))
    assert max(worst.values()) <= H.K_BOUND, worst


def test_workspace_bound_splits_the_call(monkeypatch):
    """O = 1296, F = 384.  M = 1000: four slabs; under XB_HEAD_SCRATCH_MB=1 the call runs as 11 launches over blocks of output rows
    with the same slabs -- the same bytes.  M = 4099: 17 slabs by default, 10 longer ones under the bound -- another order of
    the sums, within the bound."""
    F, O = 384, 1296
    ctx = _context(F, O)
    a = H.inputs(1000, O, F, seed=11)
    (dw, db), r0 = _measure(ctx, a, "M=1000, default workspace")
    b = H.inputs(4099, O, F, seed=12)
    _, r1 = _measure(ctx, b, "M=4099, default workspace")
    monkeypatch.setenv("XB_HEAD_SCRATCH_MB", "1")
    dw1, db1 = ctx.head_grad(*a)
    assert dw.tobytes() == dw1.tobytes() and db.tobytes() == db1.tobytes()
    _, r2 = _measure(ctx, b, "M=4099, 1 MB workspace")
    monkeypatch.delenv("XB_HEAD_SCRATCH_MB")
    dw2, _ = ctx.head_grad(*a)
    assert dw.tobytes() == dw2.tobytes()
    ctx.close()
    assert max(r0, r1, r2) <= H.K_BOUND, (r0, r1, r2)


def test_context_operand_is_the_explicit_one():
    """X = NULL after an encode of 3 chunks of 2000 samples at features 96: the last LSTM layer's output where the encoder left it."""
    F, O, n = 96, 64, 3
    ctx = _context(F, O, chunk_len=2000, n=n)
    rng = np.random.default_rng(2)
    y = ctx.encode(rng.standard_normal((n, 2000)).astype(np.float32), expand_blanks=False)
    assert y.shape == (ctx.T, n, O) and ctx.T == 400
    dy = (rng.standard_normal(y.shape) * 1e-4).astype(np.float32)
    dw, db = ctx.head_grad(y, dy)
    x_hi, x_lo = ctx.debug_layer_output(1, n)
    ew, eb = ctx.head_grad(y, dy, x_hi, x_lo)
    assert dw.tobytes() == ew.tobytes() and db.tobytes() == eb.tobytes()
    a = (y.reshape(-1, O), dy.reshape(-1, O), x_hi.reshape(-1, F), x_lo.reshape(-1, F))
    r = H.ratios((dw, db), H.head_grad_f64(*a, SCALE), H.bound(*a, SCALE))
    print("context form, M = %d: |err| / bound dW %.3g db %.3g" % (ctx.T * n, *r))
    assert max(r) <= H.K_BOUND
    with pytest.raises(_lib.XbError, match="last encoder pass"):
        ctx.head_grad(y[:10], dy[:10])
    with pytest.raises(_lib.XbError, match="both"):
        ctx._check(ctx.lib.xb_head_grad(ctx.h, y.ctypes.data, dy.ctypes.data, x_hi.ctypes.data, None, y.shape[0] * n,
                                        dw.ctypes.data, db.ctypes.data))
    ctx.close()


def test_refuses_a_head_that_is_not_three_products():
    ctx = _context(32, 64, precision=_lib.XB_PREC_F16F8)
    a = H.inputs(21, 64, 32)
    with pytest.raises(_lib.XbError, match="three fp16 products"):
        ctx.head_grad(*a)
    ctx.close()
