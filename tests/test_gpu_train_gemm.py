"""GPU: the fp32 products of training (csrc/xb_train_gemm.hip) -- xb_linear_f32_dev, xb_wgrad_f32_dev, xb_head_dz_dev.

The products are held to float64 numpy.  The tolerance is measured, not chosen, by the rule of tests/test_gpu_lstm_train.py: the
error of torch in float32 on the CPU against the same float64 result on the same float32 inputs, per tensor and relative to the
tensor's maximum -- the device must stay within MARGIN = 8 times that.  Every comparison prints both errors.

  linear   M in {1, 17, 65} x N in {16, 48, 125} x K in {16, 125, 200} (a lone row, a ragged row tile, one past a workgroup's 64
           rows; one column tile, a ragged one, two; k of one chunk, ragged with rows that are not 16-byte aligned, several
           staging rounds), both activations, with and without bias; rows 0..16 of M = 65 are the bytes of M = 17; a repeated
           call; +-1e4 under tanh.  The widths of a real step at M = 17, with bias, both activations: (N, K) = (3072, 768) gin,
           (768, 3072) dx, (1296, 768) the scores, (768, 1296) the head's dX, (768, 625) the same at C = 625, whose rows are not
           16-byte aligned -- column tiles up to 47, up to 96 staging rounds; and the scores and the head's dX at the other
           head widths a context takes, 216, 1024, 3125 (rows not 16-byte aligned) and 4096.  The launch seam: M = 64 * 65535 + 65 rows are two
           launches; all of it against float64, and the last 129 rows (the last tile before the seam, the second launch) are
           the bytes of a call on those rows alone
  wgrad    M in {0, 1, 5, 130, 20000} x (N, K) in {(16, 16), (125, 48), (200, 125)} (20000 rows: 19 blocks of the blocked sum and
           a ragged one; not at (200, 125)), dcol included; M = 0 and a gradient of zeros give zero bytes; a repeated call; the
           shifted operands of dW_hh in both directions.  The widths of a real step at M = 130, dcol included: (N, K) =
           (3072, 768) dW_ih and dW_hh, (1296, 768) the head, (625, 768) the head at C = 625 (rows of a not 16-byte aligned), and at C = 216, 3125 and 4096
  dz       bit-equal to numpy operation by operation, |y| = scale included"""
import functools

import numpy as np
import pytest
import torch

import lstm_train_ref as R
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MARGIN = 8.0
SCALE = 5.0
LINEAR = [(M, N, K) for M in (1, 17, 65) for N in (16, 48, 125) for K in (16, 125, 200)]
WGRAD = [(M, N, K) for M in (0, 1, 5, 130, 20000) for N, K in ((16, 16), (125, 48), (200, 125)) if not (M == 20000 and N == 200)]
LINEAR_REAL = [(3072, 768), (768, 3072), (1296, 768), (768, 1296), (768, 625)]
WGRAD_REAL = [(3072, 768), (1296, 768), (625, 768)]
# the head widths of the other (n_base, state_len) pairs: 216 (6, 2), 1024 (4, 4), 3125 (5, 4), 4096 (4, 5)
LINEAR_REAL += [(216, 768), (768, 216), (1024, 768), (3125, 768), (768, 3125), (4096, 768), (768, 4096)]
WGRAD_REAL += [(216, 768), (3125, 768), (4096, 768)]
SEAM_ROWS = 64 * 65535                 # rows of one launch of xb_linear_f32: 65535 blocks of 64 in the grid's y dimension
RATIOS = []


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0, 4, 2, 32, 19, 5, 5.0, 2.0, 100, 1)        # the products use the context's stream only
    yield c
    c.close()
    if RATIOS:
        print("largest ratio to torch float32: %.2f (%s)" % max(RATIOS))


def _dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)


def held(what, got, ref, yard):
    err = R.rel(got, ref)
    ratio = err / yard if yard else (0.0 if err == 0.0 else float("inf"))
    RATIOS.append((ratio, what))
    print("%-34s device %.3g  torch float32 %.3g  ratio %.2f" % (what, err, yard, ratio))
    assert np.isfinite(got).all(), what
    assert err <= MARGIN * yard, (what, err, yard)


# ---- linear --------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def linear_case(N, K):
    """Inputs for the largest M (smaller M are its first rows), the float64 results and torch float32's, for (act, bias)."""
    rng = np.random.default_rng(1000 * N + K)
    a = rng.standard_normal((65, K)).astype(np.float32)
    w = rng.uniform(-2.0 / np.sqrt(K), 2.0 / np.sqrt(K), (N, K)).astype(np.float32)
    b = (0.5 * rng.standard_normal(N)).astype(np.float32)
    out = {}
    for act in (0, 1):
        for bias in (False, True):
            z = a.astype(np.float64) @ w.astype(np.float64).T + (b.astype(np.float64) if bias else 0.0)
            zt = torch.nn.functional.linear(torch.from_numpy(a), torch.from_numpy(w), torch.from_numpy(b) if bias else None)
            out[act, bias] = (SCALE * np.tanh(z) if act else z, (SCALE * torch.tanh(zt) if act else zt).numpy())
    for x in (a, w, b):
        x.setflags(write=False)
    return a, w, b, out


def dev_linear(ctx, a, w, b, act, scale=SCALE):
    M, K = a.shape
    N = w.shape[0]
    da, dw, db = _dev(a), _dev(w), (None if b is None else _dev(b))
    out = torch.full((M, N), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.linear_f32_dev(da.data_ptr(), dw.data_ptr(), None if b is None else db.data_ptr(), M, N, K, act, scale, out.data_ptr())
    ctx.synchronize()
    return out.cpu().numpy()


@pytest.mark.parametrize("M,N,K", LINEAR)
def test_linear_against_float64(ctx, M, N, K):
    a, w, b, out = linear_case(N, K)
    for (act, bias), (ref, t32) in out.items():
        got = dev_linear(ctx, a[:M], w, b if bias else None, act)
        held("linear M%d N%d K%d act%d bias%d" % (M, N, K, act, bias), got, ref[:M], R.rel(t32[:M], ref[:M]))


@pytest.mark.parametrize("N,K", LINEAR_REAL)
def test_linear_at_the_widths_of_a_real_step(ctx, N, K):
    a, w, b, out = linear_case(N, K)
    for act in (0, 1):
        ref, t32 = out[act, True]
        got = dev_linear(ctx, a[:17], w, b, act)
        held("linear M17 N%d K%d act%d bias1" % (N, K, act), got, ref[:17], R.rel(t32[:17], ref[:17]))


def test_linear_across_the_launch_seam(ctx):
    M, N, K = SEAM_ROWS + 65, 8, 8
    rng = np.random.default_rng(65535)
    a = rng.standard_normal((M, K), dtype=np.float32)
    w = rng.uniform(-2.0 / np.sqrt(K), 2.0 / np.sqrt(K), (N, K)).astype(np.float32)
    b = (0.5 * rng.standard_normal(N)).astype(np.float32)
    ref = a.astype(np.float64) @ w.astype(np.float64).T + b.astype(np.float64)
    t32 = torch.nn.functional.linear(torch.from_numpy(a), torch.from_numpy(w), torch.from_numpy(b)).numpy()
    got = dev_linear(ctx, a, w, b, 0)
    held("linear M%d N%d K%d act0 bias1" % (M, N, K), got, ref, R.rel(t32, ref))
    assert SEAM_ROWS - 64 <= M - 129 < SEAM_ROWS < M                   # the rows compared lie on both sides of the seam
    assert got[M - 129:].tobytes() == dev_linear(ctx, a[M - 129:], w, b, 0).tobytes()


@pytest.mark.parametrize("N,K", [(48, 125), (125, 200)])
def test_linear_rows_do_not_depend_on_the_batch_and_repeat(ctx, N, K):
    a, w, b, _ = linear_case(N, K)
    for act in (0, 1):
        whole, part = dev_linear(ctx, a, w, b, act), dev_linear(ctx, a[:17], w, b, act)
        assert np.ascontiguousarray(whole[:17]).tobytes() == part.tobytes()
        assert dev_linear(ctx, a, w, b, act).tobytes() == whole.tobytes()


def test_linear_saturated_tanh_stays_finite(ctx):
    a, w, b, _ = linear_case(125, 200)
    big = np.where(np.arange(125) % 2 == 0, np.float32(1e4), np.float32(-1e4)).astype(np.float32)
    got = dev_linear(ctx, a[:17], w, big, 1)
    assert np.isfinite(got).all() and np.abs(got).max() <= SCALE
    assert np.array_equal(got, np.broadcast_to(np.sign(big) * np.float32(SCALE), got.shape))


# ---- wgrad ---------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def wgrad_case(M, N, K):
    rng = np.random.default_rng(7 * M + 1000 * N + K)
    a = rng.standard_normal((M, N)).astype(np.float32)
    b = rng.standard_normal((M, K)).astype(np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    ta, tb = torch.from_numpy(a), torch.from_numpy(b)
    ref = (a64.T @ b64, a64.sum(axis=0))
    t32 = ((ta.t() @ tb).numpy(), ta.sum(dim=0).numpy())
    a.setflags(write=False)
    b.setflags(write=False)
    return a, b, ref, t32


def dev_wgrad(ctx, a, b, N, K, want_col=True, block_rows=None):
    M = a.shape[0]
    da, db = _dev(a), _dev(b)
    dw = torch.full((N, K), float("nan"), dtype=torch.float32, device=DEV)
    dcol = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.wgrad_f32_dev(da.data_ptr() if M else None, db.data_ptr() if M else None, M, N, K, dw.data_ptr(), dcol.data_ptr() if want_col else None,
                      block_rows=block_rows)
    ctx.synchronize()
    return dw.cpu().numpy(), dcol.cpu().numpy()


@pytest.mark.parametrize("M,N,K", WGRAD)
def test_wgrad_against_float64(ctx, M, N, K):
    a, b, ref, t32 = wgrad_case(M, N, K)
    dw, dcol = dev_wgrad(ctx, a, b, N, K)
    if M == 0:
        assert dw.tobytes() == bytes(dw.nbytes) and dcol.tobytes() == bytes(dcol.nbytes)
        return
    held("wgrad M%d N%d K%d dw" % (M, N, K), dw, ref[0], R.rel(t32[0], ref[0]))
    held("wgrad M%d N%d K%d dcol" % (M, N, K), dcol, ref[1], R.rel(t32[1], ref[1]))
    again = dev_wgrad(ctx, a, b, N, K)
    assert again[0].tobytes() == dw.tobytes() and again[1].tobytes() == dcol.tobytes()
    only = dev_wgrad(ctx, a, b, N, K, want_col=False)
    assert only[0].tobytes() == dw.tobytes() and np.isnan(only[1]).all()


@pytest.mark.parametrize("N,K", WGRAD_REAL)
def test_wgrad_at_the_widths_of_a_real_step(ctx, N, K):
    a, b, ref, t32 = wgrad_case(130, N, K)
    dw, dcol = dev_wgrad(ctx, a, b, N, K)
    held("wgrad M130 N%d K%d dw" % (N, K), dw, ref[0], R.rel(t32[0], ref[0]))
    held("wgrad M130 N%d K%d dcol" % (N, K), dcol, ref[1], R.rel(t32[1], ref[1]))


@pytest.mark.parametrize("M", [5, 130])
def test_wgrad_of_a_zero_gradient_gives_zero_bytes(ctx, M):
    _, b, _, _ = wgrad_case(M, 125, 48)
    dw, dcol = dev_wgrad(ctx, np.zeros((M, 125), np.float32), -np.abs(b), 125, 48)
    assert dw.tobytes() == bytes(dw.nbytes) and dcol.tobytes() == bytes(dcol.nbytes)


@pytest.mark.parametrize("reverse", [False, True])
def test_wgrad_shifted_operands_give_dw_hh(ctx, reverse):
    T, n, F = 3, 5, 16
    rng = np.random.default_rng(31 + reverse)
    y = rng.standard_normal((T, n, F)).astype(np.float32)
    dgin = rng.standard_normal((T, n, 4 * F)).astype(np.float32)
    hp = R.h_prev(y.astype(np.float64), reverse).reshape(T * n, F)
    ref = dgin.astype(np.float64).reshape(T * n, 4 * F).T @ hp
    t32 = (torch.from_numpy(dgin).reshape(T * n, 4 * F).t() @ torch.from_numpy(hp.astype(np.float32))).numpy()
    dy_, dg_ = _dev(y), _dev(dgin)
    dw = torch.full((4 * F, F), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    a = dg_.data_ptr() + (0 if reverse else 4 * n * 4 * F)
    b = dy_.data_ptr() + (4 * n * F if reverse else 0)
    ctx.wgrad_f32_dev(a, b, (T - 1) * n, 4 * F, F, dw.data_ptr(), None)
    ctx.synchronize()
    held("dw_hh %s" % ("rev" if reverse else "fwd"), dw.cpu().numpy(), ref, R.rel(t32, ref))


# ---- dz ------------------------------------------------------------------------------------------------------------------------
def test_head_dz_is_its_restatement_bit_for_bit(ctx):
    rng = np.random.default_rng(3)
    count = 3 * 257 + 5
    scale = np.float32(SCALE)
    y = (scale * np.tanh(3.0 * rng.standard_normal(count))).astype(np.float32)
    y[:4] = (scale, -scale, 0.0, np.nextafter(scale, np.float32(0)))
    dy = (rng.standard_normal(count) * np.float32(10.0) ** rng.integers(-9, 1, count)).astype(np.float32)
    ref = dy * (((scale - y) * (scale + y)) / scale)                  # float32 numpy: one rounding per operation
    assert ref.dtype == np.float32 and ref[0] == 0 and ref[1] == 0
    dz = torch.full((count,), float("nan"), dtype=torch.float32, device=DEV)
    d_y, d_dy = _dev(y), _dev(dy)
    torch.cuda.synchronize()
    ctx.head_dz_dev(d_y.data_ptr(), d_dy.data_ptr(), count, float(scale), dz.data_ptr())
    ctx.synchronize()
    assert dz.cpu().numpy().tobytes() == ref.tobytes()
    with pytest.raises(_lib.XbError, match="scale") as e:
        ctx.head_dz_dev(d_y.data_ptr(), d_dy.data_ptr(), count, 0.0, dz.data_ptr())
    assert e.value.code == _lib.XB_ERR_INVALID


def test_refusals_leave_the_context_usable(ctx):
    z = torch.zeros(64, dtype=torch.float32, device=DEV)
    p = z.data_ptr()
    torch.cuda.synchronize()
    for M, N, K, act in ((0, 4, 4, 0), (4, 0, 4, 0), (4, 4, 0, 0), (4, 4, 4, 2)):
        with pytest.raises(_lib.XbError, match="xb_linear_f32") as e:
            ctx.linear_f32_dev(p, p, None, M, N, K, act, 1.0, p)
        assert e.value.code == _lib.XB_ERR_INVALID
    with pytest.raises(_lib.XbError, match="null") as e:
        ctx.linear_f32_dev(None, p, None, 4, 4, 4, 0, 1.0, p)
    for M, N, K in ((-1, 4, 4), (4, 0, 4), (4, 4, 0)):
        with pytest.raises(_lib.XbError, match="xb_wgrad_f32") as e:
            ctx.wgrad_f32_dev(p, p, M, N, K, p, None)
        assert e.value.code == _lib.XB_ERR_INVALID
    a, w, b, out = linear_case(16, 16)
    held("after the refusals", dev_linear(ctx, a[:17], w, b, 0), out[0, True][0][:17], R.rel(out[0, True][1][:17], out[0, True][0][:17]))
