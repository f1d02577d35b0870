"""CPU: the weight packer (csrc/xb_pack.h, reached through libxnacall.so's non-public xb_internal_* exports) against the
roundings tests/encoder_f64.py restates (to_e4m3, split_rows_exp, to_i8_rows) and the layouts tests/pack_ref.py restates --
exactly, byte for byte, where the GPU tests meet the same code only through whole encoder runs under a score tolerance."""
import numpy as np
import pytest

import host_logic as hl
import pack_ref
from encoder_f64 import split_rows_exp, to_e4m3, to_i8_rows

SHAPES = [(3, 40, 64), (5, 304, 320)]           # rows, cols, ld; the second is the conv3 weight (16 x 19 columns, kp 320)


def _tensors(rows, cols):
    """name -> (rows, cols) float32: random weights, then the values the roundings can go wrong at."""
    rng = np.random.default_rng(rows * cols)
    base = (rng.standard_normal((rows, cols)) * 0.3).astype(np.float32)
    out = {"random": base, "zero": np.zeros((rows, cols), np.float32)}
    # the maximum on either side of a power of two and on it: 448 / max crosses 2 at 224, the exponent steps from 0 to -1
    for name, top in (("max-below", 223.9), ("max-on", 224.0), ("max-above", 224.1)):
        w = base.copy()
        w[rows - 1, cols - 1] = -top
        out[name] = w
    # exponent 0 (maximum 200): +-0, e4m3 subnormals (steps of 2^-9 below 2^-6) and their ties, ties between e4m3 neighbours
    # (1.0625 -> 1.0, 1.1875 -> 1.25, 108 -> 112, 116 -> 112: to the even code), two values with an fp16 residual
    w = base.copy()
    w[0, :24] = [0.0, -0.0, 2.0 ** -9, -2.0 ** -9, 2.0 ** -10, 3 * 2.0 ** -10, 5 * 2.0 ** -10, -7 * 2.0 ** -10, 2.0 ** -11, 2.0 ** -6,
                 2.0 ** -6 - 2.0 ** -10, 2.0 ** -6 + 2.0 ** -10, 1.0625, 1.1875, -1.0625, 1.3125, 200.0, 104.0, 108.0, -116.0,
                 1.0 + 2.0 ** -11, 1.0 + 3 * 2.0 ** -11, 1e-3, -3.3e-5]
    out["edges"] = w
    return out


@pytest.mark.parametrize("rows,cols,ld", SHAPES)
def test_split_rows_fp16_residual(rows, cols, ld):
    for name, w in _tensors(rows, cols).items():
        hi, lo, _ = hl.split_rows(w, ld)
        want_hi = w.astype(np.float16)
        want_lo = (w - want_hi.astype(np.float32)).astype(np.float16)              # the fp32 residual, rounded to fp16
        assert np.array_equal(hi[:, :cols].view(np.uint16), want_hi.view(np.uint16)), name
        assert np.array_equal(lo[:, :cols].view(np.uint16), want_lo.view(np.uint16)), name
        assert not hi[:, cols:].view(np.uint16).any() and not lo[:, cols:].view(np.uint16).any(), name
    assert np.abs(want_lo).max() > 0


@pytest.mark.parametrize("rows,cols,ld", SHAPES)
def test_split_rows_q8_image(rows, cols, ld):
    exps = {}
    for name, w in _tensors(rows, cols).items():
        hi, img, e = hl.split_rows(w, ld, q8=True)
        exps[name] = e
        assert e == split_rows_exp(w), name
        want_hi = w.astype(np.float16)
        assert np.array_equal(hi[:, :cols].view(np.uint16), want_hi.view(np.uint16)) and not hi[:, cols:].view(np.uint16).any(), name
        # per row and 32 columns [32 x e4m3(hi * 2^e) | 32 x e4m3(lo * 2^(e + 11))], lo the fp32 residual of hi
        h8 = pack_ref.e4m3_decode(img[:, :, :32]).reshape(rows, ld)
        l8 = pack_ref.e4m3_decode(img[:, :, 32:]).reshape(rows, ld)
        res = (w - want_hi.astype(np.float32)).astype(np.float64)
        want_h8, want_l8 = to_e4m3(want_hi.astype(np.float64) * 2.0 ** e), to_e4m3(res * 2.0 ** (e + 11))
        for got, want in ((h8, want_h8), (l8, want_l8)):
            assert np.array_equal(got[:, :cols], want), name
            assert np.array_equal(np.signbit(got[:, :cols]), np.signbit(want)), name
            assert not got[:, cols:].any() and not np.signbit(got[:, cols:]).any(), name
        if name == "edges":
            assert e == 0
            assert h8[0, :20].tolist() == [0.0, -0.0, 2.0 ** -9, -2.0 ** -9, 0.0, 2.0 ** -8, 2.0 ** -8, -2.0 ** -7, 0.0, 2.0 ** -6,
                                           2.0 ** -6, 2.0 ** -6, 1.0, 1.25, -1.0, 1.25, 192.0, 104.0, 112.0, -112.0]
            assert l8[0, 20] == 1.0 and l8[0, 21] == -1.0 and np.count_nonzero(l8[0, :20]) == 0      # 2^-11 * 2^11; 1 + 3 * 2^-11 -> 1 + 2^-9 - 2^-11
    assert (exps["zero"], exps["max-below"], exps["max-on"], exps["max-above"]) == (0, 0, 0, -1)


def test_f32_to_e4m3_round_trips_every_code():
    codes = np.arange(256, dtype=np.uint8)
    values = pack_ref.e4m3_decode(codes)
    for code, v in zip(codes.tolist(), values.tolist()):
        if code & 0x7f == 0x7f:                       # the two NaN codes: what a NaN encodes to, sign kept
            assert hl.f32_to_e4m3(np.copysign(np.nan, v)) == code
        else:
            assert hl.f32_to_e4m3(v) == code, code
    assert np.array_equal(to_e4m3(values[codes & 0x7f != 0x7f]), values[codes & 0x7f != 0x7f])       # the restatement agrees on them
    assert hl.f32_to_e4m3(1e9) == 0x7e and hl.f32_to_e4m3(-np.inf) == 0xfe and hl.f32_to_e4m3(464.0) == 0x7e


def test_i8_limbs():
    rng = np.random.default_rng(5)
    w = (rng.standard_normal((12, 96)) * 0.2).astype(np.float32)
    w[3] = 0.0                                        # a zero row: scale 1
    w[4, :3] = [w[4].max() * 4, -0.0, 1e-9]
    d1, d0, sc = hl.i8_limbs(w)
    s = np.abs(w).max(axis=1, keepdims=True)
    s[s == 0] = 1.0
    assert s.dtype == np.float32 and s[3, 0] == 1.0
    q = np.rint((w / s) * np.float32(32512.0))        # float32, operation by operation
    assert q.dtype == np.float32
    assert np.array_equal(256 * d1.astype(np.int64) + d0, q.astype(np.int64))
    # both digits in [-128, 127]: int8 by type, and the low one the balanced remainder, so that the high one needs no more
    qi = q.astype(np.int64)
    assert d1.dtype == np.int8 and d0.dtype == np.int8 and np.array_equal(d0, ((qi + 128) & 255) - 128)
    assert np.abs(qi).max(axis=1).tolist() == [32512] * 3 + [0] + [32512] * 8 and np.abs(d1).max() == 127
    assert np.array_equal(sc, s[:, 0] / (np.float32(32512.0) * np.float32(32512.0)))
    assert not d1[3].any() and not d0[3].any()


def test_i8_limbs_high_digit_equals_the_restatement():
    """encoder_f64.to_i8_rows keeps 256 d1 of the float64 quotient: compared where float32 and float64 compute w / s * 32512
    alike -- a row maximum that is a power of two and weights on a 2^-12 grid of it, so that both are exact."""
    rng = np.random.default_rng(6)
    w = (rng.integers(-4096, 4097, size=(8, 64)) * 2.0 ** -12).astype(np.float32)
    w[:, 0] = 1.0
    w *= (2.0 ** np.arange(-4, 4))[:, None].astype(np.float32)
    d1, d0, sc = hl.i8_limbs(w)
    s = np.abs(w).max(axis=1, keepdims=True).astype(np.float64)
    assert np.array_equal(256.0 * d1 * s / 32512.0, to_i8_rows(w))
    assert d0.any()


def test_gate_interleave():
    F = 32
    rng = np.random.default_rng(7)
    wih, whh = (rng.standard_normal((4 * F, F)).astype(np.float32) for _ in range(2))
    bih, bhh = (rng.standard_normal(4 * F).astype(np.float32) for _ in range(2))
    wi, wh, bb = hl.gate_interleave(wih, whh, bih, bhh)
    for unit in range(F):
        for gate in range(4):                        # row' = unit * 4 + gate  <-  row = gate * F + unit
            assert np.array_equal(wi[unit * 4 + gate], wih[gate * F + unit])
            assert np.array_equal(wh[unit * 4 + gate], whh[gate * F + unit])
    assert bb.dtype == np.float32 and np.array_equal(bb.reshape(F, 4), (bih + bhh).reshape(4, F).T)


@pytest.mark.parametrize("nsplit", [1, 2, 3])
@pytest.mark.parametrize("rows,K", [(33, 32), (33, 64), (256, 32), (256, 64)])
def test_fragment_major(rows, K, nsplit):
    # every 2-byte element its own value (hi even, lo odd), so that a piece in the wrong place cannot pass
    order = np.random.default_rng(rows + K).permutation(32768)[:2 * rows * K].astype(np.uint16).reshape(2, rows, K)
    hi, lo = 2 * order[0], 2 * order[1] + 1
    got, kstride = hl.fragment_major(hi, lo, rows, K, nsplit)
    want, want_stride = pack_ref.fragment_major(hi, lo, rows, K, nsplit)
    assert kstride == want_stride == 256 // 32 * (2 if nsplit == 1 else 4) * 1024
    assert got.size == want.size == K // 32 * kstride
    got = got.reshape(want.shape)
    assert np.array_equal(got, want)
    # rows from `rows` up to the padded 256 are zero: per 32-row block, whichever lanes hold them
    blocks_with_rows = -(-rows // 32)
    assert not got[:, blocks_with_rows:].any()
    assert got[:, :blocks_with_rows].any(axis=(2, 3, 4)).all()
    if rows == 33:                                    # block 1 holds row 32 alone
        lanes = got[:, 1].any(axis=(0, 1, 3))
        assert lanes.tolist() == [l % (16 if nsplit == 3 else 32) == 0 for l in range(64)]
