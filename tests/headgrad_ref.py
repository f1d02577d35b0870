"""Numpy restatements of xb_head_grad (include/xna_basecaller.h): the gradient of the CRF head's weight and bias,
dW = dZ^T X and db = sum_m dZ with dZ = dY * (scale - Y^2 / scale), from the RAW blank-less scores Y, their gradient dY and the
head's input X = x_hi + x_lo (fp16 pairs).

  head_grad_f64      everything in float64: the reference the device is held to
  head_grad_kernel   the operands as the kernel rounds them -- dZ in fp32, multiplied by the call's power of two, split into fp16
                     hi + lo; the three products hi*hi + hi*lo + lo*hi -- with the sums in float64: what remains when the fp32
                     accumulation of the MFMA is taken away
  head_grad_single   fp16-rounded dZ against x_hi alone: the arithmetic that a dropped residual product would leave
  bound              the elementwise yardstick 2^-24 (|dZ|^T |X|) and 2^-24 sum |dZ|; a result is within the contract when
                     |result - f64| <= K_BOUND * bound

K_BOUND is 4 x the largest ratio measured on the MI355X over tests/test_gpu_headgrad.py's cases (see there and DESIGN.md 4.2.5)."""
import numpy as np

# MI355X, tests/test_gpu_headgrad.py: the largest |device - float64| / bound over all its cases is 7.94 (features 384, 64 columns,
# one row -- with a single row nothing averages, the ratio is the fp32 rounding of dZ and of the result); 4099 rows give 0.6 - 0.8.
# That was measured at 64, 125 and 1296 columns, and K_MEASURED and K_BOUND stay what it gave.  The widths added since (216, 625,
# 1024, 3125, 4096 columns) reach 5.8 - 8.2, but for 16.3 at one row, 1024 columns, features 96: head_grad_kernel above, whose sums
# are float64, gives 15.7 there, so it is the operands, not the accumulation -- one of that row's 1024 dZ values lies 2^18.4 below the call's
# largest, its lo part (4.2e-7 after the prescale) falls among fp16's subnormals and leaves 14.7 x 2^-24 of dZ behind, and with one
# row no other term covers it: all 96 elements of that output row, and no other, exceed 8.
K_MEASURED = 7.94
K_BOUND = 4 * K_MEASURED


def exponent(dy, scale):
    """The power of two the kernel multiplies dZ by: 14 - frexp's exponent of max|dY| * scale (an fp32 product)."""
    a = np.float32(np.abs(np.asarray(dy, np.float32)).max(initial=np.float32(0))) * np.float32(scale)
    if not (a > 0) or not np.isfinite(a):
        return 0
    return 14 - int(np.frexp(a)[1])


def split16(v):
    """fp32 -> (hi, lo) fp16 with hi = fp16(v), lo = fp16(v - hi)."""
    v = np.asarray(v, np.float32)
    hi = v.astype(np.float16)
    return hi, (v - hi.astype(np.float32)).astype(np.float16)


def planes(x):
    """fp32 X -> the uint16 bit patterns (x_hi, x_lo) the entry point takes."""
    hi, lo = split16(x)
    return hi.view(np.uint16), lo.view(np.uint16)


def x_value(x_hi, x_lo):
    """The float64 value hi + lo of fp16 bit patterns."""
    return np.asarray(x_hi).view(np.float16).astype(np.float64) + np.asarray(x_lo).view(np.float16).astype(np.float64)


def dz_f64(y, dy, scale):
    y, dy = np.asarray(y, np.float64), np.asarray(dy, np.float64)
    return dy * (float(scale) - y * y / float(scale))


def head_grad_f64(y, dy, x_hi, x_lo, scale):
    dz = dz_f64(y, dy, scale)
    return dz.T @ x_value(x_hi, x_lo), dz.sum(axis=0)


def dz_kernel(y, dy, scale, e):
    """(dY * 2^e) * (((scale - Y) * (scale + Y)) / scale), every operation in fp32 on its own: scale - Y^2 / scale in the form that
    does not cancel where tanh saturates."""
    y, dy, s = np.asarray(y, np.float32), np.asarray(dy, np.float32), np.float32(scale)
    return np.ldexp(dy, e).astype(np.float32) * (((s - y) * (s + y)) / s)


def head_grad_kernel(y, dy, x_hi, x_lo, scale, prescale=True):
    e = exponent(dy, scale) if prescale else 0
    dz = dz_kernel(y, dy, scale, e)
    zh, zl = (p.astype(np.float64) for p in split16(dz))
    xh, xl = (np.asarray(p).view(np.float16).astype(np.float64) for p in (x_hi, x_lo))
    dw = zh.T @ xh + zh.T @ xl + zl.T @ xh
    db = dz.astype(np.float64).sum(axis=0)
    return np.ldexp(dw, -e).astype(np.float32), np.ldexp(db, -e).astype(np.float32)


def head_grad_single(y, dy, x_hi, x_lo, scale):
    e = exponent(dy, scale)
    zh = dz_kernel(y, dy, scale, e).astype(np.float16).astype(np.float64)
    xh = np.asarray(x_hi).view(np.float16).astype(np.float64)
    return np.ldexp(zh.T @ xh, -e).astype(np.float32), np.ldexp(zh.sum(axis=0), -e).astype(np.float32)


def bound(y, dy, x_hi, x_lo, scale):
    dz = np.abs(dz_f64(y, dy, scale))
    return 2.0 ** -24 * (dz.T @ np.abs(x_value(x_hi, x_lo))), 2.0 ** -24 * dz.sum(axis=0)


def ratios(got, ref, bnd):
    """max over the elements of |got - ref| / bound, for (dW, db); an element whose bound is 0 must be exact."""
    out = []
    for g, r, b in zip(got, ref, bnd):
        err = np.abs(np.asarray(g, np.float64) - r)
        assert np.all(err[b == 0] == 0), "a value differs where the bound is zero"
        out.append(float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else 0.0)
    return tuple(out)


def inputs(M, O, F, scale=5.0, seed=0, lo=1e-6, hi=1e-3, zero_cols=()):
    """Y = scale tanh(N(0,1)), dY of magnitudes log-uniform in [lo, hi] with random signs (columns `zero_cols` all zero: rows of dW and entries of db that must come out as exact zeros), X uniform in
    (-1, 1) as fp16 planes: what a mean loss over a batch and the last LSTM layer hand the head."""
    rng = np.random.default_rng(seed)
    y = (scale * np.tanh(rng.standard_normal((M, O)))).astype(np.float32)
    mag = np.exp(rng.uniform(np.log(lo), np.log(hi), (M, O)))
    dy = (mag * rng.choice([-1.0, 1.0], (M, O))).astype(np.float32)
    for c in zero_cols:
        dy[:, c] = 0.0
    x_hi, x_lo = planes(rng.uniform(-1.0, 1.0, (M, F)).astype(np.float32))
    return y, dy, x_hi, x_lo
