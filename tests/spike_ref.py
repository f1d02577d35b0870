"""A plain-Python / numpy restatement of xb_spike_chunks' contract (include/xna_basecaller.h): the reference's synthetic
spiking (ub-bonito/bonito/spike_chunks.py: spike_read, spike_chunk, sim_signals, compute_med_mad_squiggly) with the contract's
counter-based draws, its own logarithm and AS241's PPND16.  Test infrastructure only: float64 written out operation by
operation; the squiggle's draws are vectorised in uint64, everything else is scalar."""
import math
import struct

import numpy as np

import splice_ref
from splice_ref import GOLDEN_GAMMA, mix

KMER_LEN = 6
KMER_REPS = 100
FLT_EPSILON = 2.0 ** -23
LN2_HI = 6.93147180369123816490e-01
LN2_LO = 1.90821492927058770002e-10
SQRT2 = 1.4142135623730951
LOG_COEFFS = [1.0 / d for d in (19.0, 17.0, 15.0, 13.0, 11.0, 9.0, 7.0, 5.0, 3.0)]


def stream_base(seed, chunk, stream):
    return mix(mix(int(seed) + GOLDEN_GAMMA * (int(chunk) + 1)) + GOLDEN_GAMMA * (int(stream) + 1))


class Stream:
    """Stream s of chunk c: draw k is z = mix(base + G (k + 1)), addressed by k."""

    def __init__(self, seed, chunk, stream):
        self.base = stream_base(seed, chunk, stream)

    def z(self, k):
        return mix(self.base + GOLDEN_GAMMA * (int(k) + 1))

    def bounded(self, k, m):
        return ((self.z(k) >> 32) * int(m)) >> 32

    def unit(self, k):
        return (self.z(k) >> 11) * 2.0 ** -53

    def units(self, k0, count):
        """unit(k0), .., unit(k0 + count - 1) as a float64 array."""
        with np.errstate(over="ignore"):
            z = np.uint64(self.base) + np.uint64(GOLDEN_GAMMA) * (np.arange(count, dtype=np.uint64) + np.uint64(k0 + 1))
            z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
            z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
            z = z ^ (z >> np.uint64(31))
        return (z >> np.uint64(11)).astype(np.float64) * 2.0 ** -53


class Sequential:
    """Stream 0 as splice_ref.Draws spends it: next() is draw k = 0, 1, .."""

    def __init__(self, seed, chunk):
        self.stream, self.k = Stream(seed, chunk, 0), 0

    def next(self):
        self.k += 1
        return self.stream.z(self.k - 1)

    def bounded(self, m):
        return ((self.next() >> 32) * int(m)) >> 32

    def unit(self):
        return (self.next() >> 11) * 2.0 ** -53


def xb_log(x):
    """The contract's logarithm of a positive, finite, normal float64."""
    bits = struct.unpack("<Q", struct.pack("<d", x))[0]
    e = (bits >> 52) - 1023
    m = struct.unpack("<d", struct.pack("<Q", (bits & 0x000FFFFFFFFFFFFF) | 0x3FF0000000000000))[0]
    if m > SQRT2:
        m = m * 0.5
        e = e + 1
    f = m - 1.0
    s = f / (2.0 + f)
    z = s * s
    q = 1.0 / 21.0
    for c in LOG_COEFFS:
        q = q * z + c
    t = (s * z) * q
    logm = 2.0 * (s + t)
    de = float(e)
    return de * LN2_HI + (logm + de * LN2_LO)


def ppnd16(p, log=xb_log):
    """AS241 PPND16 with the coefficients and operation order of CPython's statistics._normal_dist_inv_cdf (mu 0, sigma 1)."""
    q = p - 0.5
    if math.fabs(q) <= 0.425:
        r = 0.180625 - q * q
        num = (((((((2.5090809287301226727e+3 * r + 3.3430575583588128105e+4) * r + 6.7265770927008700853e+4) * r +
                  4.5921953931549871457e+4) * r + 1.3731693765509461125e+4) * r + 1.9715909503065514427e+3) * r +
                1.3314166789178437745e+2) * r + 3.3871328727963666080e+0) * q
        den = (((((((5.2264952788528545610e+3 * r + 2.8729085735721942674e+4) * r + 3.9307895800092710610e+4) * r +
                  2.1213794301586595867e+4) * r + 5.3941960214247511077e+3) * r + 6.8718700749205790830e+2) * r +
                4.2313330701600911252e+1) * r + 1.0)
        return num / den
    r = p if q <= 0.0 else 1.0 - p
    r = math.sqrt(-log(r))
    if r <= 5.0:
        r = r - 1.6
        num = (((((((7.74545014278341407640e-4 * r + 2.27238449892691845833e-2) * r + 2.41780725177450611770e-1) * r +
                  1.27045825245236838258e+0) * r + 3.64784832476320460504e+0) * r + 5.76949722146069140550e+0) * r +
                4.63033784615654529590e+0) * r + 1.42343711074968357734e+0)
        den = (((((((1.05075007164441684324e-9 * r + 5.47593808499534494600e-4) * r + 1.51986665636164571966e-2) * r +
                  1.48103976427480074590e-1) * r + 6.89767334985100004550e-1) * r + 1.67638483018380384940e+0) * r +
                2.05319162663775882187e+0) * r + 1.0)
    else:
        r = r - 5.0
        num = (((((((2.01033439929228813265e-7 * r + 2.71155556874348757815e-5) * r + 1.24266094738807843860e-3) * r +
                  2.65321895265761230930e-2) * r + 2.96560571828504891230e-1) * r + 1.78482653991729133580e+0) * r +
                5.46378491116411436990e+0) * r + 6.65790464350110377720e+0)
        den = (((((((2.04426310338993978564e-15 * r + 1.42151175831644588870e-7) * r + 1.84631831751005468180e-5) * r +
                  7.86869131145613259100e-4) * r + 1.48753612908506148525e-2) * r + 1.36929880922735805310e-1) * r +
                5.99832206555888793690e-1) * r + 1.0)
    x = num / den
    return -x if q < 0.0 else x


def letters_with_tail(tgt):
    """target[:length] + ATATA (TATAT when the last letter is A), as labels."""
    return list(tgt) + ([1, 4, 1, 4, 1] if tgt[-1] != 1 else [4, 1, 4, 1, 4])


def kmer_index(labels):
    t = 0
    for v in labels:
        t = t * 7 + min(int(v), 6)
    return t


def median_even(values):
    """numpy.median of an even count: (a + b) / 2.0 of the two middle order statistics (-0 counted as +0)."""
    v = np.sort(np.asarray(values, dtype=np.float64) + 0.0)
    half = len(v) // 2
    return float((v[half - 1] + v[half]) / 2.0)


def med_mad(tgt, model, seed, chunk):
    mean, stdv = model
    idx = np.array([kmer_index(letters_with_tail(tgt)[i:i + KMER_LEN]) for i in range(len(tgt))])
    means, s = np.repeat(mean[idx], KMER_REPS), np.repeat(stdv[idx], KMER_REPS)
    lo = -s
    x = means + (lo + (s - lo) * Stream(seed, chunk, 1).units(0, len(means)))
    med = median_even(x)
    return med, median_even(np.absolute(x - med)) * 1.4826 + FLT_EPSILON


def spike_chunk(signal, target, length, bkp, model, chunk_index, seed, ubs_mask, prop, var_prop, pad, dist_rows, phi, noise_std,
                variable_noise, stats=None):
    """One chunk -> (signal float32, target uint8, spiked, med, mad, status).  model: (mean, stdv) of 7^6 k-mers; phi:
    (dist_rows + 1, 2) float64; stats (a dict) collects 'positions', 'ubs' and 'empty' (k-mers without a sample)."""
    out = np.array(signal, dtype=np.float32)
    out_t = np.array(target, dtype=np.uint8)
    length = max(0, min(int(length), len(out_t)))
    N = len(out)
    stats = {} if stats is None else stats
    stats.setdefault("positions", [])
    stats.setdefault("ubs", [])
    stats.setdefault("empty", 0)
    if length == 0:
        return out, out_t, 0, 0.0, 0.0, 0
    mean, stdv = model
    tgt = [min(int(v), 6) for v in np.asarray(target)[:length]]
    b = [min(int(v), N) for v in np.asarray(bkp)[:length]]
    full = letters_with_tail(tgt)

    def missing(index):
        return out, out_t, 0, float(index), float("nan"), 2

    for i in range(length):
        if math.isnan(mean[kmer_index(full[i:i + KMER_LEN])]):
            return missing(kmer_index(full[i:i + KMER_LEN]))

    draws = Sequential(seed, chunk_index)
    if var_prop is not None and var_prop > 0:
        lo, hi = prop - var_prop, prop + var_prop
        prop = lo + (hi - lo) * draws.unit()
    ubs_pos = [p for p in range(length) if tgt[p] > 4]
    n_pos = max(splice_ref.rint(float(length) * float(prop)) - len(ubs_pos), 1)
    positions = splice_ref.choose_positions(length, n_pos, pad, ubs_pos, draws)
    n = len(positions)
    if ubs_mask == 3:
        ubs = [5 + (i & 1) for i in range(n + n % 2)]
        for i in range(len(ubs) - 1, 0, -1):
            j = draws.bounded(i + 1)
            ubs[i], ubs[j] = ubs[j], ubs[i]
        ubs = ubs[:n]
    else:
        ubs = [0 if ubs_mask == 0 else 4 + ubs_mask] * n
    stats["positions"].append(positions)
    stats["ubs"].append(ubs)

    windows = []
    for pos, ub in zip(positions, ubs):
        st = tgt[pos - KMER_LEN + 1:pos + KMER_LEN]
        if ub:
            st[KMER_LEN - 1] = ub
        idx = [kmer_index(st[i:i + KMER_LEN]) for i in range(KMER_LEN)]
        for t in idx:
            if math.isnan(mean[t]):
                return missing(t)
        windows.append(idx)

    med, mad = med_mad(tgt, model, seed, chunk_index)
    for ordinal, (pos, ub, idx) in enumerate(zip(positions, ubs, windows)):
        stream = Stream(seed, chunk_index, 2 + ordinal)
        cuts = [b[pos - KMER_LEN]]                          # what the _dev form clamps: at most N, non-decreasing in the window
        for i in range(KMER_LEN):
            cuts.append(max(b[pos - KMER_LEN + 1 + i], cuts[-1]))
        first = cuts[0]
        reps = [cuts[i + 1] - cuts[i] for i in range(KMER_LEN)]
        stats["empty"] += sum(r == 0 for r in reps)
        n_win = sum(reps)
        if dist_rows > 0:
            pa, pw = (float(v) for v in phi[stream.bounded(0, dist_rows)])
        sigma = float(noise_std)
        if noise_std > 0 and variable_noise:
            sigma = 0.0 + (float(noise_std) - 0.0) * stream.unit(1)
        na, nw = (float(v) for v in phi[dist_rows])
        i = 0
        for q in range(KMER_LEN):
            m, s = float(mean[idx[q]]), float(stdv[idx[q]])
            for _ in range(reps[q]):
                u = stream.unit(2 + i)
                if dist_rows == 0:
                    lo = -s
                    level = lo + (s - lo) * u
                else:
                    level = ppnd16(pa + u * pw) * s
                v = m + level
                if noise_std > 0:
                    v = v + ppnd16(na + stream.unit(2 + n_win + i) * nw) * sigma
                out[first + i] = np.float32((v - med) / mad)
                i += 1
        if ub:
            out_t[pos] = ub
    return out, out_t, n, med, mad, 0


def spike_batch(model):
    """A stand-in for Context.spike_chunks over `model` (what spike.spike takes as `run=`)."""
    def run(signal, targets, lengths, bkps, first_index, seed, ubs_mask, prop, var_prop=0.0, pad=5, dist_rows=0, phi=None,
            noise_std=0.0, variable_noise=False):
        n = signal.shape[0]
        phi = np.zeros((1, 2)) if phi is None else np.asarray(phi, dtype=np.float64).reshape(-1, 2)
        out, out_t = np.empty(signal.shape, np.float32), np.empty(targets.shape, np.uint8)
        spiked, status = np.zeros(n, np.int32), np.zeros(n, np.int8)
        med, mad = np.zeros(n), np.zeros(n)
        for c in range(n):
            out[c], out_t[c], spiked[c], med[c], mad[c], status[c] = spike_chunk(
                signal[c], targets[c], lengths[c], bkps[c], model, first_index + c, seed, ubs_mask, prop, var_prop, pad, dist_rows,
                phi, noise_std, variable_noise)
        return out, out_t, spiked, med, mad, status
    return run
