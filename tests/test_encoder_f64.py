"""CPU: the float64 encoder reference (tests/encoder_f64.py) against the fixtures made by the reference's own modules and
against the fp32 oracle; its defect hooks; the regime of its weight sets; and the discriminating power of the precision
table (tests/encoder_cases.py): every defect a precision claims not to have moves the float64 scores by at least
DISCRIMINATION x that precision's bound, so tests/test_gpu_precision.py would catch it."""
import functools
import json
import os

import numpy as np
import pytest
import torch

import encoder_cases as EC
import geometry_cases as GC
import oracle
from conftest import GOLDEN
from encoder_f64 import (WEIGHTS, Reference, encode, outlier_weights, rnn, sensitive_weights, split_rows_exp, to_e4m3,
                         to_e4m3_tensor, to_f16, to_i8_rows)
from xna_basecaller_amd.synthetic import encoder_shapes, peaky_weights, seeded_state_dict, seeded_weights


@pytest.mark.parametrize("name", ["f32_nb6", "f32_nb4_long", "f48_nb5", "f16_nb4"])
def test_matches_the_golden_fixtures(name):
    meta = json.load(open(os.path.join(GOLDEN, "encoder_meta.json")))
    case = [c for c in meta["cases"] if c["name"] == name][0]
    z = np.load(os.path.join(GOLDEN, "encoder_small.npz"))
    sd = {k: z["%s/w/%s" % (name, k)] for k in case["keys"]}
    r = Reference(z[name + "/signal"][:, 0, :], sd, len(case["labels"]) - 1)
    st = r.run()
    assert np.abs(r.scores() - z[name + "/scores"]).max() < 2e-5
    assert np.abs(st["conv"] - z[name + "/conv_out"].transpose(2, 0, 1)).max() < 2e-5
    assert np.abs(st["lstm0"] - z[name + "/lstm0_out"]).max() < 2e-5
    assert np.abs(st["lstm4"] - z[name + "/lstm4_out"]).max() < 2e-5


# On sensitive and outlier weights the fp32 oracle's own rounding is amplified as much as a kernel's: measured max 1.4e-5 to
# 7.3e-5, rms 1.0e-6 to 1.4e-6 at features 96 to 768 (seeded: 1.2e-6 / 2.2e-7).  There the bound is where the oracle sits.
@pytest.mark.parametrize("weights,tol", [("seeded", (2e-5, 1e-6)), ("sensitive", (2e-5, 3e-6)), ("outlier", (1e-4, 3e-6))])
@pytest.mark.parametrize("features,nb,L,N", [(32, 4, 5, 3), (64, 5, 23, 2), (96, 6, 601, 2), (128, 4, 1003, 2),
                                             (256, 6, 400, 2), (768, 5, 202, 2)])
def test_matches_the_fp32_oracle(features, nb, L, N, weights, tol):
    sd = {"seeded": seeded_weights, "sensitive": sensitive_weights, "outlier": outlier_weights}[weights](features, nb, features + nb)
    x = np.random.default_rng(L).standard_normal((N, L)).astype(np.float32)
    for expand in (True, False):
        ref = oracle.encode(x, sd, features, nb, 3, expand_blanks=expand)
        got = encode(x, sd, nb, expand_blanks=expand)
        assert got.shape == ref.shape
        err = got - ref
        assert np.abs(err).max() < tol[0] and np.sqrt((err ** 2).mean()) < tol[1], (np.abs(err).max(), np.sqrt((err ** 2).mean()))


def test_blank_layout():
    sd = sensitive_weights(32, 4, 1)
    x = np.random.default_rng(0).standard_normal((2, 100))
    r = Reference(x, sd, 4)
    a, b = r.scores(True), r.scores(False)
    assert a.shape == (20, 2, 64 * 5) and b.shape == (20, 2, 64 * 4)
    assert np.all(a.reshape(20, 2, 64, 5)[..., 0] == 2.0)
    assert np.array_equal(a.reshape(20, 2, 64, 5)[..., 1:].reshape(b.shape), b)


def test_roundings():
    # e4m3: 3 mantissa bits, ties to even, subnormal steps of 2^-9, saturation at 448
    assert to_e4m3(np.array([1.0625, 1.1875, 448.0, 1000.0, -3.0 * 2.0 ** -10, 2.0 ** -6 + 2.0 ** -10])).tolist() == \
        [1.0, 1.25, 448.0, 448.0, -2.0 ** -8, 2.0 ** -6]
    w = np.random.default_rng(0).standard_normal((96, 64)) * 0.05
    e = split_rows_exp(w)
    assert 112 < np.abs(w).max() * 2.0 ** e <= 224
    q = to_e4m3_tensor(w)
    assert np.all(np.abs(q - w) <= np.abs(w) * 2.0 ** -4 + 2.0 ** (-10 - e))
    # int8 limbs: the low digit of 16-bit fixed point with the row's max at 32512 is at most 128 units
    q = to_i8_rows(w)
    s = np.abs(w).max(axis=1, keepdims=True) / 32512.0
    assert np.all(np.abs(q - w) <= 128.5 * s) and np.abs(q - w).max() > 64 * s.min()
    assert np.all(np.rint(q / s) % 256 == 0)
    assert np.abs(to_f16(w) - w).max() <= np.abs(w).max() * 2.0 ** -11


def test_defect_hooks_touch_what_they_name():
    F, nb = 32, 4
    sd = sensitive_weights(F, nb, 3)
    x = np.random.default_rng(1).standard_normal((3, 400))
    r = Reference(x, sd, nb)
    clean = r.run()
    # a defect in layer l leaves the stages before it alone and changes the ones after it
    for d, first in [("shift:2", "lstm2"), ("flip:4", "lstm4"), ("a16:rec1", "lstm1"), ("w16:" + rnn(3, "weight_ih_l0"), "lstm3"),
                     ("bhh:order", "lstm0"), ("pad:2", "conv"), ("conv16:1", "conv"), ("a16:linear", "scores")]:
        got = r.run([d])
        order = ["conv"] + ["lstm%d" % l for l in range(5)] + ["scores"]
        i = order.index(first)
        for k in order[:i]:
            assert np.array_equal(got[k], clean[k]), (d, k)
        for k in order[i:]:
            assert not np.array_equal(got[k], clean[k]), (d, k)
    # the cached path equals a fresh computation
    fresh = Reference(x, sd, nb).run(["w16:" + rnn(2, "weight_hh_l0")])
    assert np.array_equal(fresh["scores"], r.run(["w16:" + rnn(2, "weight_hh_l0")])["scores"])
    # flipping a layer twice is the model: flip:0 runs layer 0 forward, i.e. the reversed model on the reversed time axis
    assert not np.array_equal(r.run(["flip:0"])["lstm0"], clean["lstm0"])
    # ignoring bias_hh equals loading zeros into it
    sd0 = dict(sd)
    for l in range(5):
        sd0[rnn(l, "bias_hh_l0")] = np.zeros_like(sd[rnn(l, "bias_hh_l0")])
    assert np.allclose(Reference(x, sd0, nb).run()["scores"], r.run(["bhh:ignore"])["scores"], rtol=0, atol=1e-12)
    with pytest.raises(ValueError):
        r.run(["a16:rec7"])


@pytest.mark.parametrize("weights", ["sensitive", "outlier"])
def test_weight_sets_are_sensitive(weights):
    """The regime of synthetic.peaky_weights: scores follow the signal everywhere, and at the timed size (features 768) a
    called base every 1.4 to 4 time steps; bias_hh non-zero and unlike bias_ih gate by gate."""
    for F, nb in [(32, 4), (128, 6), (768, 5), (768, 6)]:
        sd = WEIGHTS[weights](F, nb, F + nb)
        for l in range(5):
            bih, bhh = sd[rnn(l, "bias_ih_l0")].reshape(4, F), sd[rnn(l, "bias_hh_l0")].reshape(4, F)
            assert np.all(np.abs(bih - bhh).mean(axis=1) > 0.05)
            assert bhh[1].mean() - bhh[0].mean() > 0.1                     # the forget-gate offset
        x = np.random.default_rng(F).standard_normal((3, 1000)).astype(np.float32)
        s = encode(x, sd, nb)
        moved = np.abs(encode(np.roll(x, 1, axis=1), sd, nb) - s).max()
        assert moved >= 0.1, (F, nb, moved)
        if F == 768:
            rate = (oracle.decode(s.astype(np.float32), nb, 3)["labels"] != 0).mean()
            assert 0.25 <= rate <= 0.7, (F, nb, rate)
    if weights == "outlier":
        w = sd[rnn(2, "weight_hh_l0")]
        assert np.abs(w).max() > 16 * np.sqrt((w ** 2).mean())


@functools.lru_cache(maxsize=None)
def _defect_deltas(name):
    """(max, rms) |score change| of every defect in the union of the catalogues, over the case's first two picked chunks."""
    F, nb, L, N, weights = EC.CASES[name]
    sd = WEIGHTS[weights](F, nb, EC.seed_of(name))
    x = np.random.default_rng(L + N).standard_normal((N, L)).astype(np.float32)
    r = Reference(x[EC.picks(N)[:2]], sd, nb)
    clean = r.run()["scores"]
    out = {}
    for d in sorted(set(sum((EC.catalogue(p, F) for p in EC.PRECISIONS), []))):
        e = r.run([d])["scores"] - clean
        out[d] = (float(np.abs(e).max()), float(np.sqrt((e ** 2).mean())))
    return out


def test_table_is_complete():
    assert set(EC.BOUNDS) == set(EC.CASES)
    for name in EC.CASES:
        assert set(EC.BOUNDS[name]) == set(EC.PRECISIONS)
    assert set(EC.LAYER_BOUNDS) == set(EC.PRECISIONS)
    for (name, prec, d), (reason, ratio) in EC.EXCLUDED.items():
        assert d in EC.catalogue(prec, EC.CASES[name][0]) and reason in EC.REASONS and ratio <= EC.DISCRIMINATION     # (ratios rounded to 2 decimals)


@pytest.mark.parametrize("name", list(EC.CASES))
def test_discriminating_power(name):
    F = EC.CASES[name][0]
    deltas = _defect_deltas(name)
    weak = []
    for prec in EC.PRECISIONS:
        bmax, brms = EC.BOUNDS[name][prec]
        for d in EC.catalogue(prec, F):
            dmax, drms = deltas[d]
            ratio = max(dmax / bmax, drms / brms)
            if (name, prec, d) in EC.EXCLUDED:
                continue
            if ratio < EC.DISCRIMINATION:
                weak.append((prec, d, round(ratio, 2)))
    assert not weak, weak


# ---- geometry: state lengths, windows and strides other than (3, 19, 5) -----------------------------------------------------
def _seeded_weights_before(features, n_base, seed=25):
    """seeded_weights as it was before it took state_len and winlen."""
    keys, shapes = encoder_shapes(features, n_base)
    return seeded_state_dict(keys, shapes, seed)


def _peaky_weights_before(features, n_base, seed=25, input_gain=2.0, linear_gain=10.0, blank_bias=2.0):
    """peaky_weights as it was before it took state_len and winlen."""
    sd = _seeded_weights_before(features, n_base, seed)
    for l in range(4, 9):
        k = "encoder.%d.rnn.weight_ih_l0" % l
        sd[k] = (sd[k] * np.float32(input_gain)).astype(np.float32)
        sd["encoder.%d.rnn.bias_ih_l0" % l] = np.zeros_like(sd["encoder.%d.rnn.bias_ih_l0" % l])
    sd["encoder.9.linear.weight"] = (sd["encoder.9.linear.weight"] * np.float32(linear_gain)).astype(np.float32)
    sd["encoder.9.linear.bias"] = np.full_like(sd["encoder.9.linear.bias"], -np.float32(blank_bias))
    return sd


def _sensitive_before(features, nb, seed, outlier):
    """encoder_f64._sensitive as it was before it took state_len and winlen."""
    sd = _peaky_weights_before(features, nb, seed, blank_bias=3.0)
    rng = np.random.default_rng(1000 + seed)
    F = features
    for l in range(5):
        sd[rnn(l, "bias_ih_l0")] = (0.1 * rng.standard_normal(4 * F)).astype(np.float32)
        sd[rnn(l, "bias_hh_l0")] = (0.1 * rng.standard_normal(4 * F) + np.repeat([0.0, 0.2, 0.0, 0.0], F)).astype(np.float32)
    if outlier:
        for k in sorted(sd):
            a = sd[k].astype(np.float64).reshape(-1)
            norm = np.sqrt((a ** 2).sum())
            hit = rng.random(a.size) < 0.003
            hit[rng.integers(a.size)] = True
            a[hit] *= 8.0
            if norm > 0:
                a *= norm / np.sqrt((a ** 2).sum())
            sd[k] = a.reshape(sd[k].shape).astype(np.float32)
    return sd


def _same_bytes(a, b):
    return list(a) == list(b) and all(a[k].dtype == b[k].dtype and a[k].shape == b[k].shape and a[k].tobytes() == b[k].tobytes()
                                      for k in a)


@pytest.mark.parametrize("features,nb", [(32, 4), (96, 6)])
def test_default_geometry_weights_are_unchanged(features, nb):
    """The full-size golden fixtures regenerate their weights from these helpers: with the default state_len and winlen
    every tensor has the bytes it had before the helpers took them."""
    seed = features + nb
    assert _same_bytes(seeded_weights(features, nb, seed), _seeded_weights_before(features, nb, seed))
    assert _same_bytes(seeded_weights(features, nb), _seeded_weights_before(features, nb))
    assert _same_bytes(peaky_weights(features, nb, seed), _peaky_weights_before(features, nb, seed))
    assert _same_bytes(peaky_weights(features, nb, seed, blank_bias=3.0, state_len=3, winlen=19),
                       _peaky_weights_before(features, nb, seed, blank_bias=3.0))
    assert _same_bytes(sensitive_weights(features, nb, seed), _sensitive_before(features, nb, seed, False))
    assert _same_bytes(outlier_weights(features, nb, seed), _sensitive_before(features, nb, seed, True))
    # and the geometry reaches the shapes
    sd = outlier_weights(features, nb, seed, state_len=2, winlen=5)
    assert sd["encoder.2.conv.weight"].shape == (features, 16, 5) and sd["encoder.9.linear.weight"].shape == (nb ** 3, features)


def test_pad_defect_at_window_one_and_late_window():
    F, nb = 32, 4
    x = np.random.default_rng(2).standard_normal((3, 60))
    r = Reference(x, sensitive_weights(F, nb, 3, state_len=2, winlen=1), nb, winlen=1, stride=2)
    clean = r.run()
    assert clean["scores"].shape == (30, 3, 64)
    got = r.run(["pad:2"])                                   # no padding: nothing to take from the neighbours
    assert got["scores"].shape == clean["scores"].shape and np.array_equal(got["conv"], clean["conv"])
    with pytest.raises(ValueError):
        r.run(["win:late"])
    # win:late: the model on the signal advanced by one sample, except where the window meets the chunk's ends
    r = Reference(x, sensitive_weights(F, nb, 3, state_len=2, winlen=5), nb, winlen=5, stride=3)
    w = {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in r.w.items()}
    late = r.run(["win:late"])["conv"]
    clean = r.run()["conv"]
    assert late.shape == clean.shape == (20, 3, F) and not np.array_equal(late, clean)
    h = torch.from_numpy(x)[:, None, :]
    for c in (0, 1):
        h = torch.nn.functional.silu(torch.nn.functional.conv1d(h, w["encoder.%d.conv.weight" % c], w["encoder.%d.conv.bias" % c], padding=2))
    h = torch.nn.functional.pad(h, (1, 3))                   # pad - 1 on the left, pad + 1 on the right
    want = torch.nn.functional.silu(torch.nn.functional.conv1d(h, w["encoder.2.conv.weight"], w["encoder.2.conv.bias"], stride=3))
    assert np.allclose(late, want.permute(2, 0, 1).numpy(), rtol=0, atol=1e-12)


def test_geometry_table_is_complete():
    need = {"windows": {1, 3, 5, 9, 31}, "strides": {1, 2, 3, 6, 8}, "T": {1, 32, 33, 64}, "O": {64, 125, 216, 1024, 3125, 4096}}
    seen = {k: set() for k in need}
    ragged_stride, ragged_batch, corner, short = set(), False, False, False
    for name, (F, nb, sl, W, ST, L, N, weights) in GC.GEOMETRY_CASES.items():
        assert F <= 96 and N <= 70 and L <= 1300 and W % 2 == 1 and 1 <= W <= 31 and 1 <= ST <= 8 and nb ** sl <= 1024
        assert weights in WEIGHTS
        seen["windows"].add(W), seen["strides"].add(ST), seen["T"].add(GC.steps(L, W, ST)), seen["O"].add(nb ** (sl + 1))
        if L % ST:
            ragged_stride.add(ST)
        ragged_batch |= N in (65, 70) and nb ** (sl + 1) >= 1024
        corner |= (W, ST) == (31, 8)
        short |= W == 31 and L == ST
    for k in need:
        assert need[k] <= seen[k], (k, need[k] - seen[k])
    assert {3, 6, 8} <= ragged_stride and ragged_batch and corner and short
    assert set(GC.BOUNDS) == set(GC.MEASURED) == set(GC.GEOMETRY_CASES)
    for name in GC.GEOMETRY_CASES:
        assert set(GC.BOUNDS[name]) == set(GC.PRECISIONS)
        for p in GC.PRECISIONS:                                # 2-3 x the measured error
            assert all(2.0 * m <= b <= 3.0 * m for m, b in zip(GC.MEASURED[name][p], GC.BOUNDS[name][p]))
    for (name, prec, d), (reason, ratio) in GC.EXCLUDED.items():
        assert d in GC.catalogue(prec, GC.GEOMETRY_CASES[name][3]) and reason in EC.REASONS and ratio <= GC.DISCRIMINATION


def _excluded_share(excluded, triples):
    return len(excluded) / float(triples)


def test_geometry_exclusions_stay_within_the_existing_share():
    """The share of (row, precision, defect) triples left out of the discrimination check among the geometry rows may not
    exceed the share among the cases of tests/encoder_cases.py."""
    before = sum(len(EC.catalogue(p, EC.CASES[n][0])) for n in EC.CASES for p in EC.PRECISIONS)
    geo = sum(len(GC.catalogue(p, GC.GEOMETRY_CASES[n][3])) for n in GC.GEOMETRY_CASES for p in GC.PRECISIONS)
    assert _excluded_share(GC.EXCLUDED, geo) <= _excluded_share(EC.EXCLUDED, before), (len(GC.EXCLUDED), geo, len(EC.EXCLUDED), before)


@functools.lru_cache(maxsize=None)
def _geometry_deltas(name):
    F, nb, sl, W, ST, L, N, weights = GC.GEOMETRY_CASES[name]
    sd = WEIGHTS[weights](F, nb, GC.seed_of(name), state_len=sl, winlen=W)
    x = np.random.default_rng(L + N + W).standard_normal((N, L)).astype(np.float32)
    r = Reference(x[EC.picks(N)[:2]], sd, nb, winlen=W, stride=ST)
    clean = r.run()["scores"]
    out = {}
    for d in sorted(set(sum((GC.catalogue(p, W) for p in GC.PRECISIONS), []))):
        e = r.run([d])["scores"] - clean
        out[d] = (float(np.abs(e).max()), float(np.sqrt((e ** 2).mean())))
    return out


@pytest.mark.parametrize("name", list(GC.GEOMETRY_CASES))
def test_geometry_discriminating_power(name):
    W = GC.GEOMETRY_CASES[name][3]
    deltas = _geometry_deltas(name)
    weak = []
    for prec in GC.PRECISIONS:
        bmax, brms = GC.BOUNDS[name][prec]
        for d in GC.catalogue(prec, W):
            dmax, drms = deltas[d]
            ratio = max(dmax / bmax, drms / brms)
            if (name, prec, d) not in GC.EXCLUDED and ratio < GC.DISCRIMINATION:
                weak.append((prec, d, round(ratio, 2)))
    assert not weak, weak
