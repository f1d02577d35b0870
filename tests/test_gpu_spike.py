"""GPU: xb_spike_model / xb_spike_chunks through the C ABI and the `spike` CLI.  The device output EQUALS, bit for bit, what
the restatement of the contract (tests/spike_ref.py) computes -- out_signal (float32 viewed as uint32), out_targets, spiked,
status and the bit patterns of med and mad -- on the golden fixture's cases (where the restatement equals the reference's
spike_chunks.py, tests/test_spike_host.py), on seeded random chunks in every level distribution and on the named edge chunks."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import spike_cases as cases
import splice_cases
from conftest import ROOT

pytestmark = pytest.mark.gpu

SEED = 77
# 64 chunks each: N = 240 takes the 16-byte row copy, 241 the scalar one; lengths run from 12 (no position) to 120, so most
# chunks have one or two positions at prop 0.02
RANDOM_N = (240, 241)
NOISES = ((0.0, False), (1.0, True))
FIRST = 5                                                # first_index of the edge chunks


def _ctx(model="fixture"):
    from xna_basecaller_amd import _lib
    _lib.require_gpu()
    ctx = _lib.mapper_context(0)
    if model is not None:
        ctx.spike_model(*(cases.model() if model == "fixture" else cases.edge_model(model)))
    return ctx


def _same(got, want, what=""):
    assert np.array_equal(got[5], want[5]), (what, "status", np.flatnonzero(got[5] != want[5])[:5])
    assert np.array_equal(got[2], want[2]), (what, "spiked", np.flatnonzero(got[2] != want[2])[:5])
    for k, name in ((3, "med"), (4, "mad")):
        a, b = np.asarray(got[k], np.float64).view(np.uint64), np.asarray(want[k], np.float64).view(np.uint64)
        nan = np.isnan(got[k]) & np.isnan(want[k])
        assert np.array_equal(a[~nan], b[~nan]) and np.array_equal(np.isnan(got[k]), np.isnan(want[k])), \
            (what, name, np.flatnonzero(a != b)[:5], got[k][:3], want[k][:3])
    bad = np.flatnonzero((got[1] != want[1]).any(axis=1))
    assert bad.size == 0, (what, "targets", bad[:5])
    bad = np.flatnonzero((got[0].view(np.uint32) != np.asarray(want[0], np.float32).view(np.uint32)).any(axis=1))
    assert bad.size == 0, (what, "signal", bad[:5], [np.flatnonzero(got[0][b] != want[0][b])[:8] for b in bad[:2]])


@functools.lru_cache(maxsize=None)
def _random(N, std_dist, noise):
    data = cases.random_set(2000 + N, 64, N)
    kw = dict(ubs_mask=3, prop=0.02, var_prop=0.01, pad=5, **cases.dist_args(std_dist, *NOISES[noise]))
    stats = {}
    return data, kw, cases.reference(data, cases.model(), 0, SEED, kw, stats=stats), stats


@pytest.mark.parametrize("index", range(7))
def test_golden_cases_equal_the_restatement_and_the_reference(index):
    _, meta = cases.golden()
    case = meta["cases"][index]
    data = cases.dna()
    kw = cases.case_args(case)
    ctx = _ctx()
    got = ctx.spike_chunks(*data, 0, meta["seed"], **kw)
    _same(got, cases.reference(data, cases.model(), 0, meta["seed"], kw), case["name"])
    ref = cases.expected(case)                           # the reference's own labels, counts, med and mad
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2])
    assert np.array_equal(got[3].view(np.uint64), ref[3].view(np.uint64)) and np.array_equal(got[4].view(np.uint64), ref[4].view(np.uint64))
    if case["exact"]:
        assert np.array_equal(got[0].view(np.uint32), ref[0].view(np.uint32))
    ctx.close()


@pytest.mark.parametrize("noise", range(2))
@pytest.mark.parametrize("std_dist", cases.STD_DISTS)
@pytest.mark.parametrize("N", RANDOM_N)
def test_random_chunks_equal_the_restatement(N, std_dist, noise):
    data, kw, want, stats = _random(N, std_dist, noise)
    ctx = _ctx()
    _same(ctx.spike_chunks(*data, 0, SEED, **kw), want, (N, std_dist, noise))
    counts = [len(p) for p in stats["positions"]]
    assert want[2].sum() == sum(counts) and sum(c in (1, 2) for c in counts) > 32 and 0 in want[2] and not want[5].any()
    ctx.close()


def _edge(name):
    """(data, model, keyword arguments): the named edge chunks."""
    kw = dict(ubs_mask=3, prop=0.1, var_prop=0.0, pad=5, **cases.dist_args("truncnorm_shift_1.5_0.5", 1.0, True))
    if name == "length_20":                              # no valid base: unchanged, spiked 0 (med and mad still computed)
        chunks = [cases.one_chunk(s, L, 200, Lt=24) for s, L in ((1, 1), (2, 6), (3, 19), (4, 20))]
        return tuple(np.concatenate([c[k] for c in chunks]) for k in range(4)), "fixture", kw
    if name == "length_41":                              # 4100 squiggle values: no multiple of 64 or 256
        return cases.one_chunk(5, 41, 300), "fixture", kw
    if name == "bases_700":                              # 70000 values: counts past 2^16
        return cases.one_chunk(6, 700, 1500), "fixture", dict(kw, prop=0.01)
    if name in ("ties", "signs"):
        return cases.random_set(7, 8, 240), name, kw
    if name == "last_letter_a":                          # the TATAT tail
        return cases.one_chunk(8, 50, 300, last=1), "fixture", kw
    if name == "empty_bases":                            # a zero repetition at every position of chunk 0, an empty window in chunk 1
        data = cases.one_chunk(9, 60, 400)
        data = tuple(np.concatenate([a, a]) for a in data)
        stats = {}
        cases.reference(data, cases.model(), FIRST, SEED, kw, stats=stats)      # the positions do not depend on the breakpoints
        bk = data[3].copy()
        for pos in stats["positions"][0]:
            bk[0, pos - 3] = bk[0, pos - 4]
        pos = stats["positions"][1][0]
        bk[1, pos - 6:pos + 1] = bk[1, pos - 6]
        return data[:3] + (bk,), "fixture", kw
    if name == "pad2_missing_kmer":                      # a window that holds an existing UB: no such k-mer, status 2
        data = cases.random_set(10, 16, 240)
        data[1][:, 25] = np.where(data[2] > 40, 5, data[1][:, 25])
        return data, "fixture", dict(kw, pad=2, prop=0.3)
    raise KeyError(name)


EDGES = ("length_20", "length_41", "bases_700", "ties", "signs", "last_letter_a", "empty_bases", "pad2_missing_kmer")


@pytest.mark.parametrize("name", EDGES)
def test_edge_chunks(name):
    data, model, kw = _edge(name)
    mdl = cases.model() if model == "fixture" else cases.edge_model(model)
    stats = {}
    want = cases.reference(data, mdl, FIRST, SEED, kw, stats=stats)
    ctx = _ctx(model)
    got = ctx.spike_chunks(*data, FIRST, SEED, **kw)
    _same(got, want, name)
    if name == "length_20":
        assert not got[2].any() and not got[5].any() and np.array_equal(got[0], data[0]) and np.array_equal(got[1], data[1])
        assert (got[4] > 0).all()
    elif name == "empty_bases":
        assert stats["empty"] >= 6 + len(stats["positions"][0]) and (got[2] > 0).all()
    elif name == "pad2_missing_kmer":
        bad = got[5] == 2
        assert bad.any() and not bad.all() and not got[2][bad].any() and np.isnan(got[4][bad]).all()
        assert np.array_equal(got[0][bad], data[0][bad]) and np.array_equal(got[1][bad], data[1][bad])
        for t in got[3][bad]:                            # the k-mer named holds two unnatural bases
            assert sum(d > 4 for d in (int(t) // 7 ** q % 7 for q in range(6))) == 2
    elif name == "ties":
        assert (mdl[1][~np.isnan(mdl[0])] == 0).sum() > 1000 and (got[2] > 0).any()
    elif name == "signs":
        assert (got[3] < 20).all() and (mdl[0][~np.isnan(mdl[0])] < 0).any() and (mdl[0][~np.isnan(mdl[0])] > 0).any()
    elif name == "bases_700":
        assert got[2][0] >= 5
    else:
        assert got[2][0] >= 1
    ctx.close()


def test_host_and_dev_forms_agree():
    import torch
    data, kw, want, _ = _random(241, "truncnorm_shift_1.5_0.5", 1)
    ctx = _ctx()
    dev = torch.device("cuda:0")
    d_in = [torch.from_numpy(a).to(dev) for a in (data[0], data[1], data[2], data[3].view(np.int16))]
    n, N = data[0].shape
    Lt = data[1].shape[1]
    d_out = [torch.full((n, N), -7.0, dtype=torch.float32, device=dev), torch.full((n, Lt), 9, dtype=torch.uint8, device=dev),
             torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7.0, dtype=torch.float64, device=dev),
             torch.full((n,), -7.0, dtype=torch.float64, device=dev), torch.full((n,), -7, dtype=torch.int8, device=dev)]
    torch.cuda.synchronize()
    ctx.spike_chunks_dev(*(t.data_ptr() for t in d_in), n, N, Lt, 0, SEED, kw["ubs_mask"], kw["prop"], kw["var_prop"], kw["pad"],
                         kw["dist_rows"], kw["phi"], kw["noise_std"], kw["variable_noise"], *(t.data_ptr() for t in d_out))
    ctx.synchronize()
    _same([t.cpu().numpy() for t in d_out], want, "dev form")
    ctx.close()


def test_two_batch_splits_agree():
    """64 chunks in one call, then as 23 + 41 with first_index set: identical; another first_index gives other draws."""
    data, kw, want, _ = _random(240, "truncnorm", 1)
    ctx = _ctx()
    whole = ctx.spike_chunks(*data, 1000, SEED, **kw)
    parts = [ctx.spike_chunks(*(a[lo:hi] for a in data), 1000 + lo, SEED, **kw) for lo, hi in ((0, 23), (23, 64))]
    for k in range(6):
        assert np.array_equal(whole[k].view(np.uint8), np.concatenate([p[k] for p in parts]).view(np.uint8)), k
    assert not np.array_equal(whole[0], want[0])         # want was drawn at first_index 0
    ctx.close()


def test_limits_leave_the_context_usable():
    from xna_basecaller_amd import _lib
    _, meta = cases.golden()
    case = meta["cases"][1]
    data = cases.dna()
    good = cases.case_args(case)
    want = cases.reference(tuple(a[:3] for a in data), cases.model(), 0, meta["seed"], good)
    ctx = _ctx(None)
    with pytest.raises(_lib.XbError) as e:               # no model yet
        ctx.spike_chunks(*data, 0, 1, **good)
    assert e.value.code == _lib.XB_ERR_STATE
    mean, stdv = cases.model()
    neg = stdv.copy()
    neg[np.flatnonzero(~np.isnan(mean))[4]] = -1.0
    for m, s, word in ((mean[:-1], stdv[:-1], "117648 k-mers"), (mean, neg, "stdv -1"),
                       (np.where(np.isnan(mean), np.inf, mean), stdv, "mean inf")):
        with pytest.raises(_lib.XbError) as e:
            ctx.spike_model(m, s)
        assert e.value.code == _lib.XB_ERR_INVALID and word in str(e.value), str(e.value)
    with pytest.raises(_lib.XbError) as e:               # a refused model does not count as one
        ctx.spike_chunks(*data, 0, 1, **good)
    assert e.value.code == _lib.XB_ERR_STATE
    ctx.spike_model(mean, stdv)
    one = tuple(a[:1] for a in data)
    wide = np.zeros((1, 65536), np.float32)
    long_t, long_b = np.zeros((1, 65536), np.uint8), np.zeros((1, 65536), np.uint16)
    decreasing = data[3][:2].copy()
    decreasing[1, 4] = decreasing[1, 2]
    two = tuple(a[:2] for a in data)
    flat = good["phi"].copy()
    flat[1, 1] = 0.0
    full = good["phi"].copy()
    full[3] = (0.5, 0.5)
    for d, kw, word in (((wide,) + one[1:], {}, "65536 samples"),
                        ((one[0], long_t, one[2], long_b), {}, "65536 entries"),
                        (one, dict(pad=-1), "pad = -1"),
                        (one, dict(ubs_mask=-1), "ubs_mask = -1"),
                        (one, dict(ubs_mask=4), "ubs_mask = 4"),
                        (one, dict(prop=0.9, var_prop=0.2), "prop = 0.9"),
                        (one, dict(dist_rows=33, phi=np.full((34, 2), 0.25)), "dist_rows = 33"),
                        (one, dict(phi=flat), "distribution row 1"),
                        (one, dict(phi=full), "distribution row 3"),
                        (one, dict(noise_std=-0.5), "noise_std = -0.5"),
                        (two[:3] + (decreasing,), {}, "chunk 1"),
                        (two[:2] + (np.array([10, 65], np.int32), two[3]), {}, "chunk 1 has 65 labels")):
        with pytest.raises(_lib.XbError) as e:
            ctx.spike_chunks(*d, 0, meta["seed"], **dict(good, **kw))
        assert e.value.code == _lib.XB_ERR_INVALID and word in str(e.value), str(e.value)
        _same(ctx.spike_chunks(*(a[:3] for a in data), 0, meta["seed"], **good), want, "after " + word)
    ctx.close()


def test_spike_after_splice_keeps_and_avoids_the_spliced_bases():
    """The reference's mixed mode: `splice` on the splice fixture, then `spike` on its output."""
    _, meta = splice_cases.golden()
    case = meta["cases"][0]
    ctx = _ctx()
    lib = splice_cases.library(case["library"])
    ctx.splice_library(lib.pool, lib.rows, lib.table)
    chunks, targets, lengths, bkps = splice_cases.dna()
    spliced = ctx.splice_chunks(chunks, targets, lengths, bkps, 0, meta["seed"], **splice_cases.case_args(case))
    assert np.array_equal(spliced[1], splice_cases.expected(case)[1])
    data = (spliced[0], spliced[1], lengths, bkps)
    kw = dict(ubs_mask=3, prop=0.3, var_prop=0.0, pad=3, **cases.dist_args("truncnorm_shift_1.5_0.5", 1.0, True))
    stats = {}
    want = cases.reference(data, cases.model(), 0, SEED, kw, stats=stats)
    got = ctx.spike_chunks(*data, 0, SEED, **kw)
    _same(got, want, "spike after splice")
    ok = got[5] == 0
    assert ok.sum() >= 30 and got[2][ok].sum() > 10       # chunk 27's two adjacent unnatural bases share k-mers no model has
    keep = spliced[1] > 4
    assert np.array_equal(got[1][keep], spliced[1][keep])
    rows = iter(stats["positions"])
    for c in np.flatnonzero(ok):
        for pos in next(rows):
            assert all(abs(pos - ub) > 2 * kw["pad"] for ub in np.flatnonzero(keep[c]))
    ctx.close()


def test_cli_end_to_end(tmp_path):
    """A ctc-data directory and a model file -> `spike` -> a ctc-data directory that equals the reference's output of the
    recipe's default case (chunks as float16) and that evaluate's loader opens."""
    from xna_basecaller_amd import spike as sk
    from xna_basecaller_amd.data import load_validation
    _, meta = cases.golden()
    case = meta["cases"][1]
    dna = cases.write_dir(tmp_path)
    model = cases.write_model(str(tmp_path / "kmer.model"))
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "xna_basecaller_amd", "spike", dna, out, "-r", model, "--ubs", case["ubs"], "--prop-ubs",
           str(case["prop_ubs"]), "--ub-pad", str(case["pad"]), "--std-dist", case["std_dist"], "--noise-std", str(case["noise_std"]),
           "--variable-noise", "--seed", str(meta["seed"]), "--batchsize", "7"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    want = cases.expected(case)
    assert "%d positions spiked" % int(want[2].sum()) in r.stderr, r.stderr
    got = {f: np.load(os.path.join(out, f)) for f in sk.FILES}
    assert got["chunks.npy"].dtype == np.float16 and np.array_equal(got["chunks.npy"], want[0].astype(np.float16))
    assert got["references.npy"].dtype == np.uint8 and np.array_equal(got["references.npy"], want[1])
    assert np.array_equal(got["breakpoints.npy"], np.load(os.path.join(dna, "breakpoints.npy")))
    lines = open(os.path.join(out, "spike_stats.csv")).read().split()
    assert lines[0] == "index,spiked,med,mad" and [float(ln.split(",")[2]) for ln in lines[1:]] == [float(v) for v in want[3]]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--overwrite" in r.stderr
    chunks, targets, lengths = load_validation(None, out)
    assert chunks.shape[1] == want[0].shape[1] and len(lengths) == len(chunks) >= 1 and (targets > 4).any()
