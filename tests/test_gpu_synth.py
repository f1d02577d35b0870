"""GPU: xb_synth_chunks through the C ABI and the `synth` CLI.  The device output EQUALS, bit for bit, what the restatement of
the contract (tests/synth_ref.py) computes -- out_signal (float32 viewed as uint32), out_targets, spiked, status and the bit
patterns of med and mad -- on the golden fixture's cases (where it also equals the reference's own arrays,
tests/golden/synth.npz), on seeded random chunks in every level distribution and on the named edge chunks."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import spike_cases
import splice_cases
import synth_cases as cases
from conftest import ROOT
from synth_cases import same as _same

pytestmark = pytest.mark.gpu

SEED = 77
# 64 chunks each: N = 240 takes the 16-byte row copy, 241 the scalar one; lengths run from 12 (no position) to 120; 21 and 16
# of the chunks end short of N (spike_cases.random_set draws the last breakpoint of every other chunk), so their tails keep the
# input
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


@functools.lru_cache(maxsize=None)
def _random(N, std_dist, noise):
    data = cases.random_set(2000 + N, 64, N)
    kw = dict(ubs_mask=3, prop=0.02, var_prop=0.01, pad=5, **cases.dist_args(std_dist, *NOISES[noise]))
    stats = {}
    want = cases.reference(data, cases.model(), 0, SEED, kw, stats=stats)
    for a in data + want:
        a.setflags(write=False)
    return data, kw, want, stats


@pytest.mark.parametrize("index", range(7))
def test_golden_cases_equal_the_restatement_and_the_reference(index):
    _, meta = cases.golden()
    case = meta["cases"][index]
    data = cases.dna()
    ctx = _ctx()
    got = ctx.synth_chunks(*data, 0, meta["seed"], **cases.case_args(case))
    ctx.close()
    _same(got, cases.golden_reference(index)[0], case["name"])
    ref = cases.expected(case)                           # the reference's own arrays; where it raised: status 2, the input
    bad = cases.raised(case)
    ok = ref[5] == 0
    assert np.array_equal(got[1], ref[1]) and np.array_equal(got[2], ref[2]) and np.array_equal(got[5], ref[5])
    assert np.array_equal(got[3][ok].view(np.uint64), ref[3][ok].view(np.uint64))
    assert np.array_equal(got[4][ok].view(np.uint64), ref[4][ok].view(np.uint64))
    from xna_basecaller_amd import spike as sk
    assert {c: sk.index_kmer(got[3][c]) for c in bad} == bad and np.isnan(got[4][~ok]).all()
    steps = np.abs(got[0].view(np.int32).astype(np.int64) - ref[0].view(np.int32).astype(np.int64))
    print("%s: %d of %d values differ from the reference's, the largest by %d float32 steps"
          % (case["name"], (steps > 0).sum(), case["values_synthesised"], steps.max()))
    assert steps.max() <= (0 if case["exact"] else 1) and (steps > 0).sum() == case["values_differing_from_restatement"]


@pytest.mark.parametrize("noise", range(2))
@pytest.mark.parametrize("std_dist", cases.STD_DISTS)
@pytest.mark.parametrize("N", RANDOM_N)
def test_random_chunks_equal_the_restatement(N, std_dist, noise):
    data, kw, want, stats = _random(N, std_dist, noise)
    ctx = _ctx()
    got = ctx.synth_chunks(*data, 0, SEED, **kw)
    ctx.close()
    _same(got, want, (N, std_dist, noise))
    total = np.minimum(data[3][np.arange(64), data[2] - 1], N)
    assert (total < N).sum() >= 16 and (total == N).sum() >= 16 and 0 in want[2] and not want[5].any()
    for c in np.flatnonzero(total < N)[:8]:              # the kept tail, and nothing kept before it
        assert np.array_equal(got[0][c, total[c]:], data[0][c, total[c]:]) and (got[0][c, :total[c]] != data[0][c, :total[c]]).all()
    assert stats["total"] == int(total.sum())


def _edge(name):
    """(data, model, keyword arguments): the named edge chunks."""
    kw = dict(ubs_mask=3, prop=0.1, var_prop=0.0, pad=5, **cases.dist_args("truncnorm_shift_1.5_0.5", 1.0, True))
    if name == "length_20":                              # no valid base, yet synthesised: spiked 0, output != input
        chunks = [cases.one_chunk(s, L, 200, Lt=24) for s, L in ((1, 1), (2, 6), (3, 19), (4, 20))]
        return tuple(np.concatenate([c[k] for c in chunks]) for k in range(4)), "fixture", kw
    if name == "length_41":                              # 4100 squiggle values: no multiple of 64 or 256
        return cases.one_chunk(5, 41, 300), "fixture", kw
    if name == "bases_700":                              # 70000 values: counts past 2^16; 24 passes of lanes over the samples
        return cases.one_chunk(6, 700, 1500), "fixture", dict(kw, prop=0.01)
    if name in ("ties", "signs"):
        return cases.random_set(7, 8, 240), name, kw
    if name == "last_letter_a":                          # the TATAT tail
        return cases.one_chunk(8, 50, 300, last=1), "fixture", kw
    if name == "empty_bases":                            # chunk 0: an empty first base and a run of six; chunk 1: every other base
        data = cases.one_chunk(9, 60, 400)
        data = tuple(np.concatenate([a, a]) for a in data)
        bk = data[3].copy()
        bk[0, 0] = 0
        bk[0, 20:26] = bk[0, 19]
        bk[1, 1:59:2] = bk[1, 0:58:2]
        return data[:3] + (bk,), "fixture", kw
    if name == "pad2_missing_kmer":                      # a new UB five bases from an existing one, or two new ones three apart
        data = cases.random_set(10, 16, 240)
        data[1][:, 25] = np.where(data[2] > 40, 5, data[1][:, 25])
        return data, "fixture", dict(kw, pad=2, prop=0.3)
    if name == "ubs_mask_0":                             # the DNA as it is, re-synthesised
        return cases.random_set(11, 8, 241), "fixture", dict(kw, ubs_mask=0)
    raise KeyError(name)


EDGES = ("length_20", "length_41", "bases_700", "ties", "signs", "last_letter_a", "empty_bases", "pad2_missing_kmer", "ubs_mask_0")


@pytest.mark.parametrize("name", EDGES)
def test_edge_chunks(name):
    data, model, kw = _edge(name)
    mdl = cases.model() if model == "fixture" else cases.edge_model(model)
    stats = {}
    want = cases.reference(data, mdl, FIRST, SEED, kw, stats=stats)
    ctx = _ctx(model)
    got = ctx.synth_chunks(*data, FIRST, SEED, **kw)
    ctx.close()
    _same(got, want, name)
    if name == "length_20":
        assert not got[2].any() and not got[5].any() and np.array_equal(got[1], data[1]) and (got[0] != data[0]).all()
        assert (got[4] > 0).all()
    elif name == "empty_bases":
        assert stats["empty"] == 7 + 29 and (got[2] > 0).all() and (got[0] != data[0]).all()
    elif name == "pad2_missing_kmer":
        bad = got[5] == 2
        assert bad.any() and not got[2][bad].any() and np.isnan(got[4][bad]).all()
        assert np.array_equal(got[0][bad], data[0][bad]) and np.array_equal(got[1][bad], data[1][bad])
        for t in got[3][bad]:                            # the k-mer named holds two unnatural bases
            assert sum(d > 4 for d in (int(t) // 7 ** q % 7 for q in range(6))) == 2
    elif name == "ubs_mask_0":
        assert np.array_equal(got[1], data[1]) and (got[2] > 0).any() and not got[5].any()
    elif name == "ties":
        assert (mdl[1][~np.isnan(mdl[0])] == 0).sum() > 1000 and (got[2] > 0).any()
    elif name == "signs":
        assert (got[3] < 20).all() and (mdl[0][~np.isnan(mdl[0])] < 0).any() and (mdl[0][~np.isnan(mdl[0])] > 0).any()
    elif name == "bases_700":
        assert got[2][0] >= 5 and (got[0] != data[0]).all()
    else:
        assert got[2][0] >= 1


def test_host_and_dev_forms_agree():
    import torch
    data, kw, want, _ = _random(241, "truncnorm_shift_1.5_0.5", 1)
    ctx = _ctx()
    dev = torch.device("cuda:0")
    d_in = [torch.from_numpy(np.array(a)).to(dev) for a in (data[0], data[1], data[2], data[3].view(np.int16))]
    n, N = data[0].shape
    Lt = data[1].shape[1]
    d_out = [torch.full((n, N), -7.0, dtype=torch.float32, device=dev), torch.full((n, Lt), 9, dtype=torch.uint8, device=dev),
             torch.full((n,), -7, dtype=torch.int32, device=dev), torch.full((n,), -7.0, dtype=torch.float64, device=dev),
             torch.full((n,), -7.0, dtype=torch.float64, device=dev), torch.full((n,), -7, dtype=torch.int8, device=dev)]
    torch.cuda.synchronize()
    ctx.synth_chunks_dev(*(t.data_ptr() for t in d_in), n, N, Lt, 0, SEED, kw["ubs_mask"], kw["prop"], kw["var_prop"], kw["pad"],
                         kw["dist_rows"], kw["phi"], kw["noise_std"], kw["variable_noise"], *(t.data_ptr() for t in d_out))
    ctx.synchronize()
    _same([t.cpu().numpy() for t in d_out], want, "dev form")
    ctx.close()


def test_two_batch_splits_agree():
    """64 chunks in one call, then as 23 + 41 with first_index set: identical; another first_index gives other draws."""
    data, kw, want, _ = _random(240, "truncnorm", 1)
    ctx = _ctx()
    whole = ctx.synth_chunks(*data, 1000, SEED, **kw)
    parts = [ctx.synth_chunks(*(a[lo:hi] for a in data), 1000 + lo, SEED, **kw) for lo, hi in ((0, 23), (23, 64))]
    ctx.close()
    for k in range(6):
        assert np.array_equal(whole[k].view(np.uint8), np.concatenate([p[k] for p in parts]).view(np.uint8)), k
    assert not np.array_equal(whole[0], want[0])         # want was drawn at first_index 0


def test_limits_leave_the_context_usable():
    from xna_basecaller_amd import _lib
    _, meta = cases.golden()
    case = meta["cases"][1]
    data = cases.dna()
    good = cases.case_args(case)
    want = tuple(a[:3] for a in cases.golden_reference(1)[0])
    ctx = _ctx(None)
    with pytest.raises(_lib.XbError) as e:               # no model yet
        ctx.synth_chunks(*data, 0, 1, **good)
    assert e.value.code == _lib.XB_ERR_STATE and "xb_synth_chunks" in str(e.value) and "xb_spike_model" in str(e.value)
    mean, stdv = cases.model()
    with pytest.raises(_lib.XbError):                    # a refused model does not count as one
        ctx.spike_model(mean[:-1], stdv[:-1])
    with pytest.raises(_lib.XbError) as e:
        ctx.synth_chunks(*data, 0, 1, **good)
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
            ctx.synth_chunks(*d, 0, meta["seed"], **dict(good, **kw))
        assert e.value.code == _lib.XB_ERR_INVALID and word in str(e.value) and "xb_synth_chunks:" in str(e.value), str(e.value)
        _same(ctx.synth_chunks(*(a[:3] for a in data), 0, meta["seed"], **good), want, "after " + word)
    with pytest.raises(_lib.XbError) as e:               # first_index is checked by the C ABI too
        ctx.synth_chunks(*one, -1, meta["seed"], **good)
    assert "first_index = -1" in str(e.value)
    ctx.close()


def test_synth_of_spliced_chunks_keeps_and_avoids_the_spliced_bases():
    """The reference's mixed mode: the splice fixture's output (the reference's own) as the input."""
    _, meta = splice_cases.golden()
    case = meta["cases"][0]
    _, _, lengths, bkps = splice_cases.dna()
    spliced = splice_cases.expected(case)
    data = (spliced[0], spliced[1], lengths, bkps)
    kw = dict(ubs_mask=3, prop=0.3, var_prop=0.0, pad=3, **cases.dist_args("truncnorm_shift_1.5_0.5", 1.0, True))
    stats = {}
    want = cases.reference(data, cases.model(), 0, SEED, kw, stats=stats)
    ctx = _ctx()
    got = ctx.synth_chunks(*data, 0, SEED, **kw)
    ctx.close()
    _same(got, want, "synth after splice")
    ok = got[5] == 0
    keep = spliced[1] > 4
    # three to six spliced bases a chunk leave few free ones; chunk 27's two adjacent unnatural bases share k-mers no model
    # has, and so do two new bases four apart
    assert keep.any(axis=1).sum() >= 30 and ok.sum() >= 30 and not ok.all() and got[2][ok].sum() >= 5
    assert np.array_equal(got[1][keep], spliced[1][keep])
    for c, row in enumerate(stats["positions"]):
        for pos in row:
            assert all(abs(pos - ub) > 2 * kw["pad"] for ub in np.flatnonzero(keep[c]))


def test_spike_is_unchanged_beside_synth():
    """The model table is shared: the same inputs and seed through xb_spike_chunks give spike_ref's result before and after
    an xb_synth_chunks call on the same context."""
    data = cases.random_set(2240, 64, 240)
    kw = dict(ubs_mask=3, prop=0.02, var_prop=0.01, pad=5, **cases.dist_args("truncnorm_shift_1.5_0.5", 1.0, True))
    want = spike_cases.reference(data, cases.model(), 0, SEED, kw)
    ctx = _ctx()
    _same(ctx.spike_chunks(*data, 0, SEED, **kw), want, "spike before")
    whole = ctx.synth_chunks(*data, 0, SEED, **kw)
    _same(ctx.spike_chunks(*data, 0, SEED, **kw), want, "spike after")
    ctx.close()
    assert np.array_equal(whole[1], want[1]) and np.array_equal(whole[2], want[2])      # the same positions and UBs
    assert not np.array_equal(whole[0], want[0])


def test_cli_end_to_end(tmp_path):
    """A ctc-data directory and a model file -> `synth` -> a ctc-data directory that equals the reference's output of the
    recipe's case (chunks as float16) and that evaluate's loader opens."""
    from xna_basecaller_amd import spike as sk
    from xna_basecaller_amd.data import load_validation
    _, meta = cases.golden()
    case = meta["cases"][1]
    dna = cases.write_dir(tmp_path)
    model = cases.write_model(str(tmp_path / "kmer.model"))
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "xna_basecaller_amd", "synth", dna, out, "-r", model, "--ubs", case["ubs"], "--prop-ubs",
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
    lines = open(os.path.join(out, "synth_stats.csv")).read().split()
    assert lines[0] == "index,spiked,med,mad" and [float(ln.split(",")[2]) for ln in lines[1:]] == [float(v) for v in want[3]]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--overwrite" in r.stderr
    chunks, targets, lengths = load_validation(None, out)
    assert chunks.shape[1] == want[0].shape[1] and len(lengths) == len(chunks) >= 1 and (targets > 4).any()
