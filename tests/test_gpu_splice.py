"""GPU: xb_splice_library / xb_splice_chunks through the C ABI and the `splice` CLI.  The device output EQUALS, bit for bit
(float32 viewed as uint32), what the reference's stitch_chunks.py computed on the golden fixture (tests/golden/splice.npz) and
what the restatement of the contract (tests/splice_ref.py) computes on seeded random chunks; no case excluded."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest

import splice_cases as cases
import splice_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

# chunks, samples, letters, then the parameters: every pad that changes the mask's reach (0: a base alone, 2: windows of
# neighbouring positions overlap, 5), one candidate, the default ten, 32 (more than a group holds), both UB sets, a drawn
# proportion; N = 64 and 1000 take the 16-byte row copy, 333 and 600 (label rows of N / 2 + 1) the scalar one
RANDOM_SETS = (
    (40, 64, False, dict(ubs_mask=3, prop=0.1, var_prop=0.0, cand_sample_size=10, pad=5)),
    (50, 333, False, dict(ubs_mask=1, prop=0.15, var_prop=0.1, cand_sample_size=1, pad=2)),
    (50, 600, True, dict(ubs_mask=3, prop=0.3, var_prop=0.05, cand_sample_size=32, pad=0)),
    (60, 1000, False, dict(ubs_mask=2, prop=0.08, var_prop=0.03, cand_sample_size=4, pad=5)),
)
SEED = 77


def _ctx(which="full"):
    from xna_basecaller_amd import _lib
    _lib.require_gpu()
    ctx = _lib.mapper_context(0)
    if which is not None:
        lib = cases.library(which)
        ctx.splice_library(lib.pool, lib.rows, lib.table)
    return ctx


@functools.lru_cache(maxsize=None)
def _reference(index, first_index=0):
    n, N, four, kw = RANDOM_SETS[index]
    data = cases.random_set(1000 + index, n, N, four)
    stats = {}
    ubs = [u for u in (5, 6) if kw["ubs_mask"] >> (u - 5) & 1]
    out = [splice_ref.splice_chunk(data[0][c], data[1][c], data[2][c], data[3][c], cases.library("full"), first_index + c, SEED, ubs,
                                   kw["prop"], kw["var_prop"], kw["cand_sample_size"], kw["pad"], stats=stats) for c in range(n)]
    return data, [np.array([o[k] for o in out]) for k in range(4)], stats


def _same(got, want, what=""):
    assert np.array_equal(got[2].astype(bool), np.asarray(want[2]).astype(bool)), (what, np.flatnonzero(got[2] != want[2])[:5])
    assert np.array_equal(got[3], want[3]), (what, np.flatnonzero(got[3] != want[3])[:5])
    bad = np.flatnonzero((got[1] != want[1]).any(axis=1))
    assert bad.size == 0, (what, bad[:5])
    bad = np.flatnonzero((got[0].view(np.uint32) != np.asarray(want[0], np.float32).view(np.uint32)).any(axis=1))
    assert bad.size == 0, (what, bad[:5], [np.flatnonzero(got[0][b] != want[0][b])[:8] for b in bad[:2]])


@pytest.mark.parametrize("index", range(4))
def test_golden_cases_equal_the_reference(index):
    _, meta = cases.golden()
    case = meta["cases"][index]
    ctx = _ctx(case["library"])
    chunks, targets, lengths, bkps = cases.dna()
    got = ctx.splice_chunks(chunks, targets, lengths, bkps, 0, meta["seed"], **cases.case_args(case))
    want = cases.expected(case)
    _same(got, want + ((want[1] != targets).sum(axis=1),), case["name"])
    assert got[2].sum() == case["succeeded"] and got[3].sum() == case["inserted"]
    ctx.close()


@pytest.mark.parametrize("index", range(len(RANDOM_SETS)))
def test_random_chunks_equal_the_restatement(index):
    data, want, stats = _reference(index)
    ctx = _ctx()
    got = ctx.splice_chunks(*data, 0, SEED, **RANDOM_SETS[index][3])
    _same(got, want, RANDOM_SETS[index][:3])
    assert stats["stretch"] + stats["shrink"] + stats["copy"] == want[3].sum() > 0
    if RANDOM_SETS[index][2]:
        assert stats["abandoned"] > 0                    # four letters against a two-letter library
    else:
        assert stats["stretch"] > 0 and stats["shrink"] > 0
    ctx.close()


def test_random_sets_cover_two_hundred_chunks():
    assert sum(s[0] for s in RANDOM_SETS) == 200 and min(s[1] for s in RANDOM_SETS) == 64 and max(s[1] for s in RANDOM_SETS) == 1000


def test_a_batch_equals_its_chunks_one_per_call():
    """64 chunks in one call, then each alone with first_index set: identical; another first_index gives other draws."""
    ctx = _ctx()
    kw = dict(ubs_mask=3, prop=0.1, var_prop=0.05, cand_sample_size=10, pad=5)
    data = cases.random_set(5, 64, 600)
    whole = ctx.splice_chunks(*data, 1000, SEED, **kw)
    for c in range(64):
        one = ctx.splice_chunks(*(a[c:c + 1] for a in data), 1000 + c, SEED, **kw)
        for a, b in zip(whole, one):
            assert np.array_equal(a[c:c + 1].view(np.uint8), b.view(np.uint8)), c
    moved = ctx.splice_chunks(*data, 1001, SEED, **kw)
    assert not np.array_equal(whole[1], moved[1])
    ctx.close()


def test_a_second_library_replaces_the_first():
    _, meta = cases.golden()
    full, holes = meta["cases"][0], meta["cases"][3]
    chunks, targets, lengths, bkps = cases.dna()
    ctx = _ctx("full")
    args = cases.case_args(holes)
    with_full = ctx.splice_chunks(chunks, targets, lengths, bkps, 0, meta["seed"], **args)
    lib = cases.library("holes")
    ctx.splice_library(lib.pool, lib.rows, lib.table)
    want = cases.expected(holes)
    got = ctx.splice_chunks(chunks, targets, lengths, bkps, 0, meta["seed"], **args)
    _same(got, want + ((want[1] != targets).sum(axis=1),), "holes after full")
    assert with_full[3].sum() > got[3].sum()                     # the full library abandons nothing
    lib = cases.library("full")
    ctx.splice_library(lib.pool, lib.rows, lib.table)
    want = cases.expected(full)
    _same(ctx.splice_chunks(chunks, targets, lengths, bkps, 0, meta["seed"], **cases.case_args(full)),
          want + ((want[1] != targets).sum(axis=1),), "full again")
    ctx.close()


def test_host_and_dev_forms_agree():
    import torch
    data, want, _ = _reference(3)
    kw = RANDOM_SETS[3][3]
    ctx = _ctx()
    dev = torch.device("cuda:0")
    d_in = [torch.from_numpy(a).to(dev) for a in (data[0], data[1], data[2], data[3].view(np.int16))]
    n, N = data[0].shape
    Lt = data[1].shape[1]
    d_out = [torch.full((n, N), -7.0, dtype=torch.float32, device=dev), torch.full((n, Lt), 9, dtype=torch.uint8, device=dev),
             torch.full((n,), -7, dtype=torch.int8, device=dev), torch.full((n,), -7, dtype=torch.int32, device=dev)]
    torch.cuda.synchronize()
    ctx.splice_chunks_dev(*(t.data_ptr() for t in d_in), n, N, Lt, 0, SEED, kw["ubs_mask"], kw["prop"], kw["var_prop"],
                          kw["cand_sample_size"], kw["pad"], *(t.data_ptr() for t in d_out))
    ctx.synchronize()
    _same([t.cpu().numpy() for t in d_out], want, "dev form")
    ctx.close()


def test_limits_leave_the_context_usable():
    from xna_basecaller_amd import _lib
    _, meta = cases.golden()
    case = meta["cases"][0]
    chunks, targets, lengths, bkps = cases.dna()
    ctx = _ctx(None)
    good = cases.case_args(case)
    with pytest.raises(_lib.XbError) as e:                       # no library yet
        ctx.splice_chunks(chunks, targets, lengths, bkps, 0, 1, **good)
    assert e.value.code == _lib.XB_ERR_STATE
    lib = cases.library("full")
    rows = lib.rows.copy()
    rows[5, 1] = 101
    for pool, r, table, word in ((lib.pool, rows, lib.table, "101 samples"), (lib.pool, lib.rows, lib.table[:-1], "groups"),
                                 (lib.pool[:10], lib.rows, lib.table, "pool of 10")):
        with pytest.raises(_lib.XbError) as e:
            ctx.splice_library(pool, r, table)
        assert e.value.code == _lib.XB_ERR_INVALID and word in str(e.value), str(e.value)
    ctx.splice_library(lib.pool, lib.rows, lib.table)
    wide = np.zeros((1, 65536), np.float32)
    long_t, long_b = np.zeros((1, 65536), np.uint8), np.zeros((1, 65536), np.uint16)
    one = (chunks[:1], targets[:1], lengths[:1], bkps[:1])
    decreasing = bkps[:2].copy()
    decreasing[1, 4] = decreasing[1, 2]
    for data, kw, word in (((wide,) + one[1:], {}, "65536 samples"),
                           ((one[0], long_t, one[2], long_b), {}, "65536 entries"),
                           (one, dict(cand_sample_size=0), "cand_sample_size = 0"),
                           (one, dict(cand_sample_size=33), "cand_sample_size = 33"),
                           (one, dict(pad=-1), "pad = -1"),
                           (one, dict(ubs_mask=0), "ubs_mask = 0"),
                           (one, dict(ubs_mask=4), "ubs_mask = 4"),
                           (one, dict(prop=0.9, var_prop=0.2), "prop = 0.9"),
                           ((chunks[:2], targets[:2], lengths[:2], decreasing), {}, "chunk 1"),
                           ((chunks[:2], targets[:2], np.array([10, 81], np.int32), bkps[:2]), {}, "chunk 1 has 81 labels")):
        with pytest.raises(_lib.XbError) as e:
            ctx.splice_chunks(*data, 0, meta["seed"], **dict(good, **kw))
        assert e.value.code == _lib.XB_ERR_INVALID and word in str(e.value), str(e.value)
        want = cases.expected(case)
        got = ctx.splice_chunks(chunks[:3], targets[:3], lengths[:3], bkps[:3], 0, meta["seed"], **good)
        _same(got, tuple(w[:3] for w in want) + ((want[1][:3] != targets[:3]).sum(axis=1),), "after " + word)
    ctx.close()


def test_cli_end_to_end(tmp_path):
    """DNA and XNA ctc-data directories -> `splice` -> a ctc-data directory that equals the reference's output of the same
    case (chunks as float16) and that evaluate's loader opens."""
    from xna_basecaller_amd import splice as sp
    from xna_basecaller_amd.data import load_validation
    _, meta = cases.golden()
    case = meta["cases"][1]
    dna, xna = cases.write_dirs(tmp_path)
    out = str(tmp_path / "out")
    cmd = [sys.executable, "-m", "xna_basecaller_amd", "splice", dna, xna, out, "--ubs", case["ubs"], "--prop-ubs", str(case["prop_ubs"]),
           "--var-prop-ubs", str(case["var_prop_ubs"]), "--cand-sample-size", str(case["cand_sample_size"]), "--ub-pad", str(case["pad"]),
           "--seed", str(meta["seed"]), "--batchsize", "7"]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr
    want = cases.expected(case)
    assert "%d chunks kept unchanged" % int((~want[2]).sum()) in r.stderr, r.stderr
    got = {f: np.load(os.path.join(out, f)) for f in sp.FILES}
    assert got["chunks.npy"].dtype == np.float16 and np.array_equal(got["chunks.npy"], want[0].astype(np.float16))
    assert got["references.npy"].dtype == np.uint8 and np.array_equal(got["references.npy"], want[1])
    assert np.array_equal(got["breakpoints.npy"], np.load(os.path.join(dna, "breakpoints.npy")))
    lines = open(os.path.join(out, "splice_stats.csv")).read().split()
    assert lines[0] == "index,success,inserted" and len(lines) == 1 + len(want[2])
    assert [int(ln.split(",")[1]) for ln in lines[1:]] == [int(v) for v in want[2]]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "--overwrite" in r.stderr
    chunks, targets, lengths = load_validation(None, out)
    assert chunks.shape[1] == want[0].shape[1] and targets.shape[1] == want[1].shape[1] and len(lengths) == len(chunks) >= 1
    assert (targets > 4).any()
