"""CPU: the host side of `segment` -- the specification tests/dtw_ref.py against exhaustive enumeration, the structure of
its results, reference_levels / load_kmer_poremodel against what the reference computed (tests/golden/dtwseg.json, written by
tests/golden/make_dtwseg_golden.py), and the CLI plumbing that needs no device."""
import itertools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import dtw_cases
import dtw_ref
from conftest import GOLDEN, ROOT
from xna_basecaller_amd import segment as seg


def _paths(N, M):
    """Every monotone assignment of N samples to M columns (each sample one column, no column skipped): the rows at which
    the column advances."""
    return itertools.combinations(range(1, N), M - 1)


def _columns(N, inc):
    cols, j = [], 0
    for i in range(N):
        j += i in inc
        cols.append(j)
    return cols


def test_dtw_ref_finds_the_optimal_cost_of_every_tiny_problem():
    rng = np.random.default_rng(0)
    for _ in range(60):
        N = int(rng.integers(1, 11))
        rep = int(rng.integers(1, 4))
        K = int(rng.integers(1, N // rep + 1)) if N >= rep else 1
        q, lev = dtw_cases.problem(rng, N, K)
        bp, ok, cost, _ = dtw_ref.dtw(q, lev, rep)
        r = np.repeat(lev, rep)
        if len(r) > N:
            assert not ok
            continue
        best = min(sum(abs(float(q[i]) - r[c]) for i, c in enumerate(_columns(N, inc))) for inc in _paths(N, len(r)))
        assert ok and abs(cost - best) <= 1e-12 * max(1.0, best)
        assert bp[-1] == N and (np.diff(np.concatenate(([0], bp))) >= rep).all()


def test_ties_take_the_stay_step():
    """Costs built to tie: among the optimal paths the stay-first rule, applied from the end backwards, picks the one that
    leaves each column as EARLY as the optimum allows on the way back -- i.e. at every tied cell the trace stays."""
    # all-zero costs: every path is optimal; at every cell both predecessors tie, the trace stays while it can, so the
    # advances all happen in the first rows
    bp, ok, cost, ties = dtw_ref.dtw(np.zeros(8, np.float32), np.zeros(3), 1)
    assert ok and cost == 0.0 and ties > 0 and bp.tolist() == [1, 2, 8]
    bp, ok, _, _ = dtw_ref.dtw(np.zeros(9, np.float32), np.zeros(2), 2)
    assert bp.tolist() == [2, 9]                               # columns 0 0 | 1 1: rows 0, 1, 2 advance, base 1 keeps the rest
    # enumeration: the traced path is optimal, and of all optimal paths it is the one the rule gives
    rng = np.random.default_rng(4)
    for _ in range(40):
        N, M = int(rng.integers(2, 10)), 0
        M = int(rng.integers(1, N + 1))
        q = rng.integers(0, 3, N).astype(np.float32)
        lev = rng.integers(0, 3, M).astype(np.float64)
        bp, ok, cost, _ = dtw_ref.dtw(q, lev, 1)
        costs = {inc: sum(abs(float(q[i]) - lev[c]) for i, c in enumerate(_columns(N, inc))) for inc in _paths(N, M)}
        best = min(costs.values())
        assert ok and cost == best                             # small integers: exact
        # the rule, restated independently on the set of optimal paths: walking back from the last row, prefer to stay
        optimal = [_columns(N, inc) for inc, c in costs.items() if c == best]
        i, j = N - 1, M - 1
        while i > 0:
            stay = [p for p in optimal if p[i - 1] == j]
            # staying is allowed when the prefix costs tie or staying is cheaper; among optimal paths through (i, j) the
            # prefix costs are equal, so "some optimal path stays" is exactly "the stay predecessor is not worse"
            optimal = stay if stay else [p for p in optimal if p[i - 1] == j - 1]
            j = optimal[0][i - 1]
            i -= 1
        reps = np.bincount(optimal[0], minlength=M)
        assert np.array_equal(bp, np.cumsum(reps))


def _in_order(d):
    """The contract's one addition per cell, row after row (np.sum adds pairwise)."""
    acc = float(d[0])
    for v in d[1:]:
        acc = float(v) + acc
    return acc


def test_structure():
    rng = np.random.default_rng(1)
    q, lev = dtw_cases.problem(rng, 12, 12)
    bp, ok, cost, _ = dtw_ref.dtw(q, lev, 1)                   # M = N: the diagonal
    assert ok and bp.tolist() == list(range(1, 13)) and cost == _in_order(np.abs(q.astype(np.float64) - lev))
    bp, ok, _, _ = dtw_ref.dtw(q, lev[:4], 3)                  # M = N through the repeat
    assert ok and bp.tolist() == [3, 6, 9, 12]
    bp, ok, cost, _ = dtw_ref.dtw(q, lev[:1], 1)               # M = 1
    assert ok and bp.tolist() == [12] and cost == _in_order(np.abs(q.astype(np.float64) - lev[0]))
    bp, ok, cost, _ = dtw_ref.dtw(q, lev[:5], 3)               # M > N fails: the naive split
    assert not ok and np.isinf(cost) and bp.tolist() == [3, 6, 8, 10, 12]
    q, lev = dtw_cases.problem(rng, 200, 40)
    free = dtw_ref.dtw(q, lev, 3)
    wide = dtw_ref.dtw(q, lev, 3, window=1000.0)               # a window wide enough equals no window
    assert free[1] and np.array_equal(free[0], wide[0]) and free[2] == wide[2]
    bp, ok, cost, _ = dtw_ref.dtw(q, lev, 3, window=0.0)       # too narrow: |j - i M / N| <= 0 holds on no connected path
    assert not ok and np.array_equal(bp, dtw_ref.naive_breakpoints(200, 40))
    some = dtw_ref.dtw(q, lev, 3, window=(200 / 40) * 2.0)
    assert some[1] and some[2] >= free[2]
    # the batch form: zero-filled rows, a failed chunk between two good ones
    bp, ok, cost, _ = dtw_ref.dtw_batch(np.stack([q, q, q]), [lev, np.zeros(80), lev[:7]], 3, kmax=90)
    assert ok.tolist() == [True, False, True] and (bp[0, 40:] == 0).all() and np.array_equal(bp[0, :40], free[0])


def _golden():
    with open(os.path.join(GOLDEN, "dtwseg.json")) as fh:
        return json.load(fh)


def _write_model(path, rows):
    with open(path, "w") as fh:
        fh.write("#model_name\tfixture\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\tweight\n")
        for kmer, mean, stdv in rows:
            fh.write("%s\t%r\t%r\t0.0\t0.0\t0.0\n" % (kmer, mean, stdv))
            fh.write("# a comment between rows\n")


def test_poremodel_and_levels_match_the_reference(tmp_path):
    g = _golden()
    path = str(tmp_path / "rows.model")
    _write_model(path, g["poremodel_rows"])
    model = seg.load_kmer_poremodel(path)
    assert model == {k: (m, s) for k, m, s in g["poremodel_rows"]}                       # to the last bit
    rng = np.random.RandomState(g["seed"])                      # one generator, the cases in file order
    for c in g["cases"]:
        means, stdvs = seg.kmer_levels(seg.target_string(c["target"], c["length"], c["ubs_map"]), model, c["k"], c["name"])
        assert means == c["means"] and stdvs == c["stdvs"], c["name"]
        levels = seg.reference_levels(np.array(c["target"]), c["length"], model, ubs_map=c["ubs_map"], k=c["k"], rng=rng)
        assert levels.dtype == np.float64 and len(levels) == len(c["levels"])
        if g["levels_equal"]:                                   # the generator confirmed the streams agree: equal as float64
            assert levels.tolist() == c["levels"], c["name"]
        else:
            assert np.max(np.abs(levels - np.array(c["levels"]))) <= g["levels_max_abs_diff"], c["name"]
    assert g["levels_equal"]
    short = [c for c in g["cases"] if c["name"] == "shorter_than_k"][0]
    assert short["means"] == [seg.SHORT_MEAN] * 7 and short["stdvs"] == [seg.SHORT_STDV] * 7
    with pytest.raises(ValueError) as e:                        # a k-mer the model lacks: named, with its chunk
        seg.reference_levels(np.array([5, 5, 6, 1, 2, 3, 4, 1]), 8, model, rng=np.random.RandomState(0), chunk=17)
    assert "chunk 17" in str(e.value) and "XXYACG" in str(e.value)
    with pytest.raises(ValueError):
        seg.reference_levels(np.array([1, 2]), 2, model, rng=None)


def test_naive_breakpoints_match_the_reference():
    nv = _golden()["naive"]
    lengths = np.array(nv["lengths"], np.uint16)
    targets = np.zeros((len(lengths), nv["width"]), np.uint8)
    bkps, ok = seg.naive_segment(nv["chunksize"], targets, lengths)
    assert str(bkps.dtype) == nv["dtype"] == "uint16" and bkps.tolist() == nv["breakpoints"] and ok.all()
    for n, row in zip(lengths, bkps):
        assert np.array_equal(row[:n], dtw_ref.naive_breakpoints(nv["chunksize"], int(n)))


def test_segment_does_not_depend_on_workers_or_batches(tmp_path):
    """The random draws stay on one generator in file order whatever runs the medians; the levels are built one batch ahead
    of the aligner."""
    poremodel = seg.load_kmer_poremodel(dtw_cases.write_poremodel(str(tmp_path / "synthetic.model")))
    ctc = str(tmp_path / "ctc")
    planted = dtw_cases.write_ctc_dir(ctc, poremodel)
    chunks, targets, lengths = (np.load(os.path.join(ctc, f)) for f in ("chunks.npy", "references.npy", "reference_lengths.npy"))
    seen = []

    def spy(signal, levels, ref_rep, window, kmax):
        seen.append([v.copy() for v in levels])
        return dtw_ref.device_stand_in(signal, levels, ref_rep, window, kmax)
    timings = {}
    a, ok = seg.segment(chunks, targets, lengths, poremodel, dtw=spy, workers=1, batch=1024, timings=timings)
    first = seen[0]
    del seen[:]
    b, _ = seg.segment(chunks, targets, lengths, poremodel, dtw=spy, workers=5, batch=5)
    assert len(seen) == 3 and np.array_equal(a, b) and ok.all()
    for x, y in zip(first, [v for part in seen for v in part]):
        assert np.array_equal(x, y)
    assert set(timings) == {"levels", "levels_wait", "device"} and timings["levels"] > 0
    assert a.dtype == np.uint16 and a.shape == targets.shape and (a[0, lengths[0]:] == 0).all() and a[0, lengths[0] - 1] == 1000
    close = np.concatenate([np.abs(a[i, :len(p)].astype(int) - p) <= 3 for i, p in enumerate(planted)])
    assert close.mean() >= dtw_cases.PLANTED_WITHIN_3, close.mean()       # measured 0.9443 (dtw_cases.py)
    with pytest.raises(ValueError):                            # a chunk longer than uint16 breakpoints can say
        seg.segment(np.zeros((1, 70000), np.float32), targets[:1], lengths[:1], poremodel, dtw=spy)


def _cli(*args):
    return subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "segment"] + list(args), cwd=ROOT, capture_output=True,
                          text=True, timeout=300)


def test_cli_without_a_device(tmp_path):
    ctc = tmp_path / "ctc"
    ctc.mkdir()
    lengths = np.array([7, 100, 33], np.uint16)
    targets = np.zeros((3, 104), np.uint8)
    for i, n in enumerate(lengths):
        targets[i, :n] = 1 + (np.arange(n) % 4)
    np.save(ctc / "chunks.npy", np.zeros((3, 1000), np.float16))
    np.save(ctc / "references.npy", targets)
    np.save(ctc / "reference_lengths.npy", lengths)
    r = _cli(str(ctc), "-n")
    assert r.returncode == 0, r.stderr
    out = np.load(ctc / "breakpoints-naive.npy")
    assert out.dtype == np.uint16 and out.shape == targets.shape
    assert np.array_equal(out, seg.naive_segment(1000, targets, lengths)[0]) and out[1, 99] == 1000 and out[1, 100] == 0
    # an existing output is skipped without --overwrite
    np.save(ctc / "breakpoints-naive.npy", np.zeros(3, np.uint16))
    r = _cli(str(ctc), "-n")
    assert r.returncode == 0 and "Skipping" in r.stderr and np.load(ctc / "breakpoints-naive.npy").shape == (3,)
    r = _cli(str(ctc), "-n", "--overwrite")
    assert r.returncode == 0 and np.array_equal(np.load(ctc / "breakpoints-naive.npy"), out)
    # suffix naming
    r = _cli(str(ctc), "-n", "-S", "v2")
    assert r.returncode == 0 and np.array_equal(np.load(ctc / "breakpoints-naive-v2.npy"), out)
    assert not (ctc / "breakpoints.npy").exists()
    # argument errors: no model where none is installed, a bad map, a bad repeat, no directory
    r = _cli(str(ctc), "-r", str(tmp_path / "absent.model"))
    assert r.returncode != 0 and "pore model" in r.stderr and "-r" in r.stderr
    for bad in (["-u", "A"], ["-u", "AX"], ["-R", "0"], ["-w", "-1"]):
        r = _cli(str(ctc), "-n", *bad)
        assert r.returncode != 0 and "error" in r.stderr, bad
    r = _cli(str(tmp_path / "nowhere"), "-n")
    assert r.returncode != 0 and "not a directory" in r.stderr
    r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "--help"], cwd=ROOT, capture_output=True, text=True, timeout=300)
    assert "segment" in r.stdout
