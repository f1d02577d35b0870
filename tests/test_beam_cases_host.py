"""CPU: the table of beam-search cases (tests/beam_cases.py) is what tests/test_gpu_beam.py takes it to be.  For every row the
oracle runs, its branch census shows the branches the row was written for, and the outputs hang together; on inputs whose path
stays -- which the older checks of the oracle (tests/test_beam.py) never had -- the oracle is compared with the float64
restatement that keys hypotheses by their state sequences.  The oracle is the GPU kernel's only reference."""
import functools
import math

import numpy as np
import pytest

import beam_cases as bc
import oracle
from pairs import PAIRS

COLS = oracle.BEAM_CENSUS


@functools.lru_cache(maxsize=None)
def _run(name):
    c = bc.BY_NAME[name]
    return oracle.beam_search(bc.scores(c), bc.ALPHA[c.nb], c.sl, c.W, c.cut, c.scale, c.offset, blank_score=bc.BLANK, want_census=True)


def test_the_table_holds_the_rows_it_promises():
    names = set(bc.BY_NAME)
    assert len(names) == len(bc.CASES)
    for nb, sl in PAIRS:
        for T in (1, 2, 63, 64, 65, 129):
            for form in ("const", "blank"):
                c = bc.BY_NAME["sweep-%d-sl%d-T%d-%s" % (nb, sl, T, form)]
                assert (c.nb, c.sl, c.T, c.N, c.W, c.cut, c.scale, c.offset) == (nb, sl, T, 3, 32, 100.0, 0.9722, 0.3498)
                assert c.with_blank == (form == "blank") and c.gen == ("ridge" if T >= 63 else "gauss")
    for sl in (2, 3, 4, 5):
        for T in (20, 65):
            c = bc.BY_NAME["nocut-4-sl%d-T%d" % (sl, T)]
            assert (c.nb, c.sl, c.T, c.W, c.cut, c.gen) == (4, sl, T, 32, 0.0, "gauss") and {"multi", "clash"} <= set(c.need)
    for gen, nb, sl in (("ridge", 5, 3), ("gauss", 4, 2)):
        for W in (1, 2, 5, 31):
            c = bc.BY_NAME["width-%s-W%d" % (gen, W)]
            assert (c.nb, c.sl, c.T, c.W, c.gen) == (nb, sl, 100, W, gen)
        for cut in (1.0, 1.5, 1e30):
            c = bc.BY_NAME["cut-%s-%g" % (gen, cut)]
            assert (c.nb, c.sl, c.T, c.cut, c.gen) == (nb, sl, 100, cut, gen)
    for nb, sl in ((6, 2), (4, 4), (4, 3)):
        for gen, need, every in (("zero", (), ("bisect", "ten_guesses", "start_tied")), ("grid", ("tie",), ()), ("steep", ("q50",), ()),
                                 ("blank_wins", (), ()), ("dominant", ("q50",), ()), ("gain10", ("far",), ())):
            c = bc.BY_NAME["%s-%d-sl%d" % (gen, nb, sl)]
            assert (c.nb, c.sl, c.T) == (nb, sl, 50) and set(need) <= set(c.need) and set(every) <= set(c.every)
    c = bc.BY_NAME["q1-5-sl4-T1"]
    assert (c.nb, c.sl, c.T, c.need) == (5, 4, 1, ("q1",))
    assert all(set(c.need) | set(c.every) <= set(COLS) for c in bc.CASES)


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_oracle_on_the_case_takes_its_branches_and_is_consistent(name):
    c = bc.BY_NAME[name]
    sc = bc.scores(c)
    assert np.array_equal(sc, bc.scores(c)) and np.all(np.isfinite(sc))
    o = _run(name)
    assert o["census_columns"] == COLS and o["census"].shape == (c.N, len(COLS))
    cen = {k: o["census"][:, i] for i, k in enumerate(COLS)}
    assert np.all(cen["blocks"] == c.T)
    for k in c.need:
        assert cen[k].sum() > 0, (k, {k: int(v.sum()) for k, v in cen.items()})
    for k in c.every:
        assert np.all(cen[k] == (1 if k == "start_tied" else c.T)), (k, cen[k])
    # counting changes nothing
    plain = oracle.beam_search(sc, bc.ALPHA[c.nb], c.sl, c.W, c.cut, c.scale, c.offset, blank_score=bc.BLANK)
    assert set(plain) == {"sequence", "qstring", "moves", "score"}
    for k in plain:
        assert np.array_equal(plain[k], o[k]), k
    # structure
    mv, seq, qs = o["moves"], o["sequence"], o["qstring"]
    assert np.all(mv[:, 0] == 1) and set(np.unique(mv)) <= {0, 1}
    assert np.array_equal(mv != 0, seq != 0) and np.array_equal(mv != 0, qs != 0)
    q = qs[qs != 0]
    assert q.min() >= 34 and q.max() <= 83                        # phred 1..50
    assert set(np.unique(seq[seq != 0])) <= {ord(ch) for ch in bc.ALPHA[c.nb][1:]}
    assert np.all(cen["q1"] <= (qs == 34).sum(1)) and np.all(cen["q50"] <= (qs == 83).sum(1))
    d = oracle.decode(sc, c.nb, c.sl, blank_score=bc.BLANK, want=("logz",))
    assert np.all(np.isfinite(o["score"])) and np.all(o["score"] <= d["logz"] + 1e-3)
    bases = mv.sum(1)
    if c.gen == "ridge":
        assert np.all(bases >= 0.3 * c.T) and np.all(bases <= 0.7 * c.T), bases
    if c.gen == "blank_wins":
        assert np.all(bases == 1)
    if c.gen == "dominant":
        assert np.all(q == 83) and np.all(bases == (c.T + 2) // 3) and np.array_equal(cen["q50"], bases)
    if c.gen == "zero":
        assert len(np.unique(q)) == 1


# seeds at which float64 and float32 break no near-tie differently (the cut's bisection compares sums that agree to ~1e-6)
STAYING = [(4, 4, 1), (5, 4, 1), (6, 2, 1)]


@pytest.mark.parametrize("nb,sl,seed", STAYING)
def test_oracle_against_the_float64_restatement_on_paths_that_stay(nb, sl, seed):
    T, N, W, cut = 48, 3, 32, 100.0
    steps, _ = bc.ridge(np.random.default_rng(seed), nb, sl, T, N)
    sc = np.ascontiguousarray(steps).reshape(T, N, -1)
    o = oracle.beam_search(sc, bc.ALPHA[nb], sl, beam_width=W, beam_cut=cut, blank_score=bc.BLANK, want_census=True)
    d = oracle.decode(sc, nb, sl, blank_score=bc.BLANK, want=("beta",))
    S, E = nb ** sl, nb + 1
    bases = o["moves"].sum(1)
    assert np.all(bases >= 0.3 * T) and np.all(bases <= 0.7 * T), bases               # the path stays
    assert o["census"][:, COLS.index("merges")].min() > 3 * T
    for n in range(N):
        M = np.full((T, S, E), bc.BLANK)
        M[:, :, 1:] = sc[:, n].reshape(T, S, nb)
        score, path, moves = bc._beam_py(M, d["beta"][:, n].astype(np.float64), nb, sl, W, math.log(cut))
        assert np.array_equal(o["moves"][n], np.array(moves, np.uint8))
        want = "".join(bc.ALPHA[nb][1 + s % nb] for s, m in zip(path, moves) if m)
        assert bc.strings(o["sequence"][n:n + 1])[0] == want
        assert abs(float(o["score"][n]) - score) < 2e-3


def test_a_cut_inside_0_1_is_refused():
    sc = bc.scores(bc.BY_NAME["sweep-4-sl2-T2-const"])
    for cut in (0.5, 1e-6, 0.999):
        with pytest.raises(ValueError, match="inside"):
            oracle.beam_search(sc, bc.ALPHA[4], 2, beam_cut=cut, blank_score=bc.BLANK)
    for cut in (1.0, 0.0, -1.0):
        oracle.beam_search(sc, bc.ALPHA[4], 2, beam_cut=cut, blank_score=bc.BLANK)


def test_compute_scores_refuses_the_cut_before_the_model_runs():
    import importlib
    bcall = importlib.import_module("xna_basecaller_amd.crf.basecall")

    class Model:
        class _Last:
            expand_blanks, blank_score = False, 2.0
        encoder = [_Last()]

        def basecall_chunks_beam(self, *a):
            raise AssertionError("the model was run")

    with pytest.raises(ValueError, match=r"beam_cut 0.5 inside \(0, 1\): no candidate can reach it"):
        bcall.compute_scores(Model(), np.zeros((1, 1, 100), np.float32), beam_cut=0.5)
