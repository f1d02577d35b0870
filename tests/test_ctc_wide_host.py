"""CPU tier of the wide CTC rows (tests/ctc_wide_cases.py): what the GPU tier's reference is worth at 513 .. 2048 positions.

The oracle (float32) against the float64 lattice, the two exact properties the GPU tier asserts on the device without the
oracle (a single path sums its move scores in time order, bit for bit; a row without a path gives Log.zero exactly), the gather
indices at a 2050-wide row, and the table itself: no case is vacuous, every prefetch-ring residue, every instantiation of
ctc_loss_kernel and ctc_scan_kernel and every slot occurs.  Then the library's own column and launch rules
(csrc/xb_ctc_lattice.h, through tests/host_logic.py) against the oracle's indices and the table's restatement."""
import numpy as np
import pytest

import oracle
import ctc_wide_cases as W
import host_logic as hl
from pairs import PAIRS, PAIR_IDS


def test_table_covers_what_it_claims():
    # both sides of every step of the thread rule and of every slot boundary, and the limit
    nps = {c.np for c in W.LOSS_CASES}
    assert {64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 2048} <= nps
    assert {c.np for c in W.SCAN_CASES} >= {64, 65, 128, 129, 256, 257, 512, 513, 1024, 1025, 1793, 2047, 2048}
    assert max(nps) == W.THREADS * W.PMAX
    for c in W.LOSS_CASES:
        assert c.np + 1 <= c.T <= c.np + 4
    assert {c.T % 4 for c in W.SCAN_CASES if (c.nb, c.sl) == (4, 3)} == {0, 1, 2, 3}
    assert {(c.nb, c.sl) for c in W.SCAN_CASES} == {(4, 3), (6, 3), (5, 2), (4, 5)}
    # a lone position in slots 1, 2, 4 and 7, every slot live at 2048; the half chunks end one past a multiple of 256
    assert {(c.np - 1) // W.THREADS for c in W.SCAN_CASES if c.np % W.THREADS == 1} == {1, 2, 4, 7}
    assert {l // W.THREADS for l in range(2048)} == set(range(W.PMAX))
    for c in W.SCAN_CASES:
        if c.np >= W.THREADS:
            assert W.half_positions(c.np) in (129, 257, 513, 1025) and W.half_positions(c.np) < c.np
        else:                        # the rows at the thread rule's steps: just over half
            assert W.half_positions(c.np) == c.np // 2 + 1 < c.np
    # PMAX 1, 2, 4, 8 of either kernel: by the rule over the table, and the overrides' own launches
    for cases in (W.LOSS_CASES, W.SCAN_CASES):
        assert {W.loss_launch(c.np)[1] for c in cases} == {1, 2, 4, 8}
        assert {W.loss_launch(c.np)[0] for c in cases} == {64, 128, 256}
    got = [W.loss_launch(n, o) for n, o in W.THREAD_OVERRIDES]
    assert got == [(64, 4), (64, 8), (128, 4), (64, 8), (128, 8), (256, 8), (256, 4), (256, 2)]


@pytest.mark.parametrize("c", W.LOSS_CASES, ids=W.case_id)
def test_no_case_is_vacuous(c):
    """A condition on the reference alone: the full row has a path (logz above Log.zero) and its last position is live (a
    positive restricted posterior), so a kernel that never computed the row's far end could not pass."""
    sc, targets, lens = W.build(c)
    assert lens.tolist() == [c.np + c.sl - 1, W.half_positions(c.np) + c.sl - 1, c.sl]
    o = oracle.ctc_logz(sc, targets, lens, c.nb, c.sl, want_grads=True)
    assert np.all(o["logz"] > -1e30)
    assert o["stay"][:, 0, c.np - 1].max() > 0
    assert o["stay"][:, 1, W.half_positions(c.np) - 1].max() > 0
    # the one-position chunk: the running float32 sum of its stay scores, in both semirings
    om = oracle.ctc_logz(sc, targets, lens, c.nb, c.sl, semiring="max")
    want = W.stay_sum(sc, targets, 2, c.nb, c.sl)
    assert o["logz"][2] == want and om["logz"][2] == want


@pytest.mark.parametrize("np_", W.F64_POSITIONS)
def test_oracle_against_float64_at_wide_rows(np_):
    c = [c for c in W.SCAN_CASES if c.np == np_ and (c.nb, c.sl) == (4, 3)][0]
    sc, targets, lens = W.build(c)
    stay_idx, move_idx = oracle.ctc_indices(targets, c.nb, c.sl)
    npos = lens + 1 - c.sl
    o = oracle.ctc_logz(sc, targets, lens, c.nb, c.sl, want_grads=True)
    om = oracle.ctc_logz(sc, targets, lens, c.nb, c.sl, semiring="max")
    lz = W.lattice_f64(sc, stay_idx, move_idx, npos)
    best = W.lattice_f64(sc, stay_idx, move_idx, npos, "max")
    scale = np.maximum(1.0, np.abs(lz))
    d_log = float((np.abs(o["logz"] - lz) / scale).max())
    d_max = float((np.abs(om["logz"] - best) / np.maximum(1.0, np.abs(best))).max())
    # the gradient: every path takes one edge per time step, so stay + move sums to 1 at every step of a feasible chunk
    total = o["stay"].sum(axis=2, dtype=np.float64) + o["move"].sum(axis=2, dtype=np.float64)
    d_sum = float(np.abs(total - 1.0).max())
    print("np %d: |logz - f64| / max(1, |logz|) = %.3g (Log), %.3g (Max); |sum of posteriors - 1| = %.3g; logz %s"
          % (np_, d_log, d_max, d_sum, o["logz"]))
    assert d_log <= W.F64_LOGZ_BOUND
    assert d_max <= W.F64_MAX_BOUND
    assert d_sum <= W.F64_GRADSUM_BOUND


@pytest.mark.parametrize("np_", W.PROPERTY_POSITIONS)
def test_oracle_single_path_and_infeasible_rows_are_exact(np_):
    nb, sl = 4, 3
    sc, targets, lens = W.build_single_path(np_)
    assert sc.shape[0] == np_ - 1
    want = [W.diagonal_sum(sc, targets, 0, nb, sl, np_ - 1), W.stay_sum(sc, targets, 1, nb, sl)]
    for semiring in ("log", "max"):
        o = oracle.ctc_logz(sc, targets, lens, nb, sl, semiring=semiring, want_grads=semiring == "max")
        assert o["logz"].tolist() == want
    assert np.array_equal(o["stay"][:, 0, :np_ - 1], np.eye(np_ - 1, dtype=np.float32))          # the alignment is the diagonal
    assert np.all(o["stay"][:, 0, np_ - 1] == 0) and np.all(o["stay"][:, 1, 0] == 1)

    sc, targets, lens = W.build_infeasible(np_)
    assert sc.shape[0] == np_ - 2
    for semiring in ("log", "max"):
        o = oracle.ctc_logz(sc, targets, lens, nb, sl, semiring=semiring)
        assert o["logz"][0] == W.ZERO
        assert o["logz"][1] == W.diagonal_sum(sc, targets, 1, nb, sl, np_ - 2) and o["logz"][1] > -1e30


@pytest.mark.parametrize("nb,sl", [(4, 3), (6, 3), (5, 2), (4, 5)])
def test_oracle_ctc_indices_at_a_2050_wide_row(nb, sl):
    """The gather indices against the reference's expression (crf/model.py:108-114) written out in numpy, as
    tests/test_ctc.py does at Lt = 14."""
    N, Lt = 3, 2050
    targets, _ = W.label_rows(np.random.default_rng(nb + sl), N, Lt, nb, sl, lens=[Lt, 1100, sl])
    stay_idx, move_idx = oracle.ctc_indices(targets, nb, sl)
    t0 = np.clip(targets.astype(np.int64) - 1, 0, None)
    n = Lt - (sl - 1)
    ref_stay = sum(t0[:, i:n + i] * nb ** (sl - i - 1) for i in range(sl)) * (nb + 1)
    assert stay_idx.shape == (N, n) and move_idx.shape == (N, n - 1)
    assert np.array_equal(stay_idx, ref_stay) and np.array_equal(move_idx, ref_stay[:, 1:] + t0[:, :n - 1] + 1)
    assert stay_idx.max() < nb ** sl * (nb + 1) and move_idx.max() < nb ** sl * (nb + 1)


# ---- the library's own rules (csrc/xb_ctc_lattice.h), through its host-logic exports ---------------------------------------------
@pytest.mark.parametrize("nb,sl", PAIRS, ids=PAIR_IDS)
def test_library_column_rule_is_the_oracles(nb, sl):
    """What xb_ctc_logz's host used to compute and upload: the stay column of every position and the move column into every
    position l >= 1, on ragged rows whose tails are label 0 (which reads as base 0).  The blank-less layout and the posteriors'
    column follow from the same state: st nb + base, and the blank layout's move column."""
    N, Lt = 5, 40
    targets, lens = W.label_rows(np.random.default_rng(nb * 8 + sl), N, Lt, nb, sl)
    assert (targets == 0).any() and lens[0] == Lt and lens[-1] == sl
    stay_idx, move_idx = oracle.ctc_indices(targets, nb, sl)
    stay, move, post = hl.ctc_columns(targets, nb, sl)
    assert stay.shape == stay_idx.shape == (N, Lt - sl + 1)
    assert np.array_equal(stay, stay_idx)
    assert np.array_equal(move[:, 1:], move_idx) and np.array_equal(post[:, 1:], move_idx)
    assert np.all(move[:, 0] == 0) and np.all(post[:, 0] == 0)
    _, move_nb, post_nb = hl.ctc_columns(targets, nb, sl, has_blank=False)
    assert np.array_equal(post_nb, post)
    state, edge = move_idx // (nb + 1), move_idx % (nb + 1)
    assert edge.min() >= 1 and np.array_equal(move_nb[:, 1:], state * nb + edge - 1) and np.all(move_nb[:, 0] == 0)


def test_library_launch_rule_is_the_restatement():
    for c in W.LOSS_CASES:
        threads, pmax, lds = hl.ctc_launch(c.np)
        assert (threads, pmax) == W.loss_launch(c.np), c
        assert threads * pmax >= c.np and lds == 4 * 2 * (c.np + 2)
        # the gradient kernel's launch: the same workgroup, the chains' room behind the position vector
        assert hl.ctc_launch(c.np, chains=True) == (threads, pmax, lds + 4 * 4 * c.np + 4 * c.np + 2 * c.np)
    for np_, value in W.THREAD_OVERRIDES:
        assert hl.ctc_launch(np_, value)[:2] == W.loss_launch(np_, value), (np_, value)
    assert hl.ctc_launch(1)[:2] == (64, 1) and hl.ctc_launch(2048)[:2] == (256, 8)
    assert hl.ctc_launch(2049)[1] == 0                        # refused: more than 8 positions per thread
