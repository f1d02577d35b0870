"""CPU: the schedule table of tests/test_gpu_schedules.py covers every branch of the encoder's host scheduler.

schedule_plan.plan() restates the C++ planner (plan_layer, csrc/xb_schedule.h); on the 256 CUs of an MI355X every row must
plan the label it names, and together the rows must reach every branch tag plan() can return.  This checks the table against
the restatement only: an edit of plan() or of the table that moves a row off its branch, or a tag no row reaches, fails here.
That the C++ planner agrees with plan() is checked on the CPU as well, case by case and launch by launch
(tests/test_schedule_host.py); the launch counts of tests/test_gpu_schedules.py show that the plan is what the GPU rows execute.
"""
import pytest

import schedule_plan as sp

CU = 256


@pytest.mark.parametrize("row", sp.ROWS, ids=[r[0] for r in sp.ROWS])
def test_row_plans_its_label(row):
    name, F, nb, L, N, env, label, anchors = row
    p = sp.plan(F, N, sp.chunk_T(L), CU, env)
    assert p["label"] == label
    assert set(p["tags"]) <= set(sp.BRANCHES)
    assert all(0 <= c < N for c in anchors)


@pytest.mark.parametrize("row", sp.PAIR_ROWS, ids=[r[0] for r in sp.PAIR_ROWS])
def test_pair_row_plans_its_labels(row):
    name, F, nb, L, max_batch, calls, labels = row
    assert max(calls) <= max_batch and len(calls) >= 2
    assert tuple(sp.plan(F, n, sp.chunk_T(L), CU)["label"] for n in sp.pair_passes(calls)) == labels


def test_table_reaches_every_branch():
    seen = set()
    for _, F, nb, L, N, env, _, _ in sp.ROWS:
        seen |= sp.plan(F, N, sp.chunk_T(L), CU, env)["tags"]
    assert seen == set(sp.BRANCHES), sorted(set(sp.BRANCHES) - seen)


def test_planned_launch_counts():
    """A few counts written out by hand from the planner, so that plan() itself is pinned."""
    T = sp.chunk_T(4000)
    assert T == 800 and sp.time_slabs(T, 6) == [0, 133, 266, 400, 533, 666, 800]
    # 6 event-ordered slabs: a recurrence launch and a GEMM per slab and layer
    assert sp.plan(768, 65, T, CU) == dict(sp.plan(768, 65, T, CU), lstm_rec=30, lstm_in=25, linear=6, nts=6)
    # signal mode: one recurrence launch per layer, still a GEMM per slab
    p = sp.plan(768, 641, T, CU)
    assert (p["lstm_rec"], p["lstm_in"], p["linear"]) == (5, 25, 6)
    # two chunk slabs (1024 + 257 chunks) x 5 time slabs, event-ordered
    p = sp.plan(768, 1281, sp.chunk_T(3600), CU)
    assert (p["lstm_rec"], p["lstm_in"], p["linear"], p["chunk_slabs"]) == (50, 21, 5, 2)
    # above 64 groups: five chunk slabs over all steps, the GEMMs after the layer
    p = sp.plan(768, 4161, sp.chunk_T(1000), CU)
    assert (p["lstm_rec"], p["lstm_in"], p["linear"], p["chunk_slabs"]) == (25, 5, 1, 5)
    # XB_OVERLAP=2: the recurrence in slabs, one GEMM per layer on the main stream
    p = sp.plan(768, 641, T, CU, {"XB_OVERLAP": "2"})
    assert (p["lstm_rec"], p["lstm_in"], p["linear"]) == (30, 5, 1)
    # the serial order: one launch per step
    p = sp.plan(768, 700, T, CU, sp.REFERENCE_ENV)
    assert (p["lstm_rec"], p["lstm_in"], p["linear"]) == (5 * 800, 5, 1)
    with pytest.raises(ValueError):
        sp.plan(768, 4097, T, CU, sp.REFERENCE_ENV)
    # 64 CUs hold no group of 24 members: one launch per step, and the persistent mode is refused when asked for by name
    assert sp.plan(768, 65, T, 64)["label"] == "per-step"
    with pytest.raises(ValueError):
        sp.plan(768, 65, T, 64, {"XB_LSTM_MODE": "2"})
    # a device whose CU count gives no wide range: 513 chunks take the two-groups-per-workgroup kernel
    assert sp.plan(768, 513, T, 192)["label"] == "dual/signal/uneven/ragged"
