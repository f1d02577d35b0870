"""CPU: the bottom pass of the top-layer trainer (encoder_bottom_run, csrc/xb_run_encoder.hip) runs its last LSTM layer without a
consumer: run_lstm_layer is called with next = nullptr.  That function dereferences `next` only where the plan issues slab
GEMMs beside the recurrence (the orderings `events` and `signal`) and, guarded, after it.  The planner must therefore never plan
a slab GEMM for a query with has_next = 0 -- whatever the batch, the width, the device and the knobs."""
import itertools

import pytest

import host_logic as hl
import schedule_plan as sp

FEATURES = (32, 96, 768)
BATCHES = (1, 6, 64, 65, 384, 512)
STEPS = (40, 720)
CU_COUNTS = (64, 256, 304)
# the default knobs, every knob row of the schedule tests' table, and the knobs that force an overlapped ordering
ENVS = [{}] + [dict(row[5]) for row in sp.ROWS] + [{"XB_OVERLAP": "2"}, {"XB_LSTM_SIGNAL": "1"}, {"XB_LSTM_MODE": "2"},
                                                   {"XB_SLAB_STEPS": "8", "XB_TIME_SLABS": "80"}]
NO_SLAB_GEMM = (hl.SERIAL, hl.SLABS_SERIAL_GEMM)


@pytest.mark.parametrize("F", FEATURES)
def test_a_layer_without_a_consumer_plans_no_slab_gemm(F):
    planner = hl.Planner()
    planned = 0
    for env in ENVS:
        planner.set_knobs(sp.knobs(env))
        for n, T, cu, dual_ok, signal_ok in itertools.product(BATCHES, STEPS, CU_COUNTS, (True, False), (True, False)):
            p, launches = planner.plan(F, n, T, cu, dual_ok, signal_ok, has_next=False)
            if launches is None:                      # a refused query launches nothing at all
                assert p.error == -1 and p.message
                continue
            planned += 1
            assert p.gemm_slabs == 0 and p.ordering in NO_SLAB_GEMM, (F, n, T, cu, env, dual_ok, signal_ok, hl.ORDERING_TAGS[p.ordering])
    assert planned > 1000


def test_the_same_queries_with_a_consumer_do_plan_slab_gemms():
    """... so the assertion above is about has_next, not about queries that never overlap."""
    planner = hl.Planner()
    planner.set_knobs(sp.knobs({}))
    p, _ = planner.plan(768, 512, 720, 256, has_next=True)
    assert p.gemm_slabs > 1 and p.ordering not in NO_SLAB_GEMM
    p, _ = planner.plan(768, 512, 720, 256, has_next=False)
    assert p.gemm_slabs == 0 and p.ordering in NO_SLAB_GEMM
