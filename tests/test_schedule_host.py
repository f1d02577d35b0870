"""CPU: the C++ planner of the encoder schedule (csrc/xb_schedule.h, reached through libxnacall.so's non-public
xb_internal_* exports) against its Python restatement, schedule_plan.plan(), and against the invariants every launch of a
plan must keep.

Three parts.  (1) Over every feature size, CU count, step count at the time-slab seams, batch at the chunk-slab seams,
device fact and knob set, the C plan and plan() name the same placement, ordering, slab counts and launch counts, and
refuse the same queries.  (2) What launch counts cannot see -- the chunks, steps, group slot, XCD-mask byte and arrival base
of every launch -- is checked on the launch records themselves.  (3) The knob parser against schedule_plan.knobs(), and
the batch up to which two calls pair.  tests/test_gpu_schedules.py then only has to show that the plan is executed."""
import itertools

import pytest

import host_logic as hl
import schedule_plan as sp

FEATURES = (32, 64, 96, 128, 256, 384, 512, 768)
CU_COUNTS = (64, 192, 256, 304)
STEPS = (1, 2, 124, 125, 249, 250, 720, 800)
STEPS_8 = (128, 136, 512, 520)          # 16, 17, 64 and 65 slabs of at least XB_SLAB_STEPS=8 steps
BN = sp.LG_BN


def _envs():
    envs = [dict(row[5]) for row in sp.ROWS]
    envs += [{"XB_LSTM_DUAL": "0"}, {"XB_LSTM_DUAL": "2"}, {"XB_OVERLAP": "0"}, {"XB_OVERLAP": "2"}, {"XB_LSTM_MODE": "1"},
             {"XB_LSTM_MODE": "2"}]
    unique = []
    for e in envs:
        if e not in unique:
            unique.append(e)
    return unique


ENVS = _envs()


def slots(F, cu_count):
    """(gslab0, gwide): group slots of a launch in the XCD-local placement and with the groups dealt over all XCDs."""
    members = F // sp.LG_UNITS
    return min(8 * ((cu_count // 8) // members), 64), min(cu_count // members, 64)


def batches(F, cu_count):
    """The batch sizes at the seams: one group, the capacities of a launch in every placement, the 64 group slots."""
    gslab0, gwide = slots(F, cu_count)
    ns = {1, 63, 64, 65, 4095, 4096, 4097, 4161}
    for k in (gslab0, gwide, 2 * gslab0, 2 * gwide):
        ns |= {k * BN - 1, k * BN, k * BN + 1}
    return sorted(n for n in ns if n >= 1)


def steps(env):
    return STEPS + (STEPS_8 if env.get("XB_SLAB_STEPS") == "8" else ())


def placement(p):
    if p.mode != 2:
        return "per-step"
    return ("wide-dual" if p.dual_batch else "wide") if p.wide else ("dual" if p.dual_batch else "single")


def test_the_grid_holds_what_it_is_meant_to():
    assert {"XB_LSTM_DUAL": "0"} in ENVS and {"XB_LSTM_MODE": "2"} in ENVS and len(ENVS) == 15
    assert all(row[5] in ENVS for row in sp.ROWS)
    assert [sp.plan(768, 512, T, 256, {"XB_SLAB_STEPS": "8", "XB_TIME_SLABS": "80"})["nts"] for T in STEPS_8] == [16, 17, 64, 65]
    assert slots(768, 256) == (8, 10) and batches(768, 256)[4:16] == [511, 512, 513, 639, 640, 641, 1023, 1024, 1025, 1279, 1280, 1281]
    assert slots(768, 64) == (0, 2) and slots(32, 304) == (64, 64)


@pytest.mark.parametrize("F", FEATURES)
def test_planner_equals_the_restatement(F):
    planner = hl.Planner()
    cases = refused = 0
    for env in ENVS:
        k = sp.knobs(env)
        planner.set_knobs(k)
        for cu, T in itertools.product(CU_COUNTS, steps(env)):
            for n, dual_ok, signal_ok in itertools.product(batches(F, cu), (True, False), (True, False)):
                cases += 1
                try:
                    want = sp.plan(F, n, T, cu, env, dual_ok, signal_ok)
                except ValueError:
                    want = None
                p, launches = planner.plan(F, n, T, cu, dual_ok, signal_ok)
                where = (F, n, T, cu, env, dual_ok, signal_ok)
                if want is None:
                    refused += 1
                    assert launches is None and p.error == -1 and p.message, where
                    continue
                assert launches is not None, (where, p.message)
                tags = want["tags"]
                # (the per-step label names no ordering: it is the serial one)
                ordering = hl.ORDERING_TAGS[p.ordering]
                assert placement(p) in tags and (ordering in tags if p.mode == 2 else ordering == "serial"), (where, want["label"])
                assert len(tags & {"per-step", "single", "dual", "wide", "wide-dual"}) == 1 and len(tags & set(hl.ORDERING_TAGS)) == (p.mode == 2)
                assert (p.nts, p.chunk_slabs, p.rec_launches, p.gemm_slabs) == \
                    (want["nts"], want["chunk_slabs"], want["lstm_rec"] // sp.LAYERS, want["linear"]), (where, want["label"])
                assert want["lstm_in"] == 1 + (sp.LAYERS - 1) * p.gemm_slabs
                if p.mode != 2:                      # "per-step" is the whole label
                    assert p.spread == k["XB_LSTM_SPREAD"] and len(launches) == 1
                    continue
                assert bool(p.spread and not p.wide) == ("spread" in tags) and (not p.global_groups) == ("local-groups" in tags), where
                tail = launches[-1]
                assert bool(p.dual_batch and not tail[4]) == ("single-tail" in tags), (where, want["label"])
    assert cases > 20000 and refused > 0


def check_launches(p, launches, k, F, n, T, cu, dual_ok):
    """The invariants of one plan's launch records (n0, nslab, s_begin, s_end, dual, grp0, slab, xcd_local, sync_base)."""
    L = launches.tolist()
    local, dual_knob = int(bool(k["XB_LSTM_LOCAL"])), k["XB_LSTM_DUAL"]
    if p.mode != 2:                                  # one launch per step, issued from the one record
        assert L == [[0, n, 0, T, int(dual_ok and dual_knob == 2 and n > BN), 0, 0, 0, 0]]
        assert p.rec_launches == T and n <= 64 * BN
        return
    gslab0, gwide = slots(F, cu)
    gslab = gwide if p.wide else gslab0
    assert p.gslab == gslab
    # two groups per workgroup: today's rule per XB_LSTM_DUAL value, for the batch and then for every launch of it
    threshold = BN if dual_knob == 2 else gslab * BN
    assert p.dual_batch == int(dual_ok and dual_knob != 0 and n > threshold)
    assert p.slab == (min(2 * gslab, 64) if p.dual_batch else gslab) * BN
    if p.ordering == hl.SIGNAL:
        assert L == [[0, n, 0, T, p.dual_batch, 0, 0, local, 0]]
        assert n <= p.slab and 2 <= p.nts <= 64 and p.rec_launches == 1
    else:
        assert len(L) == p.nts * p.chunk_slabs == p.rec_launches
        assert p.global_groups == (n <= 64 * BN) and (p.global_groups or p.nts == 1)
        bounds = sp.time_slabs(T, p.nts)             # time slabs partition [0, T) at T * i / nts
        assert bounds[0] == 0 and bounds[-1] == T
        rows = iter(L)
        arrivals = 0                                 # the sum of len - 1 of the earlier time slabs
        for i in range(p.nts):
            assert bounds[i] < bounds[i + 1]
            at = 0                                   # chunk slabs partition [0, n) in order, within every time slab
            for _ in range(p.chunk_slabs):
                n0, nslab, s_begin, s_end, dual, grp0, slab, xcd_local, sync_base = next(rows)
                assert n0 == at and 1 <= nslab <= p.slab and (s_begin, s_end, slab) == (bounds[i], bounds[i + 1], i)
                assert xcd_local == (local if i < 16 else 0)
                assert (grp0, sync_base) == ((n0 // BN, arrivals) if p.global_groups else (0, 0))
                assert dual == int(p.dual_batch and nslab > threshold)
                at += nslab
            assert at == n
            arrivals += bounds[i + 1] - bounds[i] - 1
    for n0, nslab, s_begin, s_end, dual, grp0, slab, xcd_local, sync_base in L:
        groups = -(-nslab // BN)
        # a launch fits its group slots: 64 at the most with two groups per workgroup, one slot per group otherwise; and
        # with global groups the 64 slots of the exchange buffer and the counters
        assert groups <= (min(2 * gslab, 64) if dual else gslab) and grp0 + groups <= 64


@pytest.mark.parametrize("F", FEATURES)
def test_launch_records_keep_their_invariants(F):
    planner = hl.Planner()
    seen = set()
    for env in ENVS:
        k = sp.knobs(env)
        planner.set_knobs(k)
        for cu, T in itertools.product(CU_COUNTS, (1, 250, 800) + steps(env)[len(STEPS):]):
            for n, dual_ok, signal_ok in itertools.product(batches(F, cu), (True, False), (True, False)):
                p, launches = planner.plan(F, n, T, cu, dual_ok, signal_ok)
                if launches is None:
                    continue
                check_launches(p, launches, k, F, n, T, cu, dual_ok)
                seen.add((placement(p), hl.ORDERING_TAGS[p.ordering], bool(p.global_groups), p.nts > 16))
    assert {s[1] for s in seen} == set(hl.ORDERING_TAGS) and {s[0] for s in seen} >= {"per-step", "single", "dual"}
    if F == 768:
        assert {s[0] for s in seen} == {"per-step", "single", "dual", "wide", "wide-dual"}
        assert {s[2] for s in seen} == {True, False} and {s[3] for s in seen} == {True, False}


def test_planner_without_a_consumer_and_without_residency():
    """The two query fields the restatement has no parameter for: a layer nobody consumes is never slabbed, and a device
    that cannot keep the persistent kernel resident plans one launch per step (or refuses XB_LSTM_MODE=2)."""
    planner = hl.Planner()
    planner.set_knobs(sp.knobs({}))
    p, launches = planner.plan(768, 700, 800, 256, has_next=False)
    assert (p.mode, p.nts, p.ordering, p.gemm_slabs, p.rec_launches) == (2, 1, hl.SERIAL, 0, 1) and len(launches) == 1
    p, launches = planner.plan(768, 700, 800, 256, resident1=False)
    assert (p.mode, p.rec_launches, p.gemm_slabs) == (1, 800, 1)
    planner.set_knobs(sp.knobs({"XB_LSTM_MODE": "2"}))
    p, launches = planner.plan(768, 700, 800, 256, resident1=False)
    assert launches is None and p.error == -1
    assert p.message == b"persistent LSTM needs 24 co-resident workgroups, device has 256 CUs"
    planner.set_knobs(sp.knobs(sp.REFERENCE_ENV))
    p, launches = planner.plan(768, 4097, 800, 256)
    assert launches is None and p.message == b"one-launch-per-step LSTM mode handles at most 4096 chunks per batch"


@pytest.mark.parametrize("env", [{}, {"XB_TIME_SLABS": "0"}, {"XB_SLAB_STEPS": "7"}, {"XB_LSTM_SIGNAL": "3"}, {"XB_LSTM_SIGNAL": "-1"},
                                 {"XB_TIME_SLABS": "80", "XB_SLAB_STEPS": "8", "XB_LSTM_SIGNAL": "1"}, sp.REFERENCE_ENV,
                                 {"XB_LSTM_DUAL": "2", "XB_OVERLAP": "2", "XB_LSTM_LOCAL": "0", "XB_LSTM_MODE": "2"}],
                         ids=lambda e: ",".join("%s=%s" % (k[3:], v) for k, v in e.items()) or "defaults")
def test_knobs_from_env_equal_the_restatement(env, monkeypatch):
    for _, name in hl.KNOBS:
        monkeypatch.delenv(name, raising=False)
    for name, v in env.items():
        monkeypatch.setenv(name, v)
    got, want = hl.knobs_from_env(), sp.knobs(env)
    for field, name in hl.KNOBS:
        if name in want:
            assert got[field] == want[name], name
    if not env:
        assert got == {"lstm_mode": 0, "lstm_dual": 1, "lstm_wide": 1, "lstm_local": 1, "lstm_signal": 2, "lstm_i8": 0, "overlap": 1,
                       "time_slabs": 16, "slab_steps": 0, "fuse": 1, "decode_async": 0, "in1_layers": 31, "x3_stages": -1,
                       "gemm4": 1, "gemm_sn": 0, "gemm_shadow_kernel": 0, "gemm_shadow_wgs": 2}


def test_knob_clamps_outside_the_schedule(monkeypatch):
    for name, v, field, want in (("XB_LSTM_I8", "2", "lstm_i8", 2), ("XB_LSTM_I8", "7", "lstm_i8", 1), ("XB_IN1_LAYERS", "33", "in1_layers", 1),
                                 ("XB_X3_STAGES", "0x1fff", "x3_stages", 0xfff), ("XB_GEMM_SN", "65", "gemm_sn", 0),
                                 ("XB_GEMM_SN", "64", "gemm_sn", 64), ("XB_GEMM_SHADOW", "8", "gemm_shadow_kernel", 8),
                                 ("XB_GEMM_SHADOW", "5", "gemm_shadow_kernel", 0), ("XB_GEMM_SHADOW_WGS", "1", "gemm_shadow_wgs", 1),
                                 ("XB_GEMM_SHADOW_WGS", "3", "gemm_shadow_wgs", 2), ("XB_LSTM_WIDE", "5", "lstm_wide", 1),
                                 ("XB_FUSE", "0", "fuse", 0), ("XB_DECODE_ASYNC", "2", "decode_async", 1), ("XB_GEMM4", "0", "gemm4", 0)):
        monkeypatch.setenv(name, v)
        assert hl.knobs_from_env()[field] == want, (name, v)
        monkeypatch.delenv(name)


def test_pair_capacity():
    cap = hl.lib().xb_internal_pair_capacity
    assert cap(768, 256, 1) == 640
    assert cap(768, 256, 0) == 512 and cap(384, 256, 1) == 512 and cap(768, 192, 1) == 512
    for name, F, nb, L, max_batch, calls, labels in sp.PAIR_ROWS:
        assert max_batch <= cap(F, 256, 1), name
