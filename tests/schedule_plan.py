"""
Python restatement of the encoder's host scheduler (plan_layer, xna_basecaller_amd/csrc/xb_schedule.h, as run_encoder /
run_lstm_layer of xb_run_encoder.hip execute it) and the table of schedules that tests/test_gpu_schedules.py runs.
tests/test_schedule_host.py holds the C++ planner to this restatement, case by case, without a GPU.

plan(F, n, T, cu_count, env) predicts, for one encoder pass over n chunks of T steps, which plan every LSTM layer takes and
how many launches the stage counters (xb_get_stage_times) record: `lstm_rec` recurrence launches, `lstm_in` input
projections (the first one plus one per time slab of layers 0..3), `linear` CRF linear slabs (one per time slab of layer 4).
Every layer takes the same plan under XB_PREC_MIXED (one recurrence arithmetic for all five layers), so the counts are
five times one layer's.  What the planner reads from the device but this restatement cannot see -- the occupancy query
behind `dual_ok` and hipStreamWaitValue32 support behind signal mode -- are parameters that default to what an MI355X has.
"""

LG_BN = 64          # chunks per group (xb_lstm.hip LG_BN)
LG_UNITS = 32       # hidden units per member workgroup (xb_lstm.hip LG_UNITS)
LAYERS = 5

# the knobs the scheduler reads (xb::knobs_from_env), with the library's defaults
DEFAULTS = {"XB_LSTM_MODE": 0, "XB_OVERLAP": 1, "XB_TIME_SLABS": 16, "XB_SLAB_STEPS": 0, "XB_LSTM_SIGNAL": 2,
            "XB_LSTM_DUAL": 1, "XB_LSTM_WIDE": 1, "XB_LSTM_LOCAL": 1, "XB_LSTM_SPREAD": 0, "XB_FUSE": 1}

# the one-launch-per-step serial order every schedule is compared with (tests/test_gpu_schedules.py)
REFERENCE_ENV = {"XB_LSTM_MODE": "1", "XB_OVERLAP": "0", "XB_LSTM_DUAL": "0", "XB_LSTM_WIDE": "0", "XB_FUSE": "0"}

# every branch tag plan() can put into a label
#   placement:  per-step (mode 1), single (one group per workgroup), dual (two), wide / wide-dual (groups dealt over all
#               XCDs up to cu_count / members slots), spread (XB_LSTM_SPREAD below the wide range)
#   ordering:   serial (one time slab, GEMM after the layer), events (a launch per time slab, the slab GEMM waits on an
#               event), signal (one launch, the slab GEMM waits on the flag word), slabs-serial-gemm (XB_OVERLAP=2)
#   details:    uneven (time slabs of unequal length), chunk-slabs (more than one chunk slab), single-tail (the last chunk
#               slab of a dual batch runs one group per workgroup), ragged (a group with fewer than 64 chunks),
#               local-groups (batch above 64 group slots: launch-local counters), no-overlap (T below two slabs),
#               mask-ends (time slabs past the 16 XCD mask bytes), signal-limit (64 slabs in signal mode),
#               write-through (XB_LSTM_LOCAL=0)
BRANCHES = ("per-step", "single", "dual", "wide", "wide-dual", "spread",
            "serial", "events", "signal", "slabs-serial-gemm",
            "uneven", "chunk-slabs", "single-tail", "ragged", "local-groups", "no-overlap", "mask-ends", "signal-limit",
            "write-through")


def knobs(env):
    k = dict(DEFAULTS)
    for name, v in (env or {}).items():
        k[name] = int(v)
    # the clamps of xb::knobs_from_env
    k["XB_TIME_SLABS"] = k["XB_TIME_SLABS"] if k["XB_TIME_SLABS"] > 0 else 1
    k["XB_SLAB_STEPS"] = k["XB_SLAB_STEPS"] if k["XB_SLAB_STEPS"] >= 8 else 0
    k["XB_LSTM_SIGNAL"] = k["XB_LSTM_SIGNAL"] if 0 <= k["XB_LSTM_SIGNAL"] <= 2 else 2
    return k


def time_slabs(T, nts):
    """Boundaries of nts time slabs over T steps (LayerPlan::step0: s_i = T * i / nts)."""
    return [T * i // nts for i in range(nts + 1)]


def plan(F, n, T, cu_count, env=None, dual_ok=True, signal_ok=True):
    """-> dict(label, tags, lstm_rec, lstm_in, linear, nts, chunk_slabs) for one encoder pass of n chunks."""
    k = knobs(env)
    members, bn = F // LG_UNITS, LG_BN
    gmax = 8 * ((cu_count // 8) // members)
    tags = []
    if k["XB_LSTM_MODE"] == 1 or (k["XB_LSTM_MODE"] == 0 and gmax < 1):
        if n > 64 * bn:
            raise ValueError("the one-launch-per-step mode handles at most %d chunks" % (64 * bn))
        tags = ["per-step"]
        rec, gemms = T, 1
        nts, nslabs = 1, 1
    else:
        if gmax < 1:
            raise ValueError("the persistent mode needs %d co-resident workgroups, %d CUs hold no group" % (members, cu_count))
        dual_ok = dual_ok and k["XB_LSTM_DUAL"] != 0
        gslab0 = min(gmax, 64)
        slots = cu_count // members
        gwide = min(slots, 64) if k["XB_LSTM_WIDE"] and slots > gslab0 else gslab0
        wide = gwide > gslab0 and (gslab0 * bn < n <= gwide * bn or
                                   (dual_ok and k["XB_LSTM_DUAL"] == 1 and 2 * gslab0 * bn < n <= 2 * gwide * bn))
        gslab = gwide if wide else gslab0

        def is_dual(m):
            return dual_ok and (m > bn if k["XB_LSTM_DUAL"] == 2 else m > gslab * bn)

        dual_batch = is_dual(n)
        slab = (min(2 * gslab, 64) if dual_batch else gslab) * bn
        global_groups = n <= 64 * bn
        min_steps = k["XB_SLAB_STEPS"] if k["XB_SLAB_STEPS"] > 0 else 125
        nts = min(T // min_steps, k["XB_TIME_SLABS"])
        overlapped = bool(k["XB_OVERLAP"]) and global_groups and nts >= 2
        if not overlapped:
            nts = 1
        starts = list(range(0, n, slab))
        nslabs = len(starts)
        signal_mode = k["XB_LSTM_SIGNAL"] == 1 or (k["XB_LSTM_SIGNAL"] == 2 and dual_batch)
        signal = (overlapped and k["XB_OVERLAP"] == 1 and signal_mode and signal_ok and n <= slab and nts <= 64)

        tags.append(("wide-dual" if dual_batch else "wide") if wide else ("dual" if dual_batch else "single"))
        if not wide and k["XB_LSTM_SPREAD"]:
            tags.append("spread")
        if signal:
            tags.append("signal")
            rec = 1
        else:
            tags.append("serial" if not overlapped else ("events" if k["XB_OVERLAP"] == 1 else "slabs-serial-gemm"))
            rec = nts * nslabs
        gemms = nts if overlapped and k["XB_OVERLAP"] == 1 else 1
        if nts > 1 and T % nts:
            tags.append("uneven")
        if nslabs > 1:
            tags.append("chunk-slabs")
        if dual_batch and not is_dual(n - starts[-1]):
            tags.append("single-tail")
        if n % bn:
            tags.append("ragged")
        if not global_groups:
            tags.append("local-groups")
        if global_groups and k["XB_OVERLAP"] and T // min_steps < 2:
            tags.append("no-overlap")
        if not signal and nts > 16 and k["XB_LSTM_LOCAL"]:
            tags.append("mask-ends")
        if signal and nts == 64:
            tags.append("signal-limit")
        if not k["XB_LSTM_LOCAL"]:
            tags.append("write-through")
    return {"label": "/".join(tags), "tags": frozenset(tags), "lstm_rec": LAYERS * rec,
            "lstm_in": 1 + (LAYERS - 1) * gemms, "linear": gemms, "nts": nts, "chunk_slabs": nslabs}


def chunk_T(L, winlen=19, stride=5):
    """Time steps of a chunk of L samples (xb_ctx_create)."""
    return (L + 2 * (winlen // 2) - winlen) // stride + 1


# One row: id, features, nb, chunk length L, batch N, knobs, the label plan() gives it on 256 CUs (the plan it must hit),
# and the chunks whose scores are checked against the fp32 oracle (empty: none).
ROWS = [
    ("L4000-N1", 768, 6, 4000, 1, {}, "single/events/uneven/ragged", ()),
    ("L4000-N65", 768, 6, 4000, 65, {}, "single/events/uneven/ragged", (0, 63, 64)),
    ("L4000-N513", 768, 6, 4000, 513, {}, "wide/events/uneven/ragged", (511, 512)),
    ("L4000-N640", 768, 6, 4000, 640, {}, "wide/events/uneven", (639,)),
    ("L4000-N641", 768, 6, 4000, 641, {}, "dual/signal/uneven/ragged", (640,)),
    ("L3600-N1000", 768, 6, 3600, 1000, {}, "dual/signal/ragged", (511, 512, 999)),
    ("L3600-N1025", 768, 6, 3600, 1025, {}, "wide-dual/signal/ragged", ()),
    ("L3600-N1280", 768, 6, 3600, 1280, {}, "wide-dual/signal", ()),
    ("L3600-N1281-nb5", 768, 5, 3600, 1281, {}, "dual/events/chunk-slabs/single-tail/ragged", (1023, 1024, 1280)),
    ("L1245-N700", 768, 6, 1245, 700, {}, "dual/serial/ragged/no-overlap", ()),
    ("L1250-N700", 768, 6, 1250, 700, {}, "dual/signal/ragged", (511, 512, 699)),
    ("L15-N65", 768, 6, 15, 65, {}, "single/serial/ragged/no-overlap", ()),
    ("L10-N65", 768, 6, 10, 65, {}, "single/serial/ragged/no-overlap", ()),
    ("L5-N65", 768, 6, 5, 65, {}, "single/serial/ragged/no-overlap", ()),
    ("L1000-N4161", 768, 6, 1000, 4161, {}, "dual/serial/chunk-slabs/single-tail/ragged/local-groups", (4095, 4096, 4160)),
    ("L4000-N600-signal", 768, 6, 4000, 600, {"XB_LSTM_SIGNAL": "1"}, "wide/signal/uneven/ragged", ()),
    ("L4000-N641-events", 768, 6, 4000, 641, {"XB_LSTM_SIGNAL": "0"}, "dual/events/uneven/ragged", ()),
    ("L3600-N512-64slabs", 768, 6, 3600, 512, {"XB_TIME_SLABS": "64", "XB_SLAB_STEPS": "8", "XB_LSTM_SIGNAL": "1"},
     "single/signal/uneven/signal-limit", ()),
    ("L3600-N512-80slabs", 768, 6, 3600, 512, {"XB_TIME_SLABS": "80", "XB_SLAB_STEPS": "8", "XB_LSTM_SIGNAL": "1"},
     "single/events/mask-ends", ()),
    ("L4000-N513-nowide", 768, 6, 4000, 513, {"XB_LSTM_WIDE": "0"}, "dual/signal/uneven/ragged", ()),
    ("L4000-N700-nolocal", 768, 6, 4000, 700, {"XB_LSTM_LOCAL": "0"}, "dual/signal/uneven/ragged/write-through", ()),
    ("L4000-N641-overlap2", 768, 6, 4000, 641, {"XB_OVERLAP": "2"}, "dual/slabs-serial-gemm/uneven/ragged", ()),
    ("L4000-N100-spread", 768, 6, 4000, 100, {"XB_LSTM_SPREAD": "1"}, "single/spread/events/uneven/ragged", ()),
    ("F384-L3600-N1100", 384, 6, 3600, 1100, {}, "wide/events/ragged", (1023, 1024, 1099)),
    ("F384-L3600-N1345", 384, 6, 3600, 1345, {}, "dual/signal/ragged", ()),
    # the same two-groups-per-workgroup shape with the write-through exchange, with event-ordered slabs, and with every
    # workgroup slot of the launch in use (g8 = gh = 16: no workgroup leaves at the top, two slots on every XCD)
    ("F384-L3600-N1345-nolocal", 384, 6, 3600, 1345, {"XB_LSTM_LOCAL": "0"}, "dual/signal/ragged/write-through", ()),
    ("F384-L3600-N1345-events", 384, 6, 3600, 1345, {"XB_LSTM_SIGNAL": "0"}, "dual/events/ragged", ()),
    ("F384-L3600-N2000", 384, 6, 3600, 2000, {}, "dual/signal/ragged", (1999,)),
    # the reference order itself, so that every label plan() can return is in the table
    ("L10-N65-per-step", 768, 6, 10, 65, REFERENCE_ENV, "per-step", ()),
]

# Pairing rows (xb_reserve_pairing): id, features, nb, L, max_batch, the batch of every call, and the label of each pass
# on 256 CUs -- two calls in flight run as one pass, a lone last call runs on its own at the synchronize.
PAIR_ROWS = [
    ("pair-2x384-L3600", 768, 6, 3600, 384, (384, 384), ("dual/signal",)),
    ("pair-2x300-L4000", 768, 6, 4000, 300, (300, 300), ("wide/events/uneven/ragged",)),
    ("pair-320+320+77-L4000", 768, 6, 4000, 320, (320, 320, 77), ("wide/events/uneven", "single/events/uneven/ragged")),
]


def pair_passes(calls):
    """Batches of the encoder passes the pairing makes of consecutive calls (two at a time, a lone last call alone)."""
    return [sum(calls[i:i + 2]) for i in range(0, len(calls), 2)]
