// xb_schedule.h -- the encoder's host scheduler as plain arithmetic: the environment knobs of a context (Knobs,
// knobs_from_env), the plan of one LSTM layer's recurrence and of the GEMM that consumes it (plan_layer), and the batch up to
// which two calls pair (pair_capacity).  No HIP: xb_run_encoder.hip executes the plans, tools/host_logic_main.cpp and
// tests/test_schedule_host.py check them without a GPU.  Also the one definition of the recurrence's group geometry, which
// xb_lstm.hip includes.
#pragma once
#include <cstdio>
#include <cstdlib>

namespace xb {

constexpr int LG_BN = 64;        // chunks per group (2 MFMA column tiles)
constexpr int LG_UNITS = 32;     // hidden units per member workgroup
// members (workgroups per group) and chunks per group of the LSTM kernel for feature size F
inline int lstm_members(int F) { return F / LG_UNITS; }
inline int lstm_group_chunks() { return LG_BN; }

// Every environment knob a context reads, with the library's defaults (xb_ctx_create: knobs_from_env once, then the
// device-dependent demotions of lstm_signal).  All ints, so that the struct is its own C form.
struct Knobs {
    int lstm_mode = 0;           // XB_LSTM_MODE (over xb_config.lstm_mode): 0 auto, 1 one launch per step, 2 persistent
    int lstm_dual = 1;           // XB_LSTM_DUAL: 0 never, 1 when a launch would otherwise need a second chunk slab, 2 always
    int lstm_wide = 1;           // XB_LSTM_WIDE: 1 (default) batches just above a launch's XCD-local capacity get up to cu_count / members group
                                 // slots with the groups dealt over all XCDs instead of a second round (plan_layer); 0: never
    int lstm_local = 1;          // XB_LSTM_LOCAL=0: always exchange h with write-through stores (A/B)
    // one recurrence launch per layer that reports its time slabs to the GEMM stream (default on where hipStreamWaitValue32 is
    // supported)
    int lstm_signal = 2;         // XB_LSTM_SIGNAL: 0 off, 1 whenever one launch holds the batch, 2 (default) only above 512 chunks (two groups per workgroup)
    int lstm_i8 = 0;             // XB_LSTM_I8 (with precision f16f8 / f16f8i): recurrence on int8 digits; 1 = all four digit
                                 // products, 2 = without d0 x d0
    int overlap = 1;             // XB_OVERLAP: 0 serial, 1 overlapped, 2 time slabs but serial GEMM (A/B)
    int time_slabs = 16;         // XB_TIME_SLABS (upper bound; a slab is at least 125 steps)
    int slab_steps = 0;          // XB_SLAB_STEPS: minimum steps per time slab (default 125)
    int fuse = 1;                // XB_FUSE=0: this context never pairs two calls
    int decode_async = 0;        // XB_DECODE_ASYNC=1: the decode of a batch runs on the third stream beside the next batch's conv + first
                                 // GEMM (rounds 2-3) instead of on the main stream with the chip to itself (round 4 default: the same step
                                 // time at every batch size -- the step is bound by the kernels' summed CU-time -- and the decode at 0.49-0.52
                                 // of the HBM roofline instead of 0.35-0.42: profiles/r04_decode_placement.txt)
    int in1_layers = 31;         // XB_IN1_LAYERS (diagnostic): layers whose input projection XB_PREC_F16F8_IN1 reduces
    int x3_stages = -1;          // XB_X3_STAGES (diagnostic, tools/x3_stages.py): stage mask of the three-product arithmetic; -1 = the precision's own
    int gemm4 = 1;               // XB_GEMM4=0: gemm8r_kernel (one workgroup per CU) instead of gemm4p_kernel (A/B comparisons)
    int gemm_sn = 0;             // XB_GEMM_SN: N tiles per XCD super-tile of gemm4p_kernel (0 = gemm_super_n's rule; experiments)
    int gemm_shadow_kernel = 0;  // XB_GEMM_SHADOW: 0 auto (by batch size), 4 gemm4p_kernel, 8 gemm8r_kernel for the slabs beside the recurrence
    int gemm_shadow_wgs = 2;     // XB_GEMM_SHADOW_WGS=1: GEMM slabs beside the recurrence run one workgroup per CU
};

// `k` with every knob the environment sets, clamped
inline Knobs knobs_from_env(Knobs k = Knobs())
{
    if (const char *e = getenv("XB_X3_STAGES")) k.x3_stages = (int)strtol(e, nullptr, 0) & 0xfff;
    if (const char *e = getenv("XB_LSTM_MODE")) k.lstm_mode = atoi(e);
    if (const char *e = getenv("XB_LSTM_DUAL")) k.lstm_dual = atoi(e);
    if (const char *e = getenv("XB_LSTM_WIDE")) k.lstm_wide = atoi(e) != 0;
    if (const char *e = getenv("XB_LSTM_LOCAL")) k.lstm_local = atoi(e) != 0;
    if (const char *e = getenv("XB_DECODE_ASYNC")) k.decode_async = atoi(e) != 0;
    if (const char *e = getenv("XB_IN1_LAYERS")) k.in1_layers = atoi(e) & 31;
    if (const char *e = getenv("XB_LSTM_I8")) k.lstm_i8 = atoi(e) == 2 ? 2 : (atoi(e) != 0);
    if (const char *e = getenv("XB_GEMM4")) k.gemm4 = atoi(e) != 0;
    if (const char *e = getenv("XB_GEMM_SN")) k.gemm_sn = atoi(e) > 0 && atoi(e) <= 64 ? atoi(e) : 0;
    if (const char *e = getenv("XB_GEMM_SHADOW_WGS")) k.gemm_shadow_wgs = atoi(e) == 1 ? 1 : 2;
    if (const char *e = getenv("XB_GEMM_SHADOW")) k.gemm_shadow_kernel = atoi(e) == 4 ? 4 : (atoi(e) == 8 ? 8 : 0);
    if (const char *e = getenv("XB_OVERLAP")) k.overlap = atoi(e);
    if (const char *e = getenv("XB_TIME_SLABS")) k.time_slabs = atoi(e) > 0 ? atoi(e) : 1;
    if (const char *e = getenv("XB_SLAB_STEPS")) k.slab_steps = atoi(e) >= 8 ? atoi(e) : 0;
    if (const char *e = getenv("XB_LSTM_SIGNAL")) k.lstm_signal = atoi(e) < 0 || atoi(e) > 2 ? 2 : atoi(e);
    if (const char *e = getenv("XB_FUSE")) k.fuse = atoi(e) != 0;
    return k;
}

// a profiler is collecting hardware counters in this process (rocprofv3 --pmc announces itself in the environment)
inline bool counter_collection_from_env()
{
    const char *cc = getenv("ROCPROF_COUNTER_COLLECTION"), *cn = getenv("ROCPROF_COUNTERS");
    return (cc && atoi(cc) != 0) || (cn && *cn);
}

// What plan_layer is asked: one layer's recurrence over n chunks of T steps on cu_count CUs.
struct PlanQuery {
    int F, n, T, cu_count;
    Knobs knobs;
    int spread;                  // XB_LSTM_SPREAD (read per call): deal every group's members over all XCDs
    int has_next;                // a GEMM consumes this layer's output (the next input projection, or the CRF linear layer)
    // the device's part: the occupancy query admits the persistent kernel with one / two groups per workgroup, and the
    // flag word of the signal-ordered slabs exists (hipStreamWaitValue32 is supported)
    int resident1, resident2, signal_ok;
};

// the order between a layer's recurrence and the GEMM that consumes it
enum PlanOrdering {
    PLAN_SERIAL = 0,             // one time slab; the GEMM follows the layer on the main stream
    PLAN_EVENTS = 1,             // a launch per time slab; the slab's GEMM waits on the second stream for an event behind it
    PLAN_SIGNAL = 2,             // ONE launch that reports its time slabs; the slab's GEMM waits for the flag word
    PLAN_SLABS_SERIAL_GEMM = 3,  // XB_OVERLAP=2: the launches of PLAN_EVENTS, the GEMM of PLAN_SERIAL
};

constexpr int PLAN_ERR_INVALID = -1;     // = XB_ERR_INVALID

// one launch of the recurrence, as LstmParams names it
struct PlanLaunch {
    int n0, nslab, s_begin, s_end, dual, grp0, slab, xcd_local;
    unsigned sync_base;
};

struct LayerPlan {
    int error = 0;               // 0, or the status the entry point returns with `message`
    char message[160] = {};
    int mode = 0;                // 1 one launch per time step, 2 persistent launches
    int wide = 0;                // the group slots are dealt over all XCDs (beyond the XCD-local capacity)
    int spread = 0;              // LstmParams.spread of every launch: wide, or asked for
    int dual_batch = 0;          // the batch runs two groups per workgroup (a tail chunk slab may still run one)
    int gslab = 0;               // group slots of a launch with one group per workgroup
    int slab = 0;                // chunks per launch
    int global_groups = 0;       // the batch fits the 64 group slots: every group keeps its slot and its counters for the layer
    int nts = 1;                 // time slabs
    int chunk_slabs = 1;
    int ordering = PLAN_SERIAL;
    int rec_launches = 0;        // recurrence launches of the layer
    int gemm_slabs = 0;          // launches of the consuming GEMM
    int n = 0, T = 0, lstm_dual = 0, dual_ok = 0, lstm_local = 0;     // what launch() still needs of the query

    int step0(int i) const { return (int)((long long)T * i / nts); }
    // two groups per workgroup for a launch of m chunks
    bool dual_for(int m) const { return dual_ok && (lstm_dual == 2 ? m > LG_BN : m > gslab * LG_BN); }

    // The launch of time slab i and chunk slab j.  PLAN_SIGNAL has the one launch (0, 0) over all steps; mode 1 as well, which
    // is then issued step by step.
    PlanLaunch launch(int i, int j) const
    {
        PlanLaunch l{};
        if (mode != 2) {
            l.nslab = n; l.s_end = T;
            l.dual = dual_ok && lstm_dual == 2 && n > LG_BN;       // tests only: the per-step variant of the dual kernel
            return l;
        }
        if (ordering == PLAN_SIGNAL) {
            l.nslab = n; l.s_end = T;
            l.dual = dual_batch;
            l.xcd_local = lstm_local;
            return l;
        }
        l.n0 = j * slab; l.nslab = (n - l.n0) < slab ? (n - l.n0) : slab;
        l.s_begin = step0(i); l.s_end = step0(i + 1);
        // a tail slab that fits the single-group launch gets one workgroup per group (twice the CUs at work)
        l.dual = dual_batch && dual_for(l.nslab);
        // counters are zeroed once per layer: consecutive launches follow each other without a memset in between, so the next
        // launch's workgroups are dispatched the moment the previous one retires
        l.grp0 = global_groups ? l.n0 / LG_BN : 0;
        l.slab = i; l.xcd_local = lstm_local && i < 16;       // 16 mask bytes per group slot
        // arrivals per member and group so far in this layer (a launch of k steps arrives k - 1 times)
        l.sync_base = global_groups ? (unsigned)(step0(i) - i) : 0u;
        return l;
    }
    // the rows [ta, tb) of time steps that time slab i of a layer running in direction `reverse` has produced
    void gemm_rows(int i, bool reverse, int *ta, int *tb) const
    {
        const int s0 = step0(i), s1 = step0(i + 1);
        *ta = reverse ? T - s1 : s0;
        *tb = reverse ? T - s0 : s1;
    }
};

inline LayerPlan plan_layer(const PlanQuery &q)
{
    const Knobs &k = q.knobs;
    const int members = lstm_members(q.F), bn = lstm_group_chunks(), n = q.n, T = q.T;
    LayerPlan p;
    p.n = n; p.T = T; p.lstm_dual = k.lstm_dual; p.lstm_local = k.lstm_local; p.spread = q.spread != 0;
    // groups per persistent launch: every workgroup must be resident at once, and workgroups are dealt to the 8 XCDs
    // strictly round-robin (block b -> XCD b % 8), i.e. groups g, g + 8, .. share ONE XCD's CUs: F = 768 (24 members per
    // group, 32 CUs per XCD) allows one group per XCD = 8 groups = 512 chunks per launch
    // ... and the occupancy calculator has to admit at least one such workgroup per CU; a context that cannot keep the
    // persistent kernel resident falls back to one launch per time step
    p.dual_ok = k.lstm_dual != 0 && q.resident2;
    const int gmax = q.resident1 ? 8 * ((q.cu_count / 8) / members) : 0;
    p.mode = k.lstm_mode;
    if (p.mode == 0) p.mode = gmax >= 1 ? 2 : 1;
    if (p.mode == 2 && gmax < 1) {
        p.error = PLAN_ERR_INVALID;
        snprintf(p.message, sizeof p.message, "persistent LSTM needs %d co-resident workgroups, device has %d CUs", members, q.cu_count);
        return p;
    }
    if (p.mode != 2) {
        if (n > 64 * bn) {
            p.error = PLAN_ERR_INVALID;
            snprintf(p.message, sizeof p.message, "one-launch-per-step LSTM mode handles at most %d chunks per batch", 64 * bn);
            return p;
        }
        p.rec_launches = T;
        p.gemm_slabs = q.has_next ? 1 : 0;
        return p;
    }
    // a workgroup can serve two groups alternately (lstm_kernel DUAL): a launch then holds 2 * gmax groups, and a
    // group's hand-off latency is covered by the other group's step.  Used when the batch does not fit gmax groups.
    // WIDE (round 5, the batch cliffs): the XCD-local placement holds gmax = 8 group slots (one group's 24 member workgroups per
    // XCD), so 513 chunks -- nine groups -- used to take the two-groups-per-workgroup kernel over five slots, i.e. the time of
    // 1024 chunks, and 1025 chunks a second launch.  The device has cu_count / members = 10 slots' worth of CUs: with a
    // group's members dealt over ALL XCDs (LstmParams.spread: 3 per XCD and group, 30 of an XCD's 32 CUs at ten slots; the
    // exchange then goes through write-through stores, a few percent slower per step) a launch holds up to 640 chunks with
    // one group per workgroup and 1280 with two.  Used exactly where it saves a round: 513..640 and 1025..1280 chunks.
    const int gslab0 = gmax > 64 ? 64 : gmax;
    const int gwide = k.lstm_wide && q.cu_count / members > gslab0 ? (q.cu_count / members > 64 ? 64 : q.cu_count / members) : gslab0;
    p.wide = gwide > gslab0 && ((n > gslab0 * bn && n <= gwide * bn) ||
                                (p.dual_ok && k.lstm_dual == 1 && n > 2 * gslab0 * bn && n <= 2 * gwide * bn));
    p.gslab = p.wide ? gwide : gslab0;
    if (p.wide) p.spread = 1;
    p.dual_batch = p.dual_for(n);
    p.slab = (p.dual_batch ? (2 * p.gslab > 64 ? 64 : 2 * p.gslab) : p.gslab) * bn;
    p.chunk_slabs = (n + p.slab - 1) / p.slab;
    // the exchange buffer and the counters have 64 group slots: with the whole batch inside them every group keeps its
    // own slot across launches, so chunk slabs and time slabs combine freely; a larger batch falls back to one launch
    // per chunk slab over all steps with launch-local slots
    p.global_groups = n <= 64 * bn;
    const int min_steps = k.slab_steps > 0 ? k.slab_steps : 125;
    p.nts = T / min_steps < k.time_slabs ? T / min_steps : k.time_slabs;
    const bool overlapped = q.has_next && k.overlap && p.global_groups && p.nts >= 2;
    if (!overlapped) p.nts = 1;
    // One launch over all steps that reports its time slabs: the GEMM stream waits on the flag word instead of on an event
    // behind a slab launch, so the recurrence is not relaunched 16 times per layer (each relaunch costs ~30 us: its
    // workgroups find their CUs taken by GEMM workgroups that slipped in at the boundary).
    // Measured (profiles/r03_lstm_slab_signal.txt): the recurrence itself gets 13 % faster (98 -> 85 ms per step at batch 512,
    // 187 -> 152 ms at 1024), but at batch 512 the GEMM then gets that much less of the chip and the step stays where it was
    // (120.5 vs 121.2 ms); with two groups per workgroup (batch 1024) the step gains 2 %.  Default: only there.
    const bool signal_mode = k.lstm_signal == 1 || (k.lstm_signal == 2 && p.dual_batch);
    if (!overlapped) p.ordering = PLAN_SERIAL;
    else if (k.overlap != 1) p.ordering = PLAN_SLABS_SERIAL_GEMM;
    else if (signal_mode && q.signal_ok && n <= p.slab && p.nts <= 64) p.ordering = PLAN_SIGNAL;
    else p.ordering = PLAN_EVENTS;
    p.rec_launches = p.ordering == PLAN_SIGNAL ? 1 : p.nts * p.chunk_slabs;
    p.gemm_slabs = !q.has_next ? 0 : (p.ordering == PLAN_EVENTS || p.ordering == PLAN_SIGNAL ? p.nts : 1);
    return p;
}

// Co-scheduling two calls: only where the pair fits one launch of two groups per workgroup (512 = the XCD-local capacity of a
// launch at features 768; with the wide placement a pair of up to 2 x 640 chunks still is ONE launch of two groups per
// workgroup, so batch sizes 513..640 pair as well).  The largest max_batch whose contexts pair.
inline int pair_capacity(int F, int cu_count, int lstm_wide)
{
    int pair_cap = 512;
    const int members = lstm_members(F), slots = members > 0 ? cu_count / members : 0;
    if (lstm_wide && members > 0 && 8 * ((cu_count / 8) / members) * lstm_group_chunks() == 512 && slots > 8)
        pair_cap = (slots > 64 ? 64 : slots) * lstm_group_chunks();
    return pair_cap;
}

}  // namespace xb
