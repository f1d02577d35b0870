// The encoder's host scheduler (csrc/xb_schedule.h), the weight packer (csrc/xb_pack.h) and the decoder of the device status
// words (csrc/xb_status.h) on their own, for a sanitizer run without a GPU and without Python:
//
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/host_logic_main.cpp -o /tmp/host_logic && /tmp/host_logic
//
// The planner walks the grid of tests/test_schedule_host.py (every feature size, CU count, step count, the batch seams, the
// device facts on and off, the knob sets) and every launch of every plan is checked to lie inside the batch, the steps and
// the 64 group slots.  The packer runs on exact-size heap blocks, so a read past a tensor or a write past an image is an
// error the sanitizer reports.  The status decoder walks the eight cases of tests/test_status_host.py.  Exit status 0 and
// "ok" when nothing failed.
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../xna_basecaller_amd/csrc/xb_pack.h"
#include "../xna_basecaller_amd/csrc/xb_schedule.h"
#include "../xna_basecaller_amd/csrc/xb_status.h"

static long failures = 0, plans = 0, launches = 0;

#define CHECK(cond)                                                         \
    do {                                                                    \
        if (!(cond)) {                                                      \
            if (failures < 20) printf("FAILED line %d: %s\n", __LINE__, #cond); \
            ++failures;                                                     \
        }                                                                   \
    } while (0)

static void check_plan(const xb::PlanQuery &q)
{
    const xb::LayerPlan p = xb::plan_layer(q);
    ++plans;
    if (p.error) {
        CHECK(p.error == xb::PLAN_ERR_INVALID && strlen(p.message) > 0 && strlen(p.message) < sizeof p.message);
        return;
    }
    CHECK(p.mode == 1 || p.mode == 2);
    if (p.mode == 1 || p.ordering == xb::PLAN_SIGNAL) {
        const xb::PlanLaunch l = p.launch(0, 0);
        ++launches;
        CHECK(l.n0 == 0 && l.nslab == q.n && l.s_begin == 0 && l.s_end == q.T && l.grp0 == 0 && l.sync_base == 0);
        CHECK(p.rec_launches == (p.mode == 1 ? q.T : 1));
        if (p.mode == 2) CHECK(q.n <= p.slab && p.nts <= 64 && (l.nslab + 63) / 64 <= (l.dual ? 2 : 1) * p.gslab);
    } else {
        CHECK(p.rec_launches == p.nts * p.chunk_slabs);
        unsigned arrivals = 0;
        for (int i = 0; i < p.nts; ++i) {
            int covered = 0;
            for (int j = 0; j < p.chunk_slabs; ++j) {
                const xb::PlanLaunch l = p.launch(i, j);
                ++launches;
                CHECK(l.n0 == covered && l.nslab >= 1 && l.nslab <= p.slab);
                CHECK(l.s_begin == p.step0(i) && l.s_end == p.step0(i + 1) && l.s_begin < l.s_end);
                const int groups = (l.nslab + 63) / 64;
                CHECK(groups <= (l.dual ? 2 : 1) * p.gslab && groups <= 64);
                CHECK(p.global_groups ? (l.grp0 == l.n0 / 64 && l.grp0 + groups <= 64 && l.sync_base == arrivals)
                                      : (l.grp0 == 0 && l.sync_base == 0));
                CHECK(l.slab == i && (!l.xcd_local || i < 16));
                covered += l.nslab;
            }
            CHECK(covered == q.n);
            arrivals += (unsigned)(p.step0(i + 1) - p.step0(i) - 1);
        }
        CHECK(p.step0(0) == 0 && p.step0(p.nts) == q.T);
    }
    // the GEMM's rows: the slabs of either direction partition [0, T)
    for (int rev = 0; rev < 2; ++rev) {
        int rows = 0;
        for (int i = 0; i < p.nts; ++i) {
            int ta, tb;
            p.gemm_rows(i, rev != 0, &ta, &tb);
            CHECK(0 <= ta && ta < tb && tb <= q.T);
            rows += tb - ta;
        }
        CHECK(rows == q.T);
    }
}

static void walk_plans()
{
    const int Fs[] = {32, 64, 96, 128, 256, 384, 512, 768}, cus[] = {64, 192, 256, 304};
    const int Ts[] = {1, 2, 124, 125, 128, 136, 249, 250, 512, 520, 720, 800};
    struct Env { int mode, dual, wide, local, signal, overlap, slabs, steps, spread; };
    const Env envs[] = {{0, 1, 1, 1, 2, 1, 16, 0, 0}, {0, 1, 1, 1, 1, 1, 16, 0, 0}, {0, 1, 1, 1, 0, 1, 16, 0, 0},
                        {0, 1, 1, 1, 1, 1, 64, 8, 0}, {0, 1, 1, 1, 1, 1, 80, 8, 0}, {0, 1, 0, 1, 2, 1, 16, 0, 0},
                        {0, 1, 1, 0, 2, 1, 16, 0, 0}, {0, 1, 1, 1, 2, 2, 16, 0, 0}, {0, 1, 1, 1, 2, 0, 16, 0, 0},
                        {0, 1, 1, 1, 2, 1, 16, 0, 1}, {0, 0, 1, 1, 2, 1, 16, 0, 0}, {0, 2, 1, 1, 2, 1, 16, 0, 0},
                        {1, 0, 0, 1, 2, 0, 16, 0, 0}, {1, 2, 1, 1, 2, 1, 16, 0, 0}, {2, 1, 1, 1, 2, 1, 16, 0, 0}};
    for (int F : Fs)
        for (int cu : cus) {
            const int members = xb::lstm_members(F), gmax = 8 * ((cu / 8) / members), gslab0 = gmax > 64 ? 64 : gmax;
            const int slots = cu / members > 64 ? 64 : cu / members;
            std::vector<int> ns = {1, 63, 64, 65, 4095, 4096, 4097, 4161};
            for (int k : {gslab0, slots, 2 * gslab0, 2 * slots})
                for (int d = -1; d <= 1; ++d)
                    if (k * 64 + d >= 1) ns.push_back(k * 64 + d);
            for (int n : ns)
                for (int T : Ts)
                    for (const Env &e : envs)
                        for (int facts = 0; facts < 8; ++facts) {
                            xb::PlanQuery q{};
                            q.F = F; q.n = n; q.T = T; q.cu_count = cu;
                            q.knobs.lstm_mode = e.mode; q.knobs.lstm_dual = e.dual; q.knobs.lstm_wide = e.wide;
                            q.knobs.lstm_local = e.local; q.knobs.lstm_signal = e.signal; q.knobs.overlap = e.overlap;
                            q.knobs.time_slabs = e.slabs; q.knobs.slab_steps = e.steps;
                            q.spread = e.spread; q.has_next = 1;
                            q.resident1 = facts & 1; q.resident2 = (facts >> 1) & 1; q.signal_ok = (facts >> 2) & 1;
                            check_plan(q);
                        }
        }
    CHECK(xb::pair_capacity(768, 256, 1) == 640 && xb::pair_capacity(768, 256, 0) == 512);
    CHECK(xb::pair_capacity(384, 256, 1) == 512 && xb::pair_capacity(768, 192, 1) == 512);
    const xb::Knobs k = xb::knobs_from_env();
    CHECK(k.time_slabs >= 1 && k.lstm_signal >= 0 && k.lstm_signal <= 2);
}

// an exact-size heap copy of a tensor (no slack behind it)
static float *heap(const std::vector<float> &v)
{
    float *p = static_cast<float *>(malloc(sizeof(float) * v.size()));
    memcpy(p, v.data(), sizeof(float) * v.size());
    return p;
}

static void walk_packer()
{
    unsigned s = 12345u;
    auto rnd = [&]() { s = s * 1664525u + 1013904223u; return ((int)(s >> 8) % 20001 - 10000) * 1e-4f; };
    const int shapes[][3] = {{3, 40, 64}, {5, 304, 320}, {33, 32, 32}, {256, 64, 64}};
    for (auto &sh : shapes) {
        const int rows = sh[0], cols = sh[1], ld = sh[2];
        std::vector<float> w((size_t)rows * cols);
        for (float &x : w) x = rnd();
        w[0] = 0.0f; w[1] = -0.0f; w[2] = 3e-5f; w[3] = 448.0f; w[4] = -1e30f;
        float *src = heap(w);
        for (int q8 = 0; q8 < 2; ++q8) {
            std::vector<xb::half_t> hi, lo;
            int e = 99;
            xb::split_rows(src, rows, cols, ld, hi, lo, q8 ? &e : nullptr);
            CHECK(hi.size() == (size_t)rows * ld && lo.size() == hi.size() && (!q8 || (e >= -16 && e <= 32)));
            for (int nsplit = 1; nsplit <= 3; ++nsplit) {
                if ((nsplit == 2) != (q8 == 1) && nsplit != 1) continue;
                std::vector<unsigned char> f4;
                size_t ks = 0;
                xb::fragment_major(hi, lo, rows, ld, ld, nsplit, f4, &ks);
                CHECK(ks == (size_t)((rows + 255) / 256 * 8) * xb::gemm4_pieces(nsplit) * 1024 && f4.size() == ks * (ld / 32));
            }
        }
        std::vector<int8_t> d1, d0;
        std::vector<float> sc;
        xb::i8_limbs(src, rows, cols, d1, d0, sc);
        for (size_t i = 0; i < d1.size(); ++i) CHECK(256 * d1[i] + d0[i] >= -32512 && 256 * d1[i] + d0[i] <= 32512);
        free(src);
    }
    for (int F : {32, 96}) {
        std::vector<float> a((size_t)4 * F * F), b((size_t)4 * F * F), c((size_t)4 * F), d((size_t)4 * F);
        for (size_t i = 0; i < a.size(); ++i) { a[i] = (float)i; b[i] = -(float)i; }
        for (size_t i = 0; i < c.size(); ++i) { c[i] = (float)i; d[i] = 0.5f; }
        float *pa = heap(a), *pb = heap(b), *pc = heap(c), *pd = heap(d);
        std::vector<float> wi, wh, bb;
        xb::gate_interleave(pa, pb, pc, pd, F, wi, wh, bb);
        for (int u = 0; u < F; ++u)
            for (int g = 0; g < 4; ++g) {
                CHECK(wi[((size_t)u * 4 + g) * F + 1] == a[((size_t)g * F + u) * F + 1] && wh[((size_t)u * 4 + g) * F] == b[((size_t)g * F + u) * F]);
                CHECK(bb[(size_t)u * 4 + g] == c[(size_t)g * F + u] + 0.5f);
            }
        free(pa); free(pb); free(pc); free(pd);
    }
    // every e4m3 code but the two NaNs is the encoding of its own value
    for (int code = 0; code < 256; ++code) {
        const int e = (code >> 3) & 15, m = code & 7;
        if ((code & 0x7f) == 0x7f) continue;
        const float v = (e == 0 ? ldexpf((float)m, -9) : ldexpf((float)(8 + m), e - 10)) * ((code & 0x80) ? -1.0f : 1.0f);
        CHECK(xb::f32_to_e4m3(v) == code);
    }
}

// the two device status words: sync word {0, 1} x data word {0, 2, 4, 6}, as tests/test_status_host.py states them
static void walk_status()
{
    const char *sync_text = "LSTM inter-workgroup sync timed out (persistent kernel was not fully resident?)";
    const char *loss_text = "xb_ctc_loss: a target length outside [state_len, Lt] or a label above n_base inside it";
    const char *scan_text = "CTC scan: a target length was outside the lattice";
    for (unsigned sync = 0; sync <= 1; ++sync)
        for (unsigned data = 0; data <= 6; data += 2) {
            const xb::DeviceStatus s = xb::decode_status(sync, data);
            const char *text = sync ? sync_text : ((data & 4) ? loss_text : (data ? scan_text : nullptr));
            const int code = sync ? XB_ERR_DEVICE : ((data & 4) ? XB_ERR_INVALID : (data ? XB_ERR_DEVICE : XB_OK));
            CHECK(s.code == code && (text ? (s.message && strcmp(s.message, text) == 0) : s.message == nullptr));
            // a report takes one condition out of the words and leaves the others for the next one
            CHECK(s.sync_left == 0 && s.data_left == (sync ? data : ((data & 4) ? (data & ~4u) : 0u)));
        }
    CHECK(xb::SYNC_LOST == 1u && xb::DATA_SCAN_LENGTH == 2u && xb::DATA_LOSS_LABEL == 4u);
}

int main()
{
    walk_plans();
    walk_packer();
    walk_status();
    printf("%ld plans, %ld launches checked\n", plans, launches);
    if (failures) printf("%ld check(s) failed\n", failures);
    else printf("ok\n");
    return failures ? 1 : 0;
}
