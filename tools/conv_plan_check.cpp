// conv_plan_check.cpp -- csrc/xb_conv_plan.h on its own, for a sanitizer run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/conv_plan_check.cpp -o conv_plan_check && ./conv_plan_check
// The six conv tensors follow one another without a gap, the section is 360 + F (16 W + 1) floats and ends on a 16-byte boundary
// whenever F is a multiple of 16, the activations of a step tile their buffer in 16-byte pieces, the route rule puts conv1 and
// conv2 on the narrow route and conv3 on the wide one, and the routes' workspaces hold what their kernels index.
// With arguments (chunk F W S n) it prints the table instead, one number per line, for the Python restatement's test; with
// (Cin Cout K stride) the route (1 narrow, 0 wide).  Exit status 0 when everything holds.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../xna_basecaller_amd/csrc/xb_conv_plan.h"

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static void check(int chunk, int F, int W, int S, size_t n)
{
    const xb::ConvPlan p = xb::conv_plan(chunk, F, W, S);
    CHECK(!p.error);
    if (p.error) return;
    size_t at = 0;
    for (int k = 0; k < xb::CONV_TENSORS; ++k) {
        CHECK(p.off[k] == at && p.len[k] > 0);
        at += p.len[k];
    }
    CHECK(at == p.params && p.params == (size_t)360 + (size_t)F * ((size_t)16 * W + 1));
    if (F % 16 == 0) CHECK(p.params % 4 == 0);
    for (int k = 0; k < xb::CONV_TENSORS; ++k) CHECK(p.off[k] % 4 == 0);          // each tensor starts on a 16-byte boundary
    const int pad = W / 2;
    CHECK(p.L1 == chunk && p.L2 == chunk && p.T == (chunk + 2 * pad - W) / S + 1 && p.T >= 1);
    const xb::ConvAct a = p.act(n);
    std::vector<std::pair<size_t, size_t>> piece = {{a.z1, n * 4 * p.L1}, {a.y1, n * 4 * p.L1}, {a.z2, n * 16 * p.L2}, {a.y2, n * 16 * p.L2},
                                                    {a.col, n * p.T * 16 * W}, {a.z3, n * p.T * F}, {a.dy2, n * 16 * p.L2}, {a.dy1, n * 4 * p.L1}};
    std::sort(piece.begin(), piece.end());
    size_t end = 0;
    for (const auto &pc : piece) {
        CHECK(pc.first == end && pc.first % 4 == 0);
        end = pc.first + xb::conv_round4(pc.second);
    }
    CHECK(end == a.floats);
    // the routes of the three layers, and their workspaces
    CHECK(xb::conv_is_narrow(1, 4, 5, 1) && xb::conv_is_narrow(4, 16, 5, 1));
    CHECK(xb::conv_is_narrow(16, F, W, S) == (S == 1 && F <= 16 && 16 * W <= 64));
    const xb::ConvNarrow c = xb::conv_narrow((int)n, 4, p.L1, 16, 5);
    CHECK(c.tiles == ((size_t)p.L1 + 255) / 256 && c.blocks == c.tiles * n && c.outputs == 336 && c.scratch_doubles == c.blocks * 336);
    const size_t rows = (size_t)p.T * n;
    const xb::ConvWide w = xb::conv_wide(rows, 16 * W, F);
    CHECK(w.dz == 0 && w.col >= rows * F && w.dcol >= w.col + rows * 16 * W && w.wt >= w.dcol + rows * 16 * W && w.forward_floats == w.dcol);
    CHECK(w.backward_floats >= w.wt + (size_t)16 * W * F && w.col % 4 == 0 && w.dcol % 4 == 0 && w.wt % 4 == 0);
}

int main(int argc, char **argv)
{
    if (argc == 6) {
        const xb::ConvPlan p = xb::conv_plan(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4]));
        const size_t n = (size_t)atoll(argv[5]);
        printf("%d\n", p.error);
        if (p.error) return 0;
        const xb::ConvAct a = p.act(n);
        printf("%zu\n%ld\n%ld\n%ld\n%zu\n", p.params, p.L1, p.L2, p.T, a.floats);
        for (int k = 0; k < xb::CONV_TENSORS; ++k) printf("%zu %zu\n", p.off[k], p.len[k]);
        printf("%zu %zu %zu %zu %zu %zu %zu %zu\n", a.z1, a.y1, a.z2, a.y2, a.col, a.z3, a.dy2, a.dy1);
        return 0;
    }
    if (argc == 5) {
        printf("%d\n", xb::conv_is_narrow(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]), atoi(argv[4])) ? 1 : 0);
        return 0;
    }
    for (size_t n : {(size_t)1, (size_t)6, (size_t)17, (size_t)98, (size_t)384}) {
        check(200, 32, 19, 5, n);
        check(1000, 32, 19, 5, n);
        check(3600, 768, 19, 5, n);
        check(4000, 96, 9, 3, n);
        check(23, 48, 19, 5, n);          // a ragged F: pieces are rounded up to 16 bytes
        check(7, 16, 4, 2, n);            // an even window
    }
    CHECK(xb::conv_out_len(23, 19, 5) == 5 && xb::conv_out_len(7, 19, 5) == 2 && xb::conv_out_len(1000, 19, 5) == 200 && xb::conv_out_len(1001, 19, 5) == 201);
    CHECK(xb::conv_out_len(1, 1, 1) == 1 && xb::conv_out_len(1, 4, 7) == 1 && xb::conv_out_len(50, 9, 3) == 17);
    CHECK(!xb::conv_is_narrow(16, 32, 19, 5) && !xb::conv_is_narrow(4, 16, 5, 2) && !xb::conv_is_narrow(4, 17, 5, 1) && !xb::conv_is_narrow(17, 4, 1, 1) &&
          !xb::conv_is_narrow(4, 16, 17, 1) && xb::conv_is_narrow(1, 16, 64, 1) && xb::conv_is_narrow(16, 16, 4, 1));
    CHECK(xb::conv_plan(0, 768, 19, 5).error == 1 && xb::conv_plan(3600, 0, 19, 5).error == 1 && xb::conv_plan(3600, 768, 0, 5).error == 1 &&
          xb::conv_plan(3600, 768, 19, 0).error == 1 && xb::conv_plan(3600, 768, 257, 5).error == 1 && xb::conv_plan(3600, 768, 256, 5).error == 0);
    // the figures of the recipe, batch 98 of 3600 samples: conv2's z is 22.6 MB, a step's conv activations about 0.4 GB
    const xb::ConvPlan r = xb::conv_plan(3600, 768, 19, 5);
    const double z2 = 4.0 * 98 * 16 * (double)r.L2 / 1e6, gb = 4.0 * (double)r.act(98).floats / 1e9;
    CHECK(z2 > 22.5 && z2 < 22.7 && gb > 0.35 && gb < 0.45 && r.params == 360 + (size_t)768 * 305);
    printf(failures ? "%d checks failed\n" : "conv plan: all checks passed\n", failures);
    return failures ? 1 : 0;
}
