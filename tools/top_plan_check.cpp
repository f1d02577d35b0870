// top_plan_check.cpp -- csrc/xb_top_plan.h on its own, for a sanitizer run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/top_plan_check.cpp -o top_plan_check && ./top_plan_check
// The tensors follow one another without a gap or an overlap, the activations of a step tile their buffer exactly, the byte
// count is the closed form T n (L 6F + 9F + 3C) floats plus parameters, for every L at the shapes the tests and the recipe use.
// With arguments (L F C rows) it prints the table instead, one number per line, for the Python restatement's test.
// Exit status 0 when everything holds.
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>
#include <utility>
#include <vector>

#include "../xna_basecaller_amd/csrc/xb_top_plan.h"

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static void check(int L, int F, int C, size_t rows)
{
    const xb::TopPlan p = xb::top_plan(L, F, C);
    CHECK(!p.error);
    if (p.error) return;
    CHECK(p.tensors == 4 * L + 2 && p.bottom_layers() == 5 - L && p.layer_index(L - 1) == 8 && p.layer_index(0) == 9 - L);
    size_t at = 0;
    for (int k = 0; k < p.tensors; ++k) {
        CHECK(p.off[k] == at && p.len[k] > 0);
        at += p.len[k];
    }
    CHECK(at == p.params && p.params == (size_t)L * ((size_t)8 * F * F + (size_t)8 * F) + (size_t)C * F + (size_t)C);
    CHECK(p.stride >= p.params && p.stride < p.params + 4 && p.stride % 4 == 0);
    for (int i = 0; i < L; ++i) CHECK(p.layer(i)[0] == (size_t)i * ((size_t)8 * F * F + (size_t)8 * F) && p.layer(i)[3] + (size_t)4 * F == (i + 1 < L ? p.layer(i + 1)[0] : p.head_w()));
    CHECK(p.head_b() == p.head_w() + (size_t)C * F);
    // the activations: pieces (offset, length) sorted by offset tile [0, act_floats)
    std::vector<std::pair<size_t, size_t>> piece = {{p.x0(rows), rows * F}, {p.gin(rows), rows * 4 * F}, {p.dgin(rows), rows * 4 * F},
                                                    {p.scores(rows), rows * C}, {p.dscores(rows), rows * C}, {p.dz(rows), rows * C}};
    for (int i = 0; i < L; ++i) {
        piece.push_back({p.y(rows, i), rows * F});
        piece.push_back({p.gates(rows, i), rows * 4 * F});
        piece.push_back({p.c(rows, i), rows * F});
    }
    std::sort(piece.begin(), piece.end());
    size_t end = 0;
    for (const auto &pc : piece) {
        CHECK(pc.first == end);
        end = pc.first + pc.second;
    }
    CHECK(end == p.act_floats(rows) && end == rows * ((size_t)L * 6 * F + (size_t)9 * F + (size_t)3 * C));
    CHECK(p.dy(rows) == p.gin(rows));
    CHECK(p.step_bytes(rows) == 4 * (p.act_floats(rows) + 4 * p.stride + p.bias_sum + p.turned));
    CHECK(p.turned >= (size_t)4 * F * F && p.turned >= (size_t)C * F && p.bias_sum == (size_t)L * 4 * F);
}

int main(int argc, char **argv)
{
    if (argc == 5) {
        const xb::TopPlan p = xb::top_plan(atoi(argv[1]), atoi(argv[2]), atoi(argv[3]));
        const size_t rows = (size_t)atoll(argv[4]);
        printf("%d\n", p.error);
        if (p.error) return 0;
        printf("%d\n%zu\n%zu\n%zu\n", p.tensors, p.params, p.stride, p.step_bytes(rows));
        for (int k = 0; k < p.tensors; ++k) printf("%zu %zu\n", p.off[k], p.len[k]);
        return 0;
    }
    for (int L = 1; L <= 5; ++L) {
        for (size_t rows : {(size_t)1, (size_t)15, (size_t)120, (size_t)720 * 98, (size_t)720 * 384}) {
            check(L, 16, 25, rows);
            check(L, 32, 125, rows);
            check(L, 96, 1296, rows);
            check(L, 768, 1296, rows);
            check(L, 768, 625, rows);
        }
    }
    CHECK(xb::top_plan(0, 768, 1296).error == 1 && xb::top_plan(6, 768, 1296).error == 1 && xb::top_plan(2, 0, 5).error == 1 && xb::top_plan(2, 16, 0).error == 1);
    // the figures of the recipe: batch 98, L = 2 about 6 GB; batch 384, L = 5 just under 40 GB
    const double gb98 = (double)xb::top_plan(2, 768, 1296).step_bytes((size_t)720 * 98) / 1e9, gb384 = (double)xb::top_plan(5, 768, 1296).step_bytes((size_t)720 * 384) / 1e9;
    CHECK(gb98 > 5.5 && gb98 < 6.5 && gb384 > 36.0 && gb384 < 40.0);
    printf(failures ? "%d checks failed\n" : "top plan: all checks passed\n", failures);
    return failures ? 1 : 0;
}
