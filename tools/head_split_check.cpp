// head_split_check.cpp -- csrc/xb_head_split.h on its own, for a sanitizer run on the CPU:
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/head_split_check.cpp -o head_split_check && ./head_split_check
// Every slab non-empty, the slabs cover the rows once, the workspace within the bound, for M = 1 .. 4097 at the heads the tests
// use, and the two training shapes; the environment texts of the bound.  Exit status 0 when everything holds.
#include <stdio.h>

#include <initializer_list>

#include "../xna_basecaller_amd/csrc/xb_head_split.h"

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) { ++failures; printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond); } \
    } while (0)

static void check(long M, int O, int F, size_t bound)
{
    const xb::HeadPlan p = xb::head_plan(M, O, F, 256, bound);
    CHECK(!p.error);
    if (p.error) return;
    CHECK(p.nslabs >= 1 && p.nslabs <= p.ksteps);
    CHECK(p.row_begin(0, M) == 0 && p.row_begin(p.nslabs, M) == M);
    for (int s = 0; s < p.nslabs; ++s) CHECK(p.row_begin(s, M) < p.row_begin(s + 1, M));
    CHECK(p.o_tiles_per_launch >= 1 && p.o_tiles_per_launch <= p.o_tiles);
    CHECK((long)p.launches * p.o_tiles_per_launch >= p.o_tiles && (long)(p.launches - 1) * p.o_tiles_per_launch < p.o_tiles);
    CHECK(p.bytes == (size_t)p.o_tiles_per_launch * p.nslabs * p.row_bytes && p.bytes <= bound);
}

int main()
{
    CHECK(xb::head_scratch_bound(nullptr) == (size_t)256 << 20);
    CHECK(xb::head_scratch_bound("0") == (size_t)1 << 20 && xb::head_scratch_bound("-5") == (size_t)1 << 20);
    CHECK(xb::head_scratch_bound("junk") == (size_t)1 << 20 && xb::head_scratch_bound("99999999") == (size_t)65536 << 20);
    const int heads[][2] = {{64, 32}, {125, 96}, {1296, 384}, {1296, 768}, {25, 32}, {1024 * 6, 768}};
    for (const auto &h : heads)
        for (long M = 1; M <= 4097; ++M)
            for (size_t bound : {(size_t)1 << 20, (size_t)256 << 20}) check(M, h[0], h[1], bound);
    for (long M : {720L * 64, 720L * 384, (long)1 << 33})
        for (size_t bound : {(size_t)1 << 20, (size_t)256 << 20}) check(M, 1296, 768, bound);
    CHECK(xb::head_plan(100, 64, 1 << 20, 256, (size_t)1 << 20).error == 1);      // one block of rows alone exceeds the bound
    printf(failures ? "%d checks failed\n" : "head split plan: all checks passed\n", failures);
    return failures ? 1 : 0;
}
