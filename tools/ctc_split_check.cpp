// How xb_ctc_loss_grad divides a call over launches (csrc/xb_ctc_split.h) on its own, for a sanitizer run without a GPU and
// without Python:
//
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ctc_split_check.cpp -o /tmp/ctc_split && /tmp/ctc_split
//
// The launches of a call are walked as ctc_grad_run walks them, against a stash allocated at exactly the size it grows the
// context's to: every chunk's slot is written end to end, so a slot past the allocation is an error the sanitizer reports.
// Exit status 0 and "ok" when every case gives the split it should.
#include <stdio.h>
#include <string.h>

#include <vector>

#include "../xna_basecaller_amd/csrc/xb_ctc_split.h"

static int failures = 0;

// chunks per launch and launches for a call; the stash is touched slot by slot
static void split(const char *what, int T, int positions, int n, const char *env, size_t want_per, size_t want_launches, size_t scale = 1)
{
    const size_t bound = xb::ctc_scratch_bound(env);
    const size_t per = xb::ctc_grad_chunks_per_launch(T, positions, n, bound);
    const size_t slot = xb::ctc_grad_slot_floats(T, positions);
    size_t launches = 0, served = 0;
    {
        // a byte stands for `scale` floats, so that the widest cases stay small on the host
        std::vector<unsigned char> stash(per * slot / scale);
        for (size_t first = 0; first < (size_t)n; first += per, ++launches) {
            const size_t count = per < (size_t)n - first ? per : (size_t)n - first;
            for (size_t i = 0; i < count; ++i) memset(stash.data() + i * (slot / scale), 1, slot / scale);
            served += count;
        }
    }
    const bool fits = per == 1 || per * slot * sizeof(float) <= bound;
    const bool ok = per == want_per && launches == want_launches && served == (size_t)n && per >= 1 && per <= (size_t)n && fits;
    printf("%-58s %s: %zu per launch, %zu launches\n", what, ok ? "ok" : "FAILED", per, launches);
    failures += !ok;
}

int main()
{
    // 311 x 298 floats = 370 KB a chunk: two fit a megabyte
    split("5 chunks of 298 positions, T 310, 1 MB", 310, 298, 5, "1", 2, 3);
    split("... the default bound holds them all", 310, 298, 5, nullptr, 5, 1);
    // the training shape: 721 x 478 floats = 1.38 MB a chunk, 384 chunks = 529 MB
    split("384 chunks of 478 positions, T 720, default", 720, 478, 384, nullptr, 384, 1, 64);
    split("... 256 MB", 720, 478, 384, "256", 194, 2, 64);
    // a chunk larger than the bound still runs, alone
    split("2 chunks of 2048 positions, T 2052, 1 MB", 2052, 2048, 2, "1", 1, 2, 64);
    split("one chunk, one position, one step", 1, 1, 1, "1", 1, 1);
    // the bound's clamps: nonsense and zero read as 1 MB, the ceiling is 65536 MB
    split("XB_CTC_SCRATCH_MB=0", 310, 298, 5, "0", 2, 3);
    split("XB_CTC_SCRATCH_MB=-3", 310, 298, 5, "-3", 2, 3);
    split("XB_CTC_SCRATCH_MB=abc", 310, 298, 5, "abc", 2, 3);
    if (xb::ctc_scratch_bound("99999999") != (size_t)65536 << 20) { printf("the ceiling FAILED\n"); ++failures; }
    // the largest call: 2048 positions, T up to 2^20, no overflow of the slot size
    if (xb::ctc_grad_slot_floats(1 << 20, 2048) != ((size_t)(1 << 20) + 1) * 2048) { printf("the slot size FAILED\n"); ++failures; }
    if (failures) printf("%d case(s) failed\n", failures);
    else printf("ok\n");
    return failures ? 1 : 0;
}
