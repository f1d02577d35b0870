// The host-side label checks of xb_ctc_loss / xb_validate_chunks (csrc/xb_ctc_check.h) on their own, for a sanitizer run
// without a GPU and without Python:
//
//   clang++ -std=c++17 -g -fsanitize=address,undefined -fno-sanitize-recover=all tools/ctc_check_main.cpp -o /tmp/ctc_check && /tmp/ctc_check
//
// Every buffer is a heap allocation of exactly the size the contract names, so a read past a row's length, past a row or
// past the lengths is an error the sanitizer reports.  Exit status 0 and "ok" when every case gives the verdict it should.
#include <stdlib.h>
#include <string.h>

#include <vector>

#include "../xna_basecaller_amd/csrc/xb_ctc_check.h"

static int failures = 0;

static void expect(const char *what, int got, int want, const char *msg, const char *word)
{
    const bool ok = got == want && (want == 0 || strstr(msg, word));
    printf("%-44s %s%s%s\n", what, ok ? "ok" : "FAILED", want ? ": " : "", want ? msg : "");
    failures += !ok;
}

int main()
{
    const int n = 4, Lt = 14, sl = 3, nb = 5;
    char msg[160];
    // rows and lengths in exact heap blocks
    std::vector<uint8_t> good((size_t)n * Lt);
    for (size_t i = 0; i < good.size(); ++i) good[i] = (uint8_t)(1 + i % nb);
    const int32_t lens0[n] = {Lt, 7, sl, 9};
    for (int b = 0; b < n; ++b) memset(good.data() + (size_t)b * Lt + lens0[b], 0, (size_t)(Lt - lens0[b]));
    auto run = [&](const std::vector<uint8_t> &t, const int32_t *l, int width) {
        uint8_t *tt = static_cast<uint8_t *>(malloc((size_t)n * width));
        int32_t *ll = static_cast<int32_t *>(malloc(sizeof(int32_t) * n));
        memcpy(tt, t.data(), (size_t)n * width);
        memcpy(ll, l, sizeof(int32_t) * n);
        msg[0] = 0;
        const int rc = xb::ctc_labels_check(tt, n, width, ll, sl, nb, msg, sizeof msg);
        free(tt);
        free(ll);
        return rc;
    };
    expect("ragged rows, all legal", run(good, lens0, Lt), 0, msg, "");
    int32_t lens[n];
    memcpy(lens, lens0, sizeof lens);
    lens[2] = sl - 1;
    expect("a length of state_len - 1", run(good, lens, Lt), -1, msg, "target_lengths[2] = 2");
    lens[2] = Lt + 1;
    expect("a length of Lt + 1 (nothing of the row read)", run(good, lens, Lt), -1, msg, "target_lengths[2] = 15");
    lens[2] = -5;
    expect("a negative length", run(good, lens, Lt), -1, msg, "target_lengths[2] = -5");
    std::vector<uint8_t> bad = good;
    bad[(size_t)0 * Lt + Lt - 1] = nb + 1;
    expect("a label n_base + 1 at a full row's end", run(bad, lens0, Lt), -1, msg, "targets[0][13] = 6");
    bad = good;
    bad[(size_t)1 * Lt + lens0[1]] = 255;                   // the first byte beyond row 1's length: not read
    expect("a label beyond a row's length", run(bad, lens0, Lt), 0, msg, "");
    bad = good;
    bad[(size_t)3 * Lt + lens0[3] - 1] = 255;
    expect("a label of 255 inside the last row", run(bad, lens0, Lt), -1, msg, "targets[3][8] = 255");
    // the widest row the loss takes and one beyond (the width itself is refused by the entry points, not here)
    const int wide = 2048 + sl;
    std::vector<uint8_t> w((size_t)n * wide, 1);
    const int32_t wl[n] = {wide, sl, wide, sl};
    expect("rows of 2051 labels", run(w, wl, wide), 0, msg, "");
    // a message longer than its buffer is cut, not overrun
    char tiny[8];
    lens[2] = sl - 1;
    {
        uint8_t *tt = static_cast<uint8_t *>(malloc(good.size()));
        memcpy(tt, good.data(), good.size());
        const int rc = xb::ctc_labels_check(tt, n, Lt, lens, sl, nb, tiny, sizeof tiny);
        free(tt);
        expect("an 8-byte message buffer", rc, -1, tiny, "target_");
    }
    if (failures) printf("%d case(s) failed\n", failures);
    else printf("ok\n");
    return failures ? 1 : 0;
}
