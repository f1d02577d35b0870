// xb_ctc_check.h -- what every host form that takes label rows checks of them before anything is staged (label_batch_check,
// xb_ctx.h): plain host code without a HIP dependency (tools/ctc_check_main.cpp runs it on its own).
#pragma once
#include <stdint.h>
#include <stdio.h>

namespace xb {

// n label rows of Lt bytes with their lengths against a model of nb bases and state length sl: 0 when every length lies in
// [sl, Lt] and every label inside a row's length in [0, nb]; else -1 with the first offence in msg.  Nothing beyond a row's
// length is read, and nothing at all of a row whose length is out of range.
inline int ctc_labels_check(const uint8_t *targets, int n, int Lt, const int32_t *lengths, int sl, int nb, char *msg, size_t msg_len)
{
    for (int b = 0; b < n; ++b) {
        const int len = lengths[b];
        if (len < sl || len > Lt) {
            snprintf(msg, msg_len, "target_lengths[%d] = %d outside [state_len = %d, %d]", b, len, sl, Lt);
            return -1;
        }
        for (int l = 0; l < len; ++l)
            if (targets[(size_t)b * Lt + l] > nb) {
                snprintf(msg, msg_len, "targets[%d][%d] = %d outside [0, n_base = %d]", b, l, targets[(size_t)b * Lt + l], nb);
                return -1;
            }
    }
    return 0;
}

}  // namespace xb
