// xb_status.h -- the two device status words of a context and what they mean to the host.  No HIP here: the decoder is
// checked on its own (tests/test_status_host.py, tools/host_logic_main.cpp).
//
// The sync word belongs to the persistent recurrence: a workgroup that gives up a rendezvous stores SYNC_LOST there, and its
// peers poll the word while they wait (LstmParams::error).  The data word belongs to the kernels that validate device-resident
// lengths and labels, which OR their bit in (CtcParams::error, CtcLossParams::error).  The words lie in different 64-byte
// lines, and nothing that writes one reads the other: a refused label never looks like a lost rendezvous.
#pragma once
#include "../../include/xna_basecaller.h"

namespace xb {

constexpr unsigned SYNC_LOST = 1u;            // sync word: a wait of the recurrence timed out
constexpr unsigned DATA_SCAN_LENGTH = 2u;     // data word: the CTC scan met a target length outside the lattice
constexpr unsigned DATA_LOSS_LABEL = 4u;      // data word: the loss / lattice kernels met a length or a label out of range

struct DeviceStatus {
    int code;                  // XB_OK or the xb_status to return
    const char *message;       // its text (nullptr with XB_OK)
    unsigned sync_left, data_left;      // the words once this report is taken out of them
};

// What a synchronising call reports for the two words, one condition at a time: a lost rendezvous first (the batch's results
// are garbage whatever else happened), then the refused loss input, then the refused scan length.
inline DeviceStatus decode_status(unsigned sync_word, unsigned data_word)
{
    if (sync_word != 0)
        return {XB_ERR_DEVICE, "LSTM inter-workgroup sync timed out (persistent kernel was not fully resident?)", 0u, data_word};
    if (data_word & DATA_LOSS_LABEL)
        return {XB_ERR_INVALID, "xb_ctc_loss: a target length outside [state_len, Lt] or a label above n_base inside it", 0u,
                data_word & ~DATA_LOSS_LABEL};
    if (data_word & DATA_SCAN_LENGTH)
        return {XB_ERR_DEVICE, "CTC scan: a target length was outside the lattice", 0u, data_word & ~DATA_SCAN_LENGTH};
    return {XB_OK, nullptr, 0u, data_word};
}

}  // namespace xb
