"""CPU: what a synchronising call reports for a context's two device status words (csrc/xb_status.h) -- the word of the
recurrence's rendezvous and the word of the kernels that validate device-resident lengths and labels.  A lost rendezvous
wins over everything; of the validation bits the loss's refusal is reported before the scan's; every text exists once, in
the header."""
import pytest

import host_logic
from xna_basecaller_amd import _lib

SYNC_TEXT = "LSTM inter-workgroup sync timed out (persistent kernel was not fully resident?)"
LOSS_TEXT = "xb_ctc_loss: a target length outside [state_len, Lt] or a label above n_base inside it"
SCAN_TEXT = "CTC scan: a target length was outside the lattice"
CASES = [(0, 0, _lib.XB_OK, None),
         (0, 2, _lib.XB_ERR_DEVICE, SCAN_TEXT),
         (0, 4, _lib.XB_ERR_INVALID, LOSS_TEXT),
         (0, 6, _lib.XB_ERR_INVALID, LOSS_TEXT),
         (1, 0, _lib.XB_ERR_DEVICE, SYNC_TEXT),
         (1, 2, _lib.XB_ERR_DEVICE, SYNC_TEXT),
         (1, 4, _lib.XB_ERR_DEVICE, SYNC_TEXT),
         (1, 6, _lib.XB_ERR_DEVICE, SYNC_TEXT)]


@pytest.mark.parametrize("sync_word,data_word,code,text", CASES, ids=["sync%d-data%d" % c[:2] for c in CASES])
def test_status_words_decode_to_the_code_and_text(sync_word, data_word, code, text):
    assert host_logic.decode_status(sync_word, data_word) == (code, text)
