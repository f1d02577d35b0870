"""
ctypes binding of libxnacall.so (include/xna_basecaller.h).  There is NO fallback: if the
library is missing or no gfx950 GPU is present the product path raises, it never computes on
the CPU (the CPU restatement lives in oracle/ and is test infrastructure only).
"""
import ctypes as C
import os
import subprocess
import threading

import numpy as np

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("XNA_LIBXNACALL", os.path.join(_HERE, "libxnacall.so"))   # override: diagnostic builds only
_lib = None

XB_STAGE_NAMES = ("conv", "lstm_in", "lstm_rec", "linear", "decode")
XB_PREC_F16X3, XB_PREC_F16, XB_PREC_F16F8, XB_PREC_F16F8_IN1, XB_PREC_MIXED = 0, 1, 2, 3, 4
PRECISIONS = {"f16x3": XB_PREC_F16X3, "f16": XB_PREC_F16, "f16f8": XB_PREC_F16F8, "f16f8i": XB_PREC_F16F8_IN1,
              "mixed": XB_PREC_MIXED}

EXPORTS = [
    "xb_ctx_create", "xb_ctx_destroy", "xb_last_error", "xb_device_count", "xb_load_weights",
    "xb_weights_ready", "xb_encode", "xb_encode_dev", "xb_decode", "xb_decode_dev", "xb_crf_logz", "xb_crf_logz_dev", "xb_crf_scans", "xb_crf_scans_dev",
    "xb_basecall_chunks", "xb_basecall_chunks_dev", "xb_synchronize", "xb_set_profiling",
    "xb_get_stage_times", "xb_reset_stage_times", "xb_geometry", "xb_version", "xb_result_stream",
    "xb_submit_chunks", "xb_collect_chunks", "xb_ctc_logz", "xb_ctc_alignments",
    "xb_comm_unique_id", "xb_comm_create", "xb_comm_destroy", "xb_comm_rank", "xb_comm_world", "xb_comm_last_error",
    "xb_gather_called", "xb_comm_fence", "xb_comm_synchronize", "xb_stream_wait_event", "xb_align_accuracy",
    "xb_beam_search", "xb_beam_search_dev", "xb_basecall_chunks_beam", "xb_reserve_pairing", "xb_pairing_active", "xb_debug_layer_output",
    "xb_decode_q", "xb_decode_q_dev", "xb_basecall_chunks_q", "xb_submit_chunks_q", "xb_collect_chunks_q",
    "xb_decode_ub", "xb_decode_ub_dev", "xb_basecall_chunks_ub", "xb_submit_chunks_ub", "xb_collect_chunks_ub",
    "xb_map_templates", "xb_map_templates_dev", "xb_ctc_targets", "xb_ctc_targets_dev", "xb_ctc_chunks",
    "xb_ub_tally", "xb_ub_tally_dev", "xb_barcode_dist", "xb_barcode_dist_dev", "xb_dtw_segment", "xb_dtw_segment_dev", "xb_dtw_scratch_bytes",
    "xb_splice_library", "xb_splice_chunks", "xb_splice_chunks_dev",
    "xb_spike_model", "xb_spike_chunks", "xb_spike_chunks_dev", "xb_synth_chunks", "xb_synth_chunks_dev",
    "xb_ctc_loss", "xb_ctc_loss_dev", "xb_validate_chunks", "xb_ctc_loss_grad", "xb_ctc_loss_grad_dev",
    "xb_head_grad", "xb_head_grad_dev", "xb_grad_norm_dev", "xb_adamw_step_dev", "xb_head_repack_dev",
    "xb_head_train_begin", "xb_head_train_step", "xb_head_get_weights", "xb_head_train_end",
    "xb_lstm_train_forward_dev", "xb_lstm_train_backward_dev",
    "xb_linear_f32_dev", "xb_wgrad_f32_dev", "xb_head_dz_dev",
    "xb_encode_bottom_dev", "xb_transpose_f32_dev",
    "xb_top_train_begin", "xb_top_train_grad", "xb_top_train_step", "xb_top_get_weights", "xb_top_train_end",
    "xb_conv_train_forward_dev", "xb_conv_train_backward_dev", "xb_full_train_begin",
]
XB_COMM_ID_BYTES = 128
# xb_status (include/xna_basecaller.h)
XB_OK, XB_ERR_INVALID, XB_ERR_HIP, XB_ERR_NOMEM, XB_ERR_STATE, XB_ERR_DEVICE, XB_ERR_NO_GPU = 0, -1, -2, -3, -4, -5, -6
XB_PIPELINE_SLOTS = 4          # include/xna_basecaller.h


class XbConfig(C.Structure):
    _fields_ = [("n_base", C.c_int32), ("state_len", C.c_int32), ("features", C.c_int32),
                ("winlen", C.c_int32), ("stride", C.c_int32), ("scale", C.c_float),
                ("blank_score", C.c_float), ("chunk_len", C.c_int32), ("max_batch", C.c_int32),
                ("precision", C.c_int32), ("lstm_mode", C.c_int32)]


class XbError(RuntimeError):
    def __init__(self, code, msg):
        super().__init__("libxnacall error %d: %s" % (code, msg))
        self.code = code


def build(force=False):
    """Compile the HIP sources for gfx950 (csrc/Makefile; hipcc cross-compiles without a GPU)."""
    args = ["make", "-C", os.path.join(_HERE, "csrc"), "-j4"]
    if force:
        args.append("-B")
    subprocess.check_call(args, stdout=subprocess.DEVNULL)
    return LIB_PATH


def load():
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise ImportError("%s not found: build it with `python -c 'import __graft_entry__ as g; g.build()'` "
                          "(no CPU fallback exists for the MI355X path)" % LIB_PATH)
    lib = C.CDLL(LIB_PATH)
    vp, ip, fp = C.c_void_p, C.c_int, C.POINTER(C.c_float)
    lib.xb_ctx_create.argtypes = [C.POINTER(vp), ip, C.POINTER(XbConfig)]
    lib.xb_ctx_destroy.argtypes = [vp]
    lib.xb_ctx_destroy.restype = None
    lib.xb_last_error.argtypes = [vp]
    lib.xb_last_error.restype = C.c_char_p
    lib.xb_version.restype = C.c_char_p
    lib.xb_load_weights.argtypes = [vp, C.c_char_p, vp, C.c_int64]
    lib.xb_weights_ready.argtypes = [vp]
    lib.xb_encode.argtypes = [vp, vp, ip, ip, vp]
    lib.xb_encode_dev.argtypes = [vp, vp, ip, ip, vp]
    lib.xb_decode.argtypes = [vp, vp, ip, ip, ip, C.c_char_p, vp, vp, vp]
    lib.xb_decode_dev.argtypes = [vp, vp, ip, ip, ip, C.c_char_p, vp, vp, vp]
    lib.xb_crf_logz.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.xb_crf_logz_dev.argtypes = [vp, vp, ip, ip, ip, vp]
    lib.xb_crf_scans.argtypes = [vp, vp, ip, ip, ip, vp, vp, vp, vp]
    lib.xb_crf_scans_dev.argtypes = [vp, vp, ip, ip, ip, vp, vp, vp, vp]
    lib.xb_basecall_chunks.argtypes = [vp, vp, ip, C.c_char_p, vp, vp]
    lib.xb_basecall_chunks_dev.argtypes = [vp, vp, ip, C.c_char_p, vp, vp]
    lib.xb_synchronize.argtypes = [vp]
    lib.xb_reserve_pairing.argtypes = [vp]
    lib.xb_pairing_active.argtypes = [vp]
    lib.xb_comm_unique_id.argtypes = [C.c_char_p]
    lib.xb_comm_create.argtypes = [C.POINTER(vp), ip, ip, ip, C.c_char_p]
    lib.xb_comm_destroy.argtypes = [vp]
    lib.xb_comm_destroy.restype = None
    lib.xb_comm_rank.argtypes = [vp]
    lib.xb_comm_world.argtypes = [vp]
    lib.xb_comm_last_error.argtypes = [vp]
    lib.xb_comm_last_error.restype = C.c_char_p
    lib.xb_gather_called.argtypes = [vp, vp, vp, vp, ip, ip, vp, vp]
    lib.xb_comm_fence.argtypes = [vp, vp, ip]
    lib.xb_comm_synchronize.argtypes = [vp]
    lib.xb_stream_wait_event.argtypes = [vp, vp]
    lib.xb_align_accuracy.argtypes = [C.c_char_p, ip, C.c_char_p, ip, C.c_double, ip, C.POINTER(C.c_double), vp]
    lib.xb_ctc_logz.argtypes = [vp, vp, ip, ip, vp, ip, vp, vp, vp, vp]
    fl = C.c_float
    lib.xb_beam_search.argtypes = [vp, vp, ip, ip, ip, C.c_char_p, ip, fl, fl, fl, vp, vp, vp, vp]
    lib.xb_beam_search_dev.argtypes = [vp, vp, ip, ip, ip, C.c_char_p, ip, fl, fl, fl, vp, vp, vp, vp]
    lib.xb_basecall_chunks_beam.argtypes = [vp, vp, ip, C.c_char_p, ip, fl, fl, fl, vp, vp, vp, vp]
    lib.xb_ctc_alignments.argtypes = [vp, vp, ip, ip, vp, ip, vp, vp, vp]
    lib.xb_submit_chunks.argtypes = [vp, ip, vp, ip, C.c_char_p]
    lib.xb_collect_chunks.argtypes = [vp, ip, vp, vp]
    lib.xb_decode_q.argtypes = [vp, vp, ip, ip, ip, C.c_char_p, fl, fl, vp, vp, vp, vp]
    lib.xb_decode_q_dev.argtypes = [vp, vp, ip, ip, ip, C.c_char_p, fl, fl, vp, vp, vp, vp]
    lib.xb_basecall_chunks_q.argtypes = [vp, vp, ip, C.c_char_p, fl, fl, vp, vp, vp, vp]
    lib.xb_submit_chunks_q.argtypes = [vp, ip, vp, ip, C.c_char_p, fl, fl]
    lib.xb_collect_chunks_q.argtypes = [vp, ip, vp, vp, vp, vp]
    lib.xb_decode_ub.argtypes = [vp, vp, ip, ip, ip, C.c_char_p, fl, fl, vp, vp, vp, vp, vp]
    lib.xb_decode_ub_dev.argtypes = [vp, vp, ip, ip, ip, C.c_char_p, fl, fl, vp, vp, vp, vp, vp]
    lib.xb_basecall_chunks_ub.argtypes = [vp, vp, ip, C.c_char_p, fl, fl, vp, vp, vp, vp, vp]
    lib.xb_submit_chunks_ub.argtypes = [vp, ip, vp, ip, C.c_char_p, fl, fl]
    lib.xb_collect_chunks_ub.argtypes = [vp, ip, vp, vp, vp, vp, vp]
    lib.xb_map_templates.argtypes = [vp, vp, vp, ip, ip, C.c_char_p, vp, ip] + [ip] * 5 + [vp] * 10
    lib.xb_map_templates_dev.argtypes = lib.xb_map_templates.argtypes
    db = C.c_double
    lib.xb_ctc_targets.argtypes = [vp, vp, ip, ip, C.c_char_p, vp, ip] + [vp] * 8 + [db, db, ip, ip, ip] + [vp] * 5
    lib.xb_ctc_targets_dev.argtypes = lib.xb_ctc_targets.argtypes
    lib.xb_ctc_chunks.argtypes = [vp, vp, ip, C.c_char_p, C.c_char_p, vp, ip] + [ip] * 5 + [db, db, ip, ip, ip] + [vp] * 17
    lib.xb_ub_tally.argtypes = [vp, vp, vp, ip, ip, C.c_char_p, vp, ip] + [vp] * 11
    lib.xb_ub_tally_dev.argtypes = lib.xb_ub_tally.argtypes
    lib.xb_barcode_dist.argtypes = [vp, vp, vp, ip, ip, C.c_char_p, vp, ip] + [vp] * 4 + [ip] * 3 + [vp] * 4
    lib.xb_barcode_dist_dev.argtypes = lib.xb_barcode_dist.argtypes
    lib.xb_dtw_segment.argtypes = [vp, vp, ip, ip, vp, vp, ip, vp, ip, vp, vp, vp]
    lib.xb_dtw_segment_dev.argtypes = lib.xb_dtw_segment.argtypes
    lib.xb_dtw_scratch_bytes.argtypes = [vp]
    lib.xb_dtw_scratch_bytes.restype = C.c_int64
    lib.xb_splice_library.argtypes = [vp, vp, C.c_int64, vp, ip, vp, ip]
    lib.xb_splice_chunks.argtypes = [vp] * 5 + [ip, ip, ip, C.c_int64, C.c_uint64, ip, db, db, ip, ip] + [vp] * 4
    lib.xb_splice_chunks_dev.argtypes = lib.xb_splice_chunks.argtypes
    lib.xb_spike_model.argtypes = [vp, vp, vp, C.c_int64]
    lib.xb_spike_chunks.argtypes = [vp] * 5 + [ip, ip, ip, C.c_int64, C.c_uint64, ip, db, db, ip, ip, vp, db, ip] + [vp] * 6
    lib.xb_spike_chunks_dev.argtypes = lib.xb_spike_chunks.argtypes
    lib.xb_synth_chunks.argtypes = lib.xb_spike_chunks.argtypes
    lib.xb_synth_chunks_dev.argtypes = lib.xb_spike_chunks.argtypes
    lib.xb_ctc_loss.argtypes = [vp, vp, ip, ip, ip, vp, ip, vp, vp, vp]
    lib.xb_ctc_loss_dev.argtypes = lib.xb_ctc_loss.argtypes
    lib.xb_validate_chunks.argtypes = [vp, vp, ip, C.c_char_p, vp, ip, vp, vp, vp, vp]
    lib.xb_ctc_loss_grad.argtypes = [vp, vp, ip, ip, ip, vp, ip, vp, C.c_float, ip, vp, vp]
    lib.xb_ctc_loss_grad_dev.argtypes = lib.xb_ctc_loss_grad.argtypes
    lib.xb_head_grad.argtypes = [vp, vp, vp, vp, vp, C.c_int64, vp, vp]
    lib.xb_head_grad_dev.argtypes = lib.xb_head_grad.argtypes
    lib.xb_grad_norm_dev.argtypes = [vp, vp, C.c_int64, vp, C.c_int64, vp]
    lib.xb_adamw_step_dev.argtypes = [vp, vp, vp, vp, vp, C.c_int64, fl, fl, fl, fl]
    lib.xb_head_repack_dev.argtypes = [vp, vp, vp]
    lib.xb_internal_head_image.argtypes = [vp, vp, vp, vp, C.c_size_t, vp]
    lib.xb_internal_head_state.argtypes = [vp] + [C.POINTER(vp)] * 4 + [C.POINTER(C.c_int64)]
    lib.xb_internal_head_plan.argtypes = [C.c_int64, ip, ip, ip, C.c_char_p, vp]
    lib.xb_internal_head_plan.restype = None
    lib.xb_head_train_begin.argtypes = [vp, vp, vp]
    lib.xb_head_train_step.argtypes = [vp, vp, ip, vp, ip, vp, fl, fp, fp]
    lib.xb_head_get_weights.argtypes = [vp, vp, vp]
    lib.xb_head_train_end.argtypes = [vp]
    lib.xb_lstm_train_forward_dev.argtypes = [vp, vp, vp, ip, ip, ip, ip, vp, vp, vp]
    lib.xb_lstm_train_backward_dev.argtypes = [vp, vp, vp, vp, vp, ip, ip, ip, ip, vp]
    lib.xb_linear_f32_dev.argtypes = [vp, vp, vp, vp, C.c_int64, ip, ip, ip, fl, vp]
    lib.xb_wgrad_f32_dev.argtypes = [vp, vp, vp, C.c_int64, ip, ip, vp, vp]
    lib.xb_internal_wgrad_blocked.argtypes = [vp, vp, vp, C.c_int64, ip, ip, vp, vp, C.c_int64]
    lib.xb_head_dz_dev.argtypes = [vp, vp, vp, C.c_int64, fl, vp]
    lib.xb_encode_bottom_dev.argtypes = [vp, vp, ip, ip, vp]
    lib.xb_transpose_f32_dev.argtypes = [vp, vp, ip, ip, vp]
    lib.xb_top_train_begin.argtypes = [vp, ip, vp]
    lib.xb_top_train_grad.argtypes = [vp, vp, ip, vp, ip, vp, fp, fp]
    lib.xb_top_train_step.argtypes = [vp, vp, ip, vp, ip, vp, fl, fp, fp]
    lib.xb_top_get_weights.argtypes = [vp, vp]
    lib.xb_top_train_end.argtypes = [vp]
    lib.xb_conv_train_forward_dev.argtypes = [vp, vp, vp, vp] + [ip] * 7 + [vp, vp]
    lib.xb_conv_train_backward_dev.argtypes = [vp, vp, vp, vp, vp] + [ip] * 7 + [vp, vp, vp]
    lib.xb_full_train_begin.argtypes = [vp, vp]
    lib.xb_internal_top_state.argtypes = [vp] + [C.POINTER(vp)] * 7 + [C.POINTER(C.c_int64)] * 2
    lib.xb_internal_peek.argtypes = [vp, vp, vp, C.c_size_t]
    lib.xb_internal_bottom_part.argtypes = [vp, vp, ip, ip, vp, ip]
    lib.xb_result_stream.argtypes = [vp]
    lib.xb_result_stream.restype = C.c_void_p
    lib.xb_set_profiling.argtypes = [vp, ip]
    lib.xb_get_stage_times.argtypes = [vp, vp, vp]
    lib.xb_reset_stage_times.argtypes = [vp]
    lib.xb_geometry.argtypes = [vp, C.POINTER(ip), C.POINTER(ip), C.POINTER(ip), C.POINTER(ip)]
    lib.xb_debug_layer_output.argtypes = [vp, ip, ip, vp, vp]
    _lib = lib
    return lib


def align_accuracy(ref, seq, balanced=False, min_coverage=0.0, want_counts=False):
    """util.accuracy (util.py:402-424) through xb_align_accuracy: percent identity of the local alignment, 0 below min_coverage."""
    r, q = ref.encode("ascii"), seq.encode("ascii")
    acc = C.c_double()
    counts = (C.c_int32 * 4)()
    rc = load().xb_align_accuracy(r, len(r), q, len(q), float(min_coverage), int(bool(balanced)), C.byref(acc), counts)
    if rc:
        raise XbError(rc, "xb_align_accuracy: bad argument")
    return (acc.value, dict(zip("=XID", counts))) if want_counts else acc.value


def source_digest():
    """sha1 (12 hex digits) over the library's sources (csrc/*.hip, *.h, Makefile and the public header): what bench.py and
    tools/hbm_traffic.py record so that a counter profile is only ever quoted for the code it was collected on."""
    import glob
    import hashlib
    h = hashlib.sha1()
    csrc = os.path.join(_HERE, "csrc")
    files = sorted(glob.glob(os.path.join(csrc, "*.hip")) + glob.glob(os.path.join(csrc, "*.h")) + [os.path.join(csrc, "Makefile")])
    files.append(os.path.join(os.path.dirname(_HERE), "include", "xna_basecaller.h"))
    for f in files:
        h.update(os.path.basename(f).encode())
        h.update(open(f, "rb").read())
    return h.hexdigest()[:12]


def device_count():
    return int(load().xb_device_count())


def require_gpu():
    if device_count() < 1:
        raise RuntimeError("no HIP device visible: the xna_basecaller_amd hot path runs on MI355X (gfx950) only")


def _ptr(a):
    if a is None:
        return None
    if isinstance(a, np.ndarray):
        return a.ctypes.data
    return int(a)          # raw device pointer (e.g. torch.Tensor.data_ptr())


def output_level(qscores=False, ub_probs=False):
    """Output level of the Viterbi decode: 0 the bases, 1 also qualities and moves (the _q entry points), 2 also the letter
    probabilities (_ub; they imply the qualities)."""
    return 2 if ub_probs else int(bool(qscores))


def _mean_flag(reduction):
    """CTC_CRF.ctc_loss's reduction as the flag of xb_ctc_loss_grad."""
    if reduction == "mean":
        return 1
    if reduction in ("none", None):
        return 0
    raise ValueError("Unknown reduction type {}".format(reduction))


def _lens_last(out):
    """An output tuple (seq, lens[, qstring, moves[, probs]]) as the pointers of the decode / basecall entry points: lens last."""
    return [_ptr(a) for a in out[:1] + out[2:] + out[1:2]]


def _calib(level, qscale, qoffset):
    return (float(qscale), float(qoffset)) if level else ()


class _Locked:
    """One library function behind a context's lock; argtypes / restype are the function's own."""
    __slots__ = ("fn", "lock")

    def __init__(self, fn, lock):
        self.fn, self.lock = fn, lock

    def __call__(self, *args):
        with self.lock:
            return self.fn(*args)

    argtypes = property(lambda self: self.fn.argtypes, lambda self, v: setattr(self.fn, "argtypes", v))
    restype = property(lambda self: self.fn.restype, lambda self, v: setattr(self.fn, "restype", v))


class _OneCallAtATime:
    """The library's functions behind one lock: an xb_ctx is used by one thread at a time (include/xna_basecaller.h), and the
    basecalling pipeline's device stage and the mapper of `--reference` reach the same context from two threads."""

    def __init__(self, lib):
        self._lib, self._lock = lib, threading.RLock()

    def __getattr__(self, name):
        call = _Locked(getattr(self._lib, name), self._lock)
        setattr(self, name, call)
        return call


class UbAccumulators:
    """The accumulators of xb_ub_tally for a library with `offsets` (R + 1): reads (R, 2) int32 rows per (template, strand),
    err (2, sum(L)) int32 errors per (strand, template position), cm (6, 7) int64 confusion matrix; zero to start with."""
    __slots__ = ("reads", "err", "cm")

    def __init__(self, offsets):
        offsets = np.asarray(offsets)
        self.reads = np.zeros((offsets.size - 1, 2), np.int32)
        self.err = np.zeros((2, int(offsets[-1])), np.int32)
        self.cm = np.zeros((6, 7), np.int64)


class Context:
    """One xb_ctx: a GPU, a stream, the device copies of the weights and all workspaces."""

    def __init__(self, device, n_base, state_len, features, winlen, stride, scale, blank_score,
                 chunk_len, max_batch, precision=XB_PREC_F16X3, lstm_mode=0):
        self.lib = _OneCallAtATime(load())
        self.cfg = XbConfig(n_base, state_len, features, winlen, stride, scale, blank_score, chunk_len,
                            max_batch, precision, lstm_mode)
        h = C.c_void_p()
        rc = self.lib.xb_ctx_create(C.byref(h), int(device), C.byref(self.cfg))
        if rc:
            raise XbError(rc, (self.lib.xb_last_error(None) or b"").decode())
        self.h = h
        T, S, Cb, Cn = C.c_int(), C.c_int(), C.c_int(), C.c_int()
        self.lib.xb_geometry(self.h, C.byref(T), C.byref(S), C.byref(Cb), C.byref(Cn))
        self.T, self.S, self.C_blank, self.C_noblank = T.value, S.value, Cb.value, Cn.value
        self.n_base, self.chunk_len, self.max_batch = n_base, chunk_len, max_batch

    def _check(self, rc):
        if rc:
            raise XbError(rc, (self.lib.xb_last_error(self.h) or b"").decode())

    def close(self):
        if getattr(self, "h", None):
            self.lib.xb_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _scores(self, scores, has_blank):
        """(T, n, C) scores as contiguous fp32 and the has_blank flag (0 / 1) of their layout, checked against the model."""
        scores = np.ascontiguousarray(scores, dtype=np.float32)
        Cin = scores.shape[2]
        if has_blank is None:
            has_blank = Cin == self.C_blank
        if Cin != (self.C_blank if has_blank else self.C_noblank):
            raise ValueError("scores last dim %d does not match the model (%d with blanks, %d without)"
                             % (Cin, self.C_blank, self.C_noblank))
        return scores, int(bool(has_blank))

    def _outputs(self, level, n, T):
        """Host outputs of an output level: (seq (n, T) int8, lens (n,) int32[, qstring (n, T) int8, moves (n, T) uint8[,
        probs (n, nb, T) uint8]])."""
        out = (np.empty((n, T), dtype=np.int8), np.empty((n,), dtype=np.int32))
        if level >= 1:
            out += (np.empty((n, T), dtype=np.int8), np.empty((n, T), dtype=np.uint8))
        if level == 2:
            out += (np.empty((n, self.n_base, T), dtype=np.uint8),)
        return out

    def load_state_dict(self, state_dict):
        """state_dict: name -> fp32 array in PyTorch layout (the 28 inference-encoder tensors)."""
        for k, v in state_dict.items():
            a = np.ascontiguousarray(np.asarray(v, dtype=np.float32))
            self._check(self.lib.xb_load_weights(self.h, k.encode(), a.ctypes.data, a.size))
        self._check(self.lib.xb_weights_ready(self.h))

    def debug_layer_output(self, which, n):
        """(hi, second) uint16 arrays (T, n, features) of LSTM layer 3 (which = 0) / 4 (1) after the last encode of n chunks."""
        F = self.cfg.features
        hi = np.empty((self.T, n, F), dtype=np.uint16)
        second = np.empty((self.T, n, F), dtype=np.uint16)
        self._check(self.lib.xb_debug_layer_output(self.h, int(which), int(n), hi.ctypes.data, second.ctypes.data))
        return hi, second

    # ---- host-buffer operators ---------------------------------------------------------
    def encode(self, signal, expand_blanks=True):
        signal = np.ascontiguousarray(signal, dtype=np.float32).reshape(-1, self.chunk_len)
        n = signal.shape[0]
        scores = np.empty((self.T, n, self.C_blank if expand_blanks else self.C_noblank), dtype=np.float32)
        self._check(self.lib.xb_encode(self.h, signal.ctypes.data, n, int(bool(expand_blanks)), scores.ctypes.data))
        return scores

    def decode(self, scores, alphabet, has_blank=None, want_labels=False):
        scores, has_blank = self._scores(scores, has_blank)
        T, n, _ = scores.shape
        labels = np.empty((n, T), dtype=np.int8) if want_labels else None
        seq, lens = self._outputs(0, n, T)
        self._check(self.lib.xb_decode(self.h, scores.ctypes.data, T, n, has_blank, "".join(alphabet).encode(), _ptr(labels),
                                       seq.ctypes.data, lens.ctypes.data))
        return (seq, lens, labels) if want_labels else (seq, lens)

    def crf_logz(self, scores, has_blank=None):
        """(T, n, C) scores -> (n,) fp32 log partition function (CTC_CRF.logZ, crf/model.py:41-46)."""
        scores, has_blank = self._scores(scores, has_blank)
        T, n, _ = scores.shape
        logz = np.empty((n,), dtype=np.float32)
        self._check(self.lib.xb_crf_logz(self.h, scores.ctypes.data, T, n, has_blank, logz.ctypes.data))
        return logz

    def crf_scans(self, scores, want=("alpha", "beta", "logz", "post"), has_blank=None):
        """(T, n, C) scores -> dict of the Log scans (xb_crf_scans): 'alpha', 'beta' (T+1, n, S), 'logz' (n,),
        'post' (T, n, S*(n_base+1))."""
        scores, has_blank = self._scores(scores, has_blank)
        T, n, _ = scores.shape
        S = self.C_blank // (self.n_base + 1)
        shapes = {"alpha": (T + 1, n, S), "beta": (T + 1, n, S), "logz": (n,), "post": (T, n, self.C_blank)}
        out = {k: np.empty(shapes[k], dtype=np.float32) for k in want}
        self._check(self.lib.xb_crf_scans(self.h, scores.ctypes.data, T, n, has_blank, _ptr(out.get("alpha")),
                                          _ptr(out.get("beta")), _ptr(out.get("logz")), _ptr(out.get("post"))))
        return out

    def ctc_logz(self, scores, targets, target_lengths, want_grads=False):
        """xb_ctc_logz: scores (T, n, C_blank), targets (n, Lt) CTC labels, target_lengths (n) -> {'logz': (n,)} and, with
        want_grads, 'stay' (T, n, np) / 'move' (T, n, np - 1), np = Lt - state_len + 1 (the restricted posteriors)."""
        scores = np.ascontiguousarray(scores, dtype=np.float32)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        tl = np.ascontiguousarray(target_lengths, dtype=np.int32)
        T, n, Cin = scores.shape
        if Cin != self.C_blank or targets.shape[0] != n or tl.shape != (n,):
            raise ValueError("ctc_logz: scores (T, n, %d), targets (n, Lt), target_lengths (n) expected" % self.C_blank)
        Lt = targets.shape[1]
        npos = Lt - (self.cfg.state_len - 1)
        out = {"logz": np.empty((n,), np.float32)}
        if want_grads:
            out["stay"] = np.empty((T, n, max(npos, 0)), np.float32)
            out["move"] = np.empty((T, n, max(npos - 1, 0)), np.float32)
        self._check(self.lib.xb_ctc_logz(self.h, scores.ctypes.data, T, n, targets.ctypes.data, Lt, tl.ctypes.data,
                                         out["logz"].ctypes.data, _ptr(out.get("stay")), _ptr(out.get("move"))))
        return out

    def ctc_alignments(self, scores, targets, target_lengths):
        """xb_ctc_alignments: (alignments (T, n, np) one-hot over target positions, max path score (n,))."""
        scores = np.ascontiguousarray(scores, dtype=np.float32)
        targets = np.ascontiguousarray(targets, dtype=np.int32)
        tl = np.ascontiguousarray(target_lengths, dtype=np.int32)
        T, n, Cin = scores.shape
        if Cin != self.C_blank or targets.shape[0] != n or tl.shape != (n,):
            raise ValueError("ctc_alignments: scores (T, n, %d), targets (n, Lt), target_lengths (n) expected" % self.C_blank)
        Lt = targets.shape[1]
        npos = Lt - (self.cfg.state_len - 1)
        al = np.empty((T, n, max(npos, 0)), np.float32)
        best = np.empty((n,), np.float32)
        self._check(self.lib.xb_ctc_alignments(self.h, scores.ctypes.data, T, n, targets.ctypes.data, Lt, tl.ctypes.data,
                                               al.ctypes.data, best.ctypes.data))
        return al, best

    @staticmethod
    def _labels(targets, lengths, n):
        """(n, Lt) label rows as contiguous uint8 (references.npy's own type) and their lengths as int32."""
        t = np.asarray(targets)
        if t.ndim != 2 or t.shape[0] != n or (t.size and (t.min() < 0 or t.max() > 255)):
            raise ValueError("targets: (n, Lt) labels 0 .. 255 expected")
        tl = np.ascontiguousarray(lengths, dtype=np.int32)
        if tl.shape != (n,):
            raise ValueError("target_lengths: (n) expected")
        return np.ascontiguousarray(t, dtype=np.uint8), tl

    def _chunk_batch(self, signal, targets, target_lengths):
        """What the calls on labelled chunks pass: signal as contiguous (n, chunk_len) fp32, and its _labels."""
        signal = np.ascontiguousarray(signal, dtype=np.float32).reshape(-1, self.chunk_len)
        return (signal,) + self._labels(targets, target_lengths, signal.shape[0])

    def _train_call(self, fn, signal, targets, target_lengths, *lr):
        """A trainer's call fn on labelled chunks, at a learning rate or without one -> (mean loss, gradient norm)."""
        signal, targets, tl = self._chunk_batch(signal, targets, target_lengths)
        loss, norm = C.c_float(), C.c_float()
        self._check(fn(self.h, signal.ctypes.data, signal.shape[0], targets.ctypes.data, targets.shape[1], tl.ctypes.data,
                       *map(float, lr), C.byref(loss), C.byref(norm)))
        return loss.value, norm.value

    def ctc_loss(self, scores, targets, target_lengths, has_blank=True, want_logz=False):
        """xb_ctc_loss: RAW scores (T, n, C) in either layout, targets (n, Lt) CTC labels, target_lengths (n) -> loss (n,) fp32 =
        CTC_CRF.ctc_loss(..., normalise_scores=True, reduction='none'); with want_logz (loss, logz_ctc)."""
        scores, has_blank = self._scores(scores, has_blank)
        T, n, _ = scores.shape
        targets, tl = self._labels(targets, target_lengths, n)
        loss = np.empty((n,), np.float32)
        logz = np.empty((n,), np.float32) if want_logz else None
        self._check(self.lib.xb_ctc_loss(self.h, scores.ctypes.data, T, n, has_blank, targets.ctypes.data, targets.shape[1],
                                         tl.ctypes.data, loss.ctypes.data, _ptr(logz)))
        return (loss, logz) if want_logz else loss

    def ctc_loss_dev(self, d_scores, T, n, has_blank, d_targets, Lt, d_lengths, d_loss, d_logz=None):
        self._check(self.lib.xb_ctc_loss_dev(self.h, _ptr(d_scores), int(T), int(n), int(bool(has_blank)), _ptr(d_targets), int(Lt),
                                             _ptr(d_lengths), _ptr(d_loss), _ptr(d_logz)))

    def ctc_loss_grad(self, scores, targets, target_lengths, has_blank=None, loss_clip=None, reduction="mean"):
        """xb_ctc_loss_grad: RAW scores (T, n, C) in either layout -> (loss (n,) fp32, clamped when clipping; grad (T, n, C) fp32 =
        d CTC_CRF.ctc_loss(..., loss_clip, reduction, normalise_scores=True) / d scores)."""
        scores, has_blank = self._scores(scores, has_blank)
        T, n, _ = scores.shape
        targets, tl = self._labels(targets, target_lengths, n)
        loss = np.empty((n,), np.float32)
        grad = np.empty_like(scores)
        self._check(self.lib.xb_ctc_loss_grad(self.h, scores.ctypes.data, T, n, has_blank, targets.ctypes.data, targets.shape[1],
                                              tl.ctypes.data, float(loss_clip or 0.0), _mean_flag(reduction), loss.ctypes.data,
                                              grad.ctypes.data))
        return loss, grad

    def ctc_loss_grad_dev(self, d_scores, T, n, has_blank, d_targets, Lt, d_lengths, d_loss, d_grad, loss_clip=None,
                          reduction="mean"):
        self._check(self.lib.xb_ctc_loss_grad_dev(self.h, _ptr(d_scores), int(T), int(n), int(bool(has_blank)), _ptr(d_targets),
                                                  int(Lt), _ptr(d_lengths), float(loss_clip or 0.0), _mean_flag(reduction),
                                                  _ptr(d_loss), _ptr(d_grad)))

    # ---- the head's gradient and trainer (csrc/xb_head.hip) ------------------------------
    def head_grad(self, y, dy, x_hi=None, x_lo=None):
        """xb_head_grad: RAW blank-less scores y and their gradient dy, both (M, C_noblank) fp32, and X (M, features) as fp16 bit
        patterns x_hi + x_lo (both None: the last LSTM layer's output of the last encode, M = T n) -> (dW (C_noblank, features),
        db (C_noblank,)) fp32, the gradient of the head's weight and bias."""
        O, F = self.C_noblank, self.cfg.features
        y = np.ascontiguousarray(y, dtype=np.float32).reshape(-1, O)
        dy = np.ascontiguousarray(dy, dtype=np.float32).reshape(-1, O)
        M = y.shape[0]
        if dy.shape != y.shape:
            raise ValueError("head_grad: y and dy of one shape (M, %d) expected" % O)
        if x_hi is not None:
            x_hi = np.ascontiguousarray(x_hi, dtype=np.uint16).reshape(-1, F)
            x_lo = np.ascontiguousarray(x_lo, dtype=np.uint16).reshape(-1, F)
            if x_hi.shape != (M, F) or x_lo.shape != (M, F):
                raise ValueError("head_grad: x_hi, x_lo (M, %d) expected" % F)
        dw, db = np.empty((O, F), np.float32), np.empty((O,), np.float32)
        self._check(self.lib.xb_head_grad(self.h, y.ctypes.data, dy.ctypes.data, _ptr(x_hi), _ptr(x_lo), M, dw.ctypes.data,
                                          db.ctypes.data))
        return dw, db

    def head_grad_dev(self, d_y, d_dy, d_x_hi, d_x_lo, rows, d_dw, d_db):
        self._check(self.lib.xb_head_grad_dev(self.h, _ptr(d_y), _ptr(d_dy), _ptr(d_x_hi), _ptr(d_x_lo), int(rows), _ptr(d_dw),
                                              _ptr(d_db)))

    def grad_norm_dev(self, d_dw, len_w, d_db, len_b, d_norm):
        self._check(self.lib.xb_grad_norm_dev(self.h, _ptr(d_dw), int(len_w), _ptr(d_db), int(len_b), _ptr(d_norm)))

    def adamw_step_dev(self, d_p, d_g, d_m, d_v, length, clip, decay, step_size, bc2_sqrt):
        self._check(self.lib.xb_adamw_step_dev(self.h, _ptr(d_p), _ptr(d_g), _ptr(d_m), _ptr(d_v), int(length), float(clip),
                                               float(decay), float(step_size), float(bc2_sqrt)))

    def head_repack_dev(self, d_w, d_b):
        self._check(self.lib.xb_head_repack_dev(self.h, _ptr(d_w), _ptr(d_b)))

    def lstm_train_forward_dev(self, d_gin, d_w_hh, T, n, F, reverse, d_y, d_gates, d_c):
        """xb_lstm_train_forward_dev: gin (T, n, 4F), W_hh (4F, F) -> y (T, n, F), gates (T, n, 4F), c (T, n, F), all fp32 on the device."""
        self._check(self.lib.xb_lstm_train_forward_dev(self.h, _ptr(d_gin), _ptr(d_w_hh), int(T), int(n), int(F), int(bool(reverse)),
                                                       _ptr(d_y), _ptr(d_gates), _ptr(d_c)))

    def lstm_train_backward_dev(self, d_dy, d_w_hh, d_gates, d_c, T, n, F, reverse, d_dgin):
        """xb_lstm_train_backward_dev: dy (T, n, F) and the forward's gates and c -> dgin (T, n, 4F)."""
        self._check(self.lib.xb_lstm_train_backward_dev(self.h, _ptr(d_dy), _ptr(d_w_hh), _ptr(d_gates), _ptr(d_c), int(T), int(n), int(F),
                                                        int(bool(reverse)), _ptr(d_dgin)))

    def head_image(self):
        """The head's weights as the forward reads them: (hi, lo (C_noblank, features) uint16, the fragment-major image (bytes),
        bias (C_noblank,) fp32)."""
        O, F = self.C_noblank, self.cfg.features
        hi, lo = np.empty((O, F), np.uint16), np.empty((O, F), np.uint16)
        f4 = np.empty(((F // 32) * (((O + 255) & ~255) // 32) * 4 * 1024,), np.uint8)
        bias = np.empty((O,), np.float32)
        self._check(self.lib.xb_internal_head_image(self.h, hi.ctypes.data, lo.ctypes.data, f4.ctypes.data, f4.size, bias.ctypes.data))
        return hi, lo, f4, bias

    def head_train_begin(self, w, b):
        O, F = self.C_noblank, self.cfg.features
        w = np.ascontiguousarray(w, dtype=np.float32)
        b = np.ascontiguousarray(b, dtype=np.float32)
        if w.shape != (O, F) or b.shape != (O,):
            raise ValueError("head_train_begin: weight (%d, %d) and bias (%d,) expected" % (O, F, O))
        self._check(self.lib.xb_head_train_begin(self.h, w.ctypes.data, b.ctypes.data))

    def head_train_step(self, signal, targets, target_lengths, lr):
        """xb_head_train_step: one AdamW step of the head on n chunks -> (mean loss before the step, gradient norm before clipping)."""
        return self._train_call(self.lib.xb_head_train_step, signal, targets, target_lengths, lr)

    def head_state_dev(self):
        """Device pointers of an open trainer's (p, m, v, g), each (W | b) fp32, and the steps taken (tests)."""
        ptrs = [C.c_void_p() for _ in range(4)]
        step = C.c_int64()
        self._check(self.lib.xb_internal_head_state(self.h, *[C.byref(p) for p in ptrs], C.byref(step)))
        return tuple(p.value for p in ptrs) + (step.value,)

    def head_get_weights(self):
        O, F = self.C_noblank, self.cfg.features
        w, b = np.empty((O, F), np.float32), np.empty((O,), np.float32)
        self._check(self.lib.xb_head_get_weights(self.h, w.ctypes.data, b.ctypes.data))
        return w, b

    def head_train_end(self):
        self._check(self.lib.xb_head_train_end(self.h))

    # ---- the fp32 products of training (csrc/xb_train_gemm.hip) -------------------------------------------------------------------
    def linear_f32_dev(self, d_a, d_w, d_bias, M, N, K, act, scale, d_out):
        """xb_linear_f32_dev: out (M, N) = act(a (M, K) w (N, K)^T + bias); act 0 identity, 1 scale * tanh.  fp32 on the device."""
        self._check(self.lib.xb_linear_f32_dev(self.h, _ptr(d_a), _ptr(d_w), _ptr(d_bias), int(M), int(N), int(K), int(act), float(scale),
                                               _ptr(d_out)))

    def wgrad_f32_dev(self, d_a, d_b, M, N, K, d_dw, d_dcol, block_rows=None):
        """xb_wgrad_f32_dev: dw (N, K) = a (M, N)^T b (M, K), dcol (N) = column sums of a (or None).  block_rows: the measurement
        entry with another length of the row blocks (a multiple of 32)."""
        if block_rows is None:
            self._check(self.lib.xb_wgrad_f32_dev(self.h, _ptr(d_a), _ptr(d_b), int(M), int(N), int(K), _ptr(d_dw), _ptr(d_dcol)))
        else:
            self._check(self.lib.xb_internal_wgrad_blocked(self.h, _ptr(d_a), _ptr(d_b), int(M), int(N), int(K), _ptr(d_dw), _ptr(d_dcol),
                                                           int(block_rows)))

    def head_dz_dev(self, d_y, d_dy, count, scale, d_dz):
        self._check(self.lib.xb_head_dz_dev(self.h, _ptr(d_y), _ptr(d_dy), int(count), float(scale), _ptr(d_dz)))

    # ---- the trainer of the head and the top LSTM layers (csrc/xb_top.hip) ----------------------------------------------------------
    def encode_bottom_dev(self, d_signal, n, layers, d_x0):
        """xb_encode_bottom_dev: signal (n, chunk_len) on the device -> x0 (T, n, features) fp32 on the device, the output of the
        convolutions (layers = 0) or of LSTM layer layers - 1."""
        self._check(self.lib.xb_encode_bottom_dev(self.h, _ptr(d_signal), int(n), int(layers), _ptr(d_x0)))

    def bottom_part_dev(self, d_signal, n, layers, d_x0, what):
        """encode_bottom_dev in halves (tools/toptrain_time.py): what = 1 the pass alone, 2 the join of the planes it left."""
        self._check(self.lib.xb_internal_bottom_part(self.h, _ptr(d_signal), int(n), int(layers), _ptr(d_x0), int(what)))

    def transpose_f32_dev(self, d_in, rows, cols, d_out):
        """xb_transpose_f32_dev: out (cols, rows) = in (rows, cols)^T, fp32 on the device."""
        self._check(self.lib.xb_transpose_f32_dev(self.h, _ptr(d_in), int(rows), int(cols), _ptr(d_out)))

    def top_params(self, layers):
        """Floats of the flat parameter buffer of a trainer of the head and the top `layers` LSTM layers (csrc/xb_top_plan.h)."""
        F, O = self.cfg.features, self.C_noblank
        return layers * (8 * F * F + 8 * F) + O * F + O

    def top_train_begin(self, layers, params):
        """xb_top_train_begin: params, the 4 layers + 2 tensors flat in state-dict order (top_params(layers) floats)."""
        params = np.ascontiguousarray(params, dtype=np.float32)
        if 1 <= layers <= 5 and params.shape != (self.top_params(layers),):
            raise ValueError("top_train_begin: %d floats expected for %d layers, got %r" % (self.top_params(layers), layers, params.shape))
        self._check(self.lib.xb_top_train_begin(self.h, int(layers), params.ctypes.data))
        self._top_layers = int(layers)

    # ---- the convolutions' training, and the trainer of every layer (csrc/xb_conv_train.hip, xb_top.hip) --------------------------
    def conv_train_forward_dev(self, d_x, d_w, d_b, n, Cin, Lin, Cout, K, stride, tnc, d_z, d_y):
        """xb_conv_train_forward_dev: x (n, Cin, Lin), w (Cout, Cin, K), b (Cout) -> the pre-activation z and y = swish(z), both
        (n, Cout, Lout), or (Lout, n, Cout) with tnc; fp32 on the device."""
        self._check(self.lib.xb_conv_train_forward_dev(self.h, _ptr(d_x), _ptr(d_w), _ptr(d_b), int(n), int(Cin), int(Lin), int(Cout), int(K),
                                                       int(stride), int(bool(tnc)), _ptr(d_z), _ptr(d_y)))

    def conv_train_backward_dev(self, d_dy, d_x, d_z, d_w, n, Cin, Lin, Cout, K, stride, tnc, d_dx, d_dw, d_db):
        """xb_conv_train_backward_dev: dy and the forward's x, z, w -> dx (n, Cin, Lin) (None: not wanted), dw (Cout, Cin, K), db (Cout)."""
        self._check(self.lib.xb_conv_train_backward_dev(self.h, _ptr(d_dy), _ptr(d_x), _ptr(d_z), _ptr(d_w), int(n), int(Cin), int(Lin), int(Cout),
                                                        int(K), int(stride), int(bool(tnc)), _ptr(d_dx), _ptr(d_dw), _ptr(d_db)))

    def full_params(self):
        """Floats of the flat parameter buffer of a trainer of every layer: the conv section of csrc/xb_conv_plan.h, then top_params(5)."""
        F = self.cfg.features
        return 360 + F * (16 * self.cfg.winlen + 1) + self.top_params(5)

    def full_train_begin(self, params):
        """xb_full_train_begin: params, all 28 tensors flat in state-dict order (full_params() floats).  top_train_grad / _step,
        top_get_weights and top_train_end serve this trainer too."""
        params = np.ascontiguousarray(params, dtype=np.float32)
        if params.shape != (self.full_params(),):
            raise ValueError("full_train_begin: %d floats expected, got %r" % (self.full_params(), params.shape))
        self._check(self.lib.xb_full_train_begin(self.h, params.ctypes.data))
        self._top_layers = "full"

    def top_train_grad(self, signal, targets, target_lengths):
        """xb_top_train_grad: the gradient of one batch, left unclipped on the device -> (mean loss, gradient norm)."""
        return self._train_call(self.lib.xb_top_train_grad, signal, targets, target_lengths)

    def top_train_step(self, signal, targets, target_lengths, lr):
        """xb_top_train_step: one clipped AdamW step on n chunks -> (mean loss before the step, gradient norm before clipping)."""
        return self._train_call(self.lib.xb_top_train_step, signal, targets, target_lengths, lr)

    def top_state_dev(self):
        """Device pointers of an open trainer: dict(p, g, m, v: the flat buffers; x0, scores, dscores of the last step (None
        before the first); rows = T n of that step; step: the steps taken) (tests)."""
        ptrs = [C.c_void_p() for _ in range(7)]
        rows, step = C.c_int64(), C.c_int64()
        self._check(self.lib.xb_internal_top_state(self.h, *[C.byref(p) for p in ptrs], C.byref(rows), C.byref(step)))
        out = dict(zip(("p", "g", "m", "v", "x0", "scores", "dscores"), (p.value for p in ptrs)))
        out.update(rows=rows.value, step=step.value)
        return out

    def peek(self, d_ptr, shape, dtype=np.float32):
        """Device memory at a raw pointer as a host array, behind everything the context has enqueued (tests)."""
        out = np.empty(shape, dtype)
        self._check(self.lib.xb_internal_peek(self.h, int(d_ptr), out.ctypes.data, out.nbytes))
        return out

    def top_get_weights(self):
        """xb_top_get_weights: the fp32 master weights, flat, as top_train_begin took them."""
        layers = getattr(self, "_top_layers", 1)
        params = np.empty((self.full_params() if layers == "full" else self.top_params(layers),), np.float32)
        self._check(self.lib.xb_top_get_weights(self.h, params.ctypes.data))
        return params

    def top_train_end(self):
        self._check(self.lib.xb_top_train_end(self.h))

    def validate_chunks(self, signal, alphabet, targets, target_lengths):
        """xb_validate_chunks: signal (n, chunk_len), targets (n, Lt), target_lengths (n) -> (seq (n, T) int8 left-packed ASCII,
        lens (n,), loss (n,) fp32): basecall_chunks' calls and ctc_loss of the same scores, which never leave the device."""
        signal, targets, tl = self._chunk_batch(signal, targets, target_lengths)
        n = signal.shape[0]
        seq, lens = self._outputs(0, n, self.T)
        loss = np.empty((n,), np.float32)
        self._check(self.lib.xb_validate_chunks(self.h, signal.ctypes.data, n, "".join(alphabet).encode(), targets.ctypes.data,
                                                targets.shape[1], tl.ctypes.data, seq.ctypes.data, lens.ctypes.data,
                                                loss.ctypes.data))
        return seq, lens, loss

    def crf_scans_dev(self, d_scores, T, n, has_blank, d_alpha=None, d_beta=None, d_logz=None, d_post=None):
        self._check(self.lib.xb_crf_scans_dev(self.h, _ptr(d_scores), T, n, int(bool(has_blank)), _ptr(d_alpha), _ptr(d_beta),
                                              _ptr(d_logz), _ptr(d_post)))

    def crf_logz_dev(self, d_scores, T, n, has_blank, d_logz):
        self._check(self.lib.xb_crf_logz_dev(self.h, _ptr(d_scores), T, n, int(bool(has_blank)), _ptr(d_logz)))

    # ---- the Viterbi basecall at an output level (output_level): 0 xb_basecall_chunks, 1 _q, 2 _ub ----------
    def basecall_chunks(self, signal, alphabet, qscale=1.0, qoffset=0.0, level=0):
        """signal (n, chunk_len) -> (seq (n, T) int8 left-packed ASCII, lens (n,)), at level 1 also (qstring, moves) and at level
        2 also probs, as decode_q / decode_ub return them."""
        signal = np.ascontiguousarray(signal, dtype=np.float32).reshape(-1, self.chunk_len)
        n = signal.shape[0]
        out = self._outputs(level, n, self.T)
        fn = (self.lib.xb_basecall_chunks, self.lib.xb_basecall_chunks_q, self.lib.xb_basecall_chunks_ub)[level]
        self._check(fn(self.h, signal.ctypes.data, n, "".join(alphabet).encode(), *_calib(level, qscale, qoffset),
                       *_lens_last(out)))
        return out

    # ---- Viterbi decode with qualities and moves (xb_decode_q), and with per-base letter probabilities (xb_decode_ub):
    #      extensions, parity unpinned ----------
    def _decode_level(self, level, scores, alphabet, qscale, qoffset, has_blank):
        scores, has_blank = self._scores(scores, has_blank)
        T, n, _ = scores.shape
        out = self._outputs(level, n, T)
        fn = (self.lib.xb_decode_q, self.lib.xb_decode_ub)[level - 1]
        self._check(fn(self.h, scores.ctypes.data, T, n, has_blank, "".join(alphabet).encode(), float(qscale), float(qoffset),
                       *_lens_last(out)))
        return out

    def decode_q(self, scores, alphabet, qscale=1.0, qoffset=0.0, has_blank=None):
        """xb_decode_q: scores (T, n, C) -> (seq (n, T) int8, lens (n,), qstring (n, T) int8 left-packed beside seq,
        moves (n, T) uint8)."""
        return self._decode_level(1, scores, alphabet, qscale, qoffset, has_blank)

    def decode_ub(self, scores, alphabet, qscale=1.0, qoffset=0.0, has_blank=None):
        """xb_decode_ub: scores (T, n, C) -> (seq, lens, qstring, moves) as decode_q returns them, plus probs (n, nb, T)
        uint8: plane b holds the probability byte of letter alphabet[1 + b] per base, left-packed beside seq."""
        return self._decode_level(2, scores, alphabet, qscale, qoffset, has_blank)

    def decode_q_dev(self, d_scores, T, n, has_blank, alphabet, qscale, qoffset, d_seq, d_qstring, d_moves, d_len):
        self._check(self.lib.xb_decode_q_dev(self.h, _ptr(d_scores), int(T), int(n), int(bool(has_blank)),
                                             "".join(alphabet).encode(), float(qscale), float(qoffset), _ptr(d_seq),
                                             _ptr(d_qstring), _ptr(d_moves), _ptr(d_len)))

    def decode_ub_dev(self, d_scores, T, n, has_blank, alphabet, qscale, qoffset, d_seq, d_qstring, d_moves, d_probs, d_len):
        self._check(self.lib.xb_decode_ub_dev(self.h, _ptr(d_scores), int(T), int(n), int(bool(has_blank)),
                                              "".join(alphabet).encode(), float(qscale), float(qoffset), _ptr(d_seq),
                                              _ptr(d_qstring), _ptr(d_moves), _ptr(d_probs), _ptr(d_len)))

    def basecall_chunks_q(self, signal, alphabet, qscale=1.0, qoffset=0.0):
        """xb_basecall_chunks_q: signal (n, chunk_len) -> (seq, lens, qstring, moves) as decode_q returns them."""
        return self.basecall_chunks(signal, alphabet, qscale, qoffset, level=1)

    def basecall_chunks_ub(self, signal, alphabet, qscale=1.0, qoffset=0.0):
        """xb_basecall_chunks_ub: signal (n, chunk_len) -> (seq, lens, qstring, moves, probs) as decode_ub returns them."""
        return self.basecall_chunks(signal, alphabet, qscale, qoffset, level=2)

    def submit_chunks_q(self, slot, signal, alphabet, qscale=1.0, qoffset=0.0):
        return self.submit_chunks(slot, signal, alphabet, qscale, qoffset, level=1)

    def collect_chunks_q(self, slot, n):
        return self.collect_chunks(slot, n, level=1)

    def submit_chunks_ub(self, slot, signal, alphabet, qscale=1.0, qoffset=0.0):
        return self.submit_chunks(slot, signal, alphabet, qscale, qoffset, level=2)

    def collect_chunks_ub(self, slot, n):
        return self.collect_chunks(slot, n, level=2)

    # ---- beam search with qualities and moves (koi.decode.beam_search at crf/basecall.py:43-46) ----------
    def _beam_out(self, n, T):
        return (np.empty((n, T), dtype=np.int8), np.empty((n, T), dtype=np.int8), np.empty((n, T), dtype=np.uint8),
                np.empty((n,), dtype=np.float32))

    def beam_search(self, scores, alphabet, beam_width=32, beam_cut=100.0, scale=1.0, offset=0.0):
        """xb_beam_search: scores (T, n, C_noblank | C_blank) -> {'sequence', 'qstring' (n, T) int8, 'moves' (n, T) uint8,
        'score' (n,)}; the stay score of blank-less scores is the context's blank_score."""
        scores = np.ascontiguousarray(scores, dtype=np.float32)
        T, n, Cin = scores.shape
        if Cin not in (self.C_blank, self.C_noblank):
            raise ValueError("scores last dim %d matches neither %d nor %d" % (Cin, self.C_blank, self.C_noblank))
        seq, q, mv, sc = self._beam_out(n, T)
        self._check(self.lib.xb_beam_search(self.h, scores.ctypes.data, T, n, int(Cin == self.C_blank), "".join(alphabet).encode(),
                                            int(beam_width), float(beam_cut), float(scale), float(offset), seq.ctypes.data,
                                            q.ctypes.data, mv.ctypes.data, sc.ctypes.data))
        return {"sequence": seq, "qstring": q, "moves": mv, "score": sc}

    def basecall_chunks_beam(self, signal, alphabet, beam_width=32, beam_cut=100.0, scale=1.0, offset=0.0):
        """xb_basecall_chunks_beam: signal (n, chunk_len) -> the same dict as beam_search, scores never leave the device."""
        signal = np.ascontiguousarray(signal, dtype=np.float32).reshape(-1, self.chunk_len)
        n = signal.shape[0]
        seq, q, mv, sc = self._beam_out(n, self.T)
        self._check(self.lib.xb_basecall_chunks_beam(self.h, signal.ctypes.data, n, "".join(alphabet).encode(), int(beam_width),
                                                     float(beam_cut), float(scale), float(offset), seq.ctypes.data, q.ctypes.data,
                                                     mv.ctypes.data, sc.ctypes.data))
        return {"sequence": seq, "qstring": q, "moves": mv, "score": sc}

    def beam_search_dev(self, d_scores, T, n, has_blank, alphabet, d_sequence, d_qstring, d_moves, d_score=None, beam_width=32,
                        beam_cut=100.0, scale=1.0, offset=0.0):
        self._check(self.lib.xb_beam_search_dev(self.h, _ptr(d_scores), int(T), int(n), int(bool(has_blank)),
                                                "".join(alphabet).encode(), int(beam_width), float(beam_cut), float(scale),
                                                float(offset), _ptr(d_sequence), _ptr(d_qstring), _ptr(d_moves), _ptr(d_score)))

    # ---- template mapper (xb_map_templates): an extension, parity unpinned ----------
    MAP_OUTPUTS = (("tmpl", np.int32), ("strand", np.int8), ("score", np.int32), ("second", np.int32), ("q_st", np.int32),
                   ("q_en", np.int32), ("r_st", np.int32), ("r_en", np.int32), ("ops", np.uint8), ("n_ops", np.int32))

    def map_templates(self, seq, seq_len, templates, offsets, scoring=(2, 4, 4, 2, 1)):
        """xb_map_templates: seq (n, W) int8 left-packed rows and seq_len (n) against the library `templates` (its letters
        concatenated, bytes) with `offsets` (R + 1) -> dict of the outputs named in MAP_OUTPUTS; ops is (n, W + Lmax)."""
        seq = np.ascontiguousarray(seq, dtype=np.int8)
        lens = np.ascontiguousarray(seq_len, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        n, W = seq.shape
        lmax = int(np.diff(off).max()) if off.size > 1 else 0
        out = {k: np.empty((n, W + lmax) if k == "ops" else (n,), dtype=dt) for k, dt in self.MAP_OUTPUTS}
        self._check(self.lib.xb_map_templates(self.h, seq.ctypes.data, lens.ctypes.data, n, W, bytes(templates), off.ctypes.data,
                                              off.size - 1, *[int(v) for v in scoring], *[out[k].ctypes.data for k, _ in self.MAP_OUTPUTS]))
        return out

    def map_templates_dev(self, d_seq, d_seq_len, n, W, templates, offsets, scoring, d_out):
        """xb_map_templates_dev: device pointers for the rows and for the outputs (d_out: name -> pointer, MAP_OUTPUTS)."""
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        self._check(self.lib.xb_map_templates_dev(self.h, _ptr(d_seq), _ptr(d_seq_len), int(n), int(W), bytes(templates),
                                                  off.ctypes.data, off.size - 1, *[int(v) for v in scoring],
                                                  *[_ptr(d_out[k]) for k, _ in self.MAP_OUTPUTS]))

    # ---- ctc-data labels of mapped rows (xb_ctc_targets, xb_ctc_chunks): parity unpinned ----------
    CTC_INPUTS = ("tmpl", "strand", "q_st", "q_en", "r_st", "r_en", "ops", "n_ops")
    CTC_OUTPUTS = (("mlen", np.int32), ("blen", np.int32), ("verdict", np.uint8), ("target", np.uint8), ("target_len", np.int32))
    FAILED_SEQ, FAILED_MAP, SKIPPED_NON_UB, FAILED_ACC, FAILED_COV = 1, 2, 4, 8, 16      # the bits of verdict

    @staticmethod
    def ctc_target_width(offsets):
        """Bytes per label row: the longest template rounded up to a multiple of 16."""
        return -(-int(np.diff(np.asarray(offsets)).max()) // 16) * 16

    def _ctc_out(self, n, offsets):
        tw = self.ctc_target_width(offsets)
        return {k: np.empty((n, tw) if k == "target" else (n,), dtype=dt) for k, dt in self.CTC_OUTPUTS}

    def ctc_targets(self, seq_len, width, mapped, templates, offsets, min_accuracy=0.95, min_coverage=0.90, ub_only=False,
                    ub_plus=5, ub_minus=6):
        """xb_ctc_targets: seq_len (n) and the mapper's outputs `mapped` (map_templates' dict, rows of `width`) -> dict of mlen,
        blen, verdict (n), target (n, TW) uint8 zero-filled behind target_len, target_len (CTC_OUTPUTS)."""
        lens = np.ascontiguousarray(seq_len, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        n = lens.shape[0]
        dts = dict(self.MAP_OUTPUTS)
        ins = [np.ascontiguousarray(mapped[k], dtype=dts[k]) for k in self.CTC_INPUTS]
        if ins[6].shape != (n, int(width) + int(np.diff(off).max())):
            raise ValueError("ctc_targets: ops is %s, (n, width + longest template) expected" % (ins[6].shape,))
        out = self._ctc_out(n, off)
        self._check(self.lib.xb_ctc_targets(self.h, lens.ctypes.data, n, int(width), bytes(templates), off.ctypes.data, off.size - 1,
                                            *[a.ctypes.data for a in ins], float(min_accuracy), float(min_coverage),
                                            int(bool(ub_only)), int(ub_plus), int(ub_minus),
                                            *[out[k].ctypes.data for k, _ in self.CTC_OUTPUTS]))
        return out

    def ctc_targets_dev(self, d_seq_len, n, width, d_mapped, templates, offsets, d_out, min_accuracy=0.95, min_coverage=0.90,
                        ub_only=False, ub_plus=5, ub_minus=6):
        """xb_ctc_targets_dev: device pointers for seq_len, the mapper's outputs (d_mapped: name -> pointer, CTC_INPUTS) and the
        outputs (d_out: name -> pointer, CTC_OUTPUTS; target 16-byte aligned); returns without waiting."""
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        self._check(self.lib.xb_ctc_targets_dev(self.h, _ptr(d_seq_len), int(n), int(width), bytes(templates), off.ctypes.data,
                                                off.size - 1, *[_ptr(d_mapped[k]) for k in self.CTC_INPUTS], float(min_accuracy),
                                                float(min_coverage), int(bool(ub_only)), int(ub_plus), int(ub_minus),
                                                *[_ptr(d_out[k]) for k, _ in self.CTC_OUTPUTS]))

    def ctc_chunks(self, signal, alphabet, templates, offsets, scoring=(2, 4, 4, 2, 1), min_accuracy=0.95, min_coverage=0.90,
                   ub_only=False, ub_plus=5, ub_minus=6):
        """xb_ctc_chunks: signal (n, chunk_len) -> dict of seq (n, T) int8, seq_len, every MAP_OUTPUTS array (ops (n, T + Lmax))
        and every CTC_OUTPUTS array: the Viterbi basecall, the mapper and the labels in one device pass."""
        signal = np.ascontiguousarray(signal, dtype=np.float32).reshape(-1, self.chunk_len)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        n = signal.shape[0]
        lmax = int(np.diff(off).max())
        out = {"seq": np.empty((n, self.T), np.int8), "seq_len": np.empty((n,), np.int32)}
        out.update({k: np.empty((n, self.T + lmax) if k == "ops" else (n,), dtype=dt) for k, dt in self.MAP_OUTPUTS})
        out.update(self._ctc_out(n, off))
        self._check(self.lib.xb_ctc_chunks(self.h, signal.ctypes.data, n, "".join(alphabet).encode(), bytes(templates),
                                           off.ctypes.data, off.size - 1, *[int(v) for v in scoring], float(min_accuracy),
                                           float(min_coverage), int(bool(ub_only)), int(ub_plus), int(ub_minus),
                                           out["seq"].ctypes.data, out["seq_len"].ctypes.data,
                                           *[out[k].ctypes.data for k, _ in self.MAP_OUTPUTS],
                                           *[out[k].ctypes.data for k, _ in self.CTC_OUTPUTS]))
        return out

    # ---- per-position UB accuracy of mapped rows (xb_ub_tally): parity unpinned ----------
    UB_INPUTS = ("tmpl", "strand", "q_st", "r_st", "r_en", "ops", "n_ops")
    UB_COUNTS = ("n_match", "ub_matches", "ub_len", "ub_area_matches", "ub_area_len", "non_ub_area_matches", "non_ub_area_len",
                 "ubs_detected")

    def ub_tally(self, rows, lens, got, library, offsets, acc=None):
        """xb_ub_tally: the rows the mapper saw (rows (n, W) int8, lens (n)) and its outputs `got` (map_templates' dict) ->
        (counts (n, 8) int32 in the order UB_COUNTS, acc): acc is a UbAccumulators (a fresh one when None) that this call has
        added to, to be passed on from call to call."""
        rows = np.ascontiguousarray(rows, dtype=np.int8)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        n, W = rows.shape
        acc = UbAccumulators(off) if acc is None else acc
        if acc.err.shape != (2, int(off[-1])) or acc.reads.shape != (off.size - 1, 2):
            raise ValueError("ub_tally: the accumulators belong to another library")
        dts = dict(self.MAP_OUTPUTS)
        ins = [np.ascontiguousarray(got[k], dtype=dts[k]) for k in self.UB_INPUTS]
        if lens.shape != (n,) or ins[5].shape != (n, W + int(np.diff(off).max())):
            raise ValueError("ub_tally: ops is %s, (n, width + longest template) expected" % (ins[5].shape,))
        counts = np.empty((n, len(self.UB_COUNTS)), np.int32)
        self._check(self.lib.xb_ub_tally(self.h, rows.ctypes.data, lens.ctypes.data, n, W, bytes(library), off.ctypes.data, off.size - 1,
                                         *[a.ctypes.data for a in ins], counts.ctypes.data, acc.reads.ctypes.data,
                                         acc.err.ctypes.data, acc.cm.ctypes.data))
        return counts, acc

    def ub_tally_dev(self, d_rows, d_lens, n, width, d_got, library, offsets, d_counts, d_reads, d_err, d_cm):
        """xb_ub_tally_dev: device pointers for the rows, the mapper's outputs (d_got: name -> pointer, UB_INPUTS), counts and
        the three accumulators; returns without waiting."""
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        self._check(self.lib.xb_ub_tally_dev(self.h, _ptr(d_rows), _ptr(d_lens), int(n), int(width), bytes(library), off.ctypes.data,
                                             off.size - 1, *[_ptr(d_got[k]) for k in self.UB_INPUTS], _ptr(d_counts), _ptr(d_reads),
                                             _ptr(d_err), _ptr(d_cm)))

    # ---- barcode distance of mapped rows (xb_barcode_dist): the per-row function pinned, the mapping unpinned ----------
    BC_INPUTS = ("tmpl", "strand", "q_st", "r_st")
    BC_OUTPUTS = ("bc_dist", "bc_start", "bc_end", "bc_obs_len")

    def barcode_dist(self, rows, lens, got, library, offsets, bc_pos, bc_len, relax=3):
        """xb_barcode_dist: the rows the mapper saw (rows (n, W) int8, lens (n)) and its outputs `got` (map_templates' dict) ->
        dict of bc_dist (-1 for an unmapped row), bc_start, bc_end, bc_obs_len, (n) int32 each (BC_OUTPUTS)."""
        rows = np.ascontiguousarray(rows, dtype=np.int8)
        lens = np.ascontiguousarray(lens, dtype=np.int32)
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        n, W = rows.shape
        dts = dict(self.MAP_OUTPUTS)
        ins = [np.ascontiguousarray(got[k], dtype=dts[k]) for k in self.BC_INPUTS]
        if lens.shape != (n,) or any(a.shape != (n,) for a in ins):
            raise ValueError("barcode_dist: %d rows, but lens and the mapper's outputs are %s" % (n, [lens.shape] + [a.shape for a in ins]))
        out = {k: np.empty((n,), np.int32) for k in self.BC_OUTPUTS}
        self._check(self.lib.xb_barcode_dist(self.h, rows.ctypes.data, lens.ctypes.data, n, W, bytes(library), off.ctypes.data,
                                             off.size - 1, *[a.ctypes.data for a in ins], int(bc_pos), int(bc_len), int(relax),
                                             *[out[k].ctypes.data for k in self.BC_OUTPUTS]))
        return out

    def barcode_dist_dev(self, d_rows, d_lens, n, width, d_got, library, offsets, bc_pos, bc_len, relax, d_out):
        """xb_barcode_dist_dev: device pointers for the rows, the mapper's outputs (d_got: name -> pointer, BC_INPUTS) and the
        outputs (d_out: name -> pointer, BC_OUTPUTS); returns without waiting."""
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        self._check(self.lib.xb_barcode_dist_dev(self.h, _ptr(d_rows), _ptr(d_lens), int(n), int(width), bytes(library),
                                                 off.ctypes.data, off.size - 1, *[_ptr(d_got[k]) for k in self.BC_INPUTS],
                                                 int(bc_pos), int(bc_len), int(relax), *[_ptr(d_out[k]) for k in self.BC_OUTPUTS]))

    # ---- DTW signal segmentation (xb_dtw_segment): an extension, parity unpinned ----------
    @staticmethod
    def _dtw_offsets(levels):
        """A list of per-chunk level arrays -> (their float64 concatenation, int32 offsets (n + 1))."""
        off = np.zeros(len(levels) + 1, np.int32)
        off[1:] = np.cumsum([len(v) for v in levels])
        flat = np.ascontiguousarray(np.concatenate([np.asarray(v, np.float64).ravel() for v in levels]) if len(levels) else [],
                                    dtype=np.float64)
        return flat, off

    def dtw_segment(self, signal, levels, ref_rep=3, window=None, kmax=None):
        """xb_dtw_segment: signal (n, N) fp32 and per chunk its float64 levels (a list of arrays, before repetition) ->
        (breakpoints (n, kmax) int32 zero-filled behind each chunk's levels, ok (n,) bool, cost (n,) float64).  window: None
        or (n,) float64 half-widths of the slanted band in columns, negative = none."""
        signal = np.ascontiguousarray(signal, dtype=np.float32)
        n, N = signal.shape
        flat, off = self._dtw_offsets(levels)
        if len(levels) != n:
            raise ValueError("dtw_segment: %d chunks, %d level arrays" % (n, len(levels)))
        kmax = int(kmax if kmax is not None else max(1, int(np.diff(off).max()) if n else 1))
        win = None if window is None else np.ascontiguousarray(window, dtype=np.float64).reshape(n)
        bp = np.empty((n, kmax), np.int32)
        ok = np.empty((n,), np.int8)
        cost = np.empty((n,), np.float64)
        self._check(self.lib.xb_dtw_segment(self.h, signal.ctypes.data, n, N, flat.ctypes.data, off.ctypes.data, int(ref_rep),
                                            _ptr(win), kmax, bp.ctypes.data, ok.ctypes.data, cost.ctypes.data))
        return bp, ok.astype(bool), cost

    def dtw_segment_dev(self, d_signal, n, N, d_levels, offsets, ref_rep, d_window, kmax, d_breakpoints, d_ok, d_cost):
        """xb_dtw_segment_dev: device pointers but for `offsets` (host, (n + 1) int32); returns without waiting."""
        off = np.ascontiguousarray(offsets, dtype=np.int32)
        self._check(self.lib.xb_dtw_segment_dev(self.h, _ptr(d_signal), int(n), int(N), _ptr(d_levels), off.ctypes.data, int(ref_rep),
                                                _ptr(d_window), int(kmax), _ptr(d_breakpoints), _ptr(d_ok), _ptr(d_cost)))

    def dtw_scratch_bytes(self):
        """Choice-bit bytes the launches of the last dtw_segment call wrote (xb_dtw_scratch_bytes)."""
        return int(self.lib.xb_dtw_scratch_bytes(self.h))

    # ---- XNA spliced augmentation (xb_splice_library, xb_splice_chunks): draws parity unpinned ----------
    def splice_library(self, pool, rows, table):
        """xb_splice_library: pool float16, rows (n_rows, 2) int32 pool offset and length, table (2 * 7^5 * 6, 2) int32 first row
        and count (splice.Library's arrays); replaces the library of an earlier call."""
        pool = np.ascontiguousarray(pool, dtype=np.float16)
        rows = np.ascontiguousarray(rows, dtype=np.int32).reshape(-1, 2)
        table = np.ascontiguousarray(table, dtype=np.int32).reshape(-1, 2)
        self._check(self.lib.xb_splice_library(self.h, pool.ctypes.data, pool.size, rows.ctypes.data, rows.shape[0],
                                               table.ctypes.data, table.shape[0]))

    def splice_chunks(self, signal, targets, lengths, breakpoints, first_index, seed, ubs_mask, prop, var_prop=0.0,
                      cand_sample_size=10, pad=5):
        """xb_splice_chunks: signal (n, N) fp32, targets (n, Lt) uint8, lengths (n), breakpoints (n, Lt) uint16 ->
        (signal (n, N) float32, targets (n, Lt) uint8, success (n,) int8, inserted (n,) int32)."""
        signal = np.ascontiguousarray(signal, dtype=np.float32)
        targets = np.ascontiguousarray(targets, dtype=np.uint8)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        bk = np.ascontiguousarray(breakpoints, dtype=np.uint16)
        n, N = signal.shape
        if targets.ndim != 2 or targets.shape[0] != n or bk.shape != targets.shape or lengths.shape != (n,):
            raise ValueError("splice_chunks: signal (n, N), targets (n, Lt), lengths (n), breakpoints (n, Lt) expected")
        out, out_t = np.empty_like(signal), np.empty_like(targets)
        ok, ins = np.empty((n,), np.int8), np.empty((n,), np.int32)
        self._check(self.lib.xb_splice_chunks(self.h, signal.ctypes.data, targets.ctypes.data, lengths.ctypes.data, bk.ctypes.data,
                                              n, N, targets.shape[1], int(first_index), int(seed) & (2 ** 64 - 1), int(ubs_mask),
                                              float(prop), float(var_prop or 0.0), int(cand_sample_size), int(pad), out.ctypes.data,
                                              out_t.ctypes.data, ok.ctypes.data, ins.ctypes.data))
        return out, out_t, ok, ins

    def splice_chunks_dev(self, d_signal, d_targets, d_lengths, d_breakpoints, n, N, Lt, first_index, seed, ubs_mask, prop, var_prop,
                          cand_sample_size, pad, d_out_signal, d_out_targets, d_success, d_inserted):
        """xb_splice_chunks_dev: device pointers; returns without waiting."""
        self._check(self.lib.xb_splice_chunks_dev(self.h, _ptr(d_signal), _ptr(d_targets), _ptr(d_lengths), _ptr(d_breakpoints),
                                                  int(n), int(N), int(Lt), int(first_index), int(seed) & (2 ** 64 - 1), int(ubs_mask),
                                                  float(prop), float(var_prop or 0.0), int(cand_sample_size), int(pad),
                                                  _ptr(d_out_signal), _ptr(d_out_targets), _ptr(d_success), _ptr(d_inserted)))

    # ---- XNA synthetic spiking (xb_spike_model, xb_spike_chunks): draws parity unpinned ----------
    def spike_model(self, mean, stdv):
        """xb_spike_model: (7^6,) float64 level means (NaN: no such k-mer) and stdvs (spike.model_table's arrays); replaces the
        table of an earlier call."""
        mean = np.ascontiguousarray(mean, dtype=np.float64).reshape(-1)
        stdv = np.ascontiguousarray(stdv, dtype=np.float64).reshape(-1)
        if mean.shape != stdv.shape:
            raise ValueError("spike_model: mean and stdv of one shape expected")
        self._check(self.lib.xb_spike_model(self.h, mean.ctypes.data, stdv.ctypes.data, mean.size))

    @staticmethod
    def _spike_phi(phi, dist_rows):
        phi = np.ascontiguousarray(np.zeros((1, 2)) if phi is None else phi, dtype=np.float64).reshape(-1, 2)
        if phi.shape[0] < int(dist_rows) + 1:
            raise ValueError("spike_chunks: a distribution table of %d rows, dist_rows + 1 = %d expected" % (phi.shape[0], dist_rows + 1))
        return phi

    def _spike_call(self, fn, name, signal, targets, lengths, breakpoints, first_index, seed, ubs_mask, prop, var_prop, pad, dist_rows,
                    phi, noise_std, variable_noise):
        signal = np.ascontiguousarray(signal, dtype=np.float32)
        targets = np.ascontiguousarray(targets, dtype=np.uint8)
        lengths = np.ascontiguousarray(lengths, dtype=np.int32)
        bk = np.ascontiguousarray(breakpoints, dtype=np.uint16)
        n, N = signal.shape
        if targets.ndim != 2 or targets.shape[0] != n or bk.shape != targets.shape or lengths.shape != (n,):
            raise ValueError("%s: signal (n, N), targets (n, Lt), lengths (n), breakpoints (n, Lt) expected" % name)
        phi = self._spike_phi(phi, dist_rows)
        out, out_t = np.empty_like(signal), np.empty_like(targets)
        spiked, status = np.empty((n,), np.int32), np.empty((n,), np.int8)
        med, mad = np.empty((n,), np.float64), np.empty((n,), np.float64)
        self._check(fn(self.h, signal.ctypes.data, targets.ctypes.data, lengths.ctypes.data, bk.ctypes.data, n, N, targets.shape[1],
                       int(first_index), int(seed) & (2 ** 64 - 1), int(ubs_mask), float(prop), float(var_prop or 0.0), int(pad),
                       int(dist_rows), phi.ctypes.data, float(noise_std), int(bool(variable_noise)), out.ctypes.data,
                       out_t.ctypes.data, spiked.ctypes.data, med.ctypes.data, mad.ctypes.data, status.ctypes.data))
        return out, out_t, spiked, med, mad, status

    def _spike_call_dev(self, fn, d_signal, d_targets, d_lengths, d_breakpoints, n, N, Lt, first_index, seed, ubs_mask, prop, var_prop,
                        pad, dist_rows, phi, noise_std, variable_noise, d_out_signal, d_out_targets, d_spiked, d_med, d_mad, d_status):
        phi = self._spike_phi(phi, dist_rows)
        self._check(fn(self.h, _ptr(d_signal), _ptr(d_targets), _ptr(d_lengths), _ptr(d_breakpoints), int(n), int(N), int(Lt),
                       int(first_index), int(seed) & (2 ** 64 - 1), int(ubs_mask), float(prop), float(var_prop or 0.0), int(pad),
                       int(dist_rows), phi.ctypes.data, float(noise_std), int(bool(variable_noise)), _ptr(d_out_signal),
                       _ptr(d_out_targets), _ptr(d_spiked), _ptr(d_med), _ptr(d_mad), _ptr(d_status)))

    def spike_chunks(self, signal, targets, lengths, breakpoints, first_index, seed, ubs_mask, prop, var_prop=0.0, pad=5,
                     dist_rows=0, phi=None, noise_std=0.0, variable_noise=False):
        """xb_spike_chunks: signal (n, N) fp32, targets (n, Lt) uint8, lengths (n), breakpoints (n, Lt) uint16, phi
        (dist_rows + 1, 2) float64 -> (signal (n, N) float32, targets (n, Lt) uint8, spiked (n,) int32, med (n,), mad (n,)
        float64, status (n,) int8)."""
        return self._spike_call(self.lib.xb_spike_chunks, "spike_chunks", signal, targets, lengths, breakpoints, first_index, seed,
                                ubs_mask, prop, var_prop, pad, dist_rows, phi, noise_std, variable_noise)

    def spike_chunks_dev(self, *args):
        """xb_spike_chunks_dev(d_signal, d_targets, d_lengths, d_breakpoints, n, N, Lt, first_index, seed, ubs_mask, prop, var_prop,
        pad, dist_rows, phi, noise_std, variable_noise, d_out_signal, d_out_targets, d_spiked, d_med, d_mad, d_status): device
        pointers but for `phi` (host); returns without waiting."""
        self._spike_call_dev(self.lib.xb_spike_chunks_dev, *args)

    # ---- XNA fully synthetic chunks (xb_synth_chunks): xb_spike_chunks' arguments and model, the whole chunk synthesised ----------
    def synth_chunks(self, signal, targets, lengths, breakpoints, first_index, seed, ubs_mask, prop, var_prop=0.0, pad=5,
                     dist_rows=0, phi=None, noise_std=0.0, variable_noise=False):
        """xb_synth_chunks: what spike_chunks takes and returns; every sample below a chunk's last breakpoint is synthesised
        from the spiked labels, and `spiked` may be 0 with the chunk still synthesised."""
        return self._spike_call(self.lib.xb_synth_chunks, "synth_chunks", signal, targets, lengths, breakpoints, first_index, seed,
                                ubs_mask, prop, var_prop, pad, dist_rows, phi, noise_std, variable_noise)

    def synth_chunks_dev(self, *args):
        """xb_synth_chunks_dev: spike_chunks_dev's arguments; returns without waiting."""
        self._spike_call_dev(self.lib.xb_synth_chunks_dev, *args)

    # ---- host pipeline: two batches in flight (xb_submit_chunks / xb_collect_chunks) ----------
    def submit_chunks(self, slot, signal, alphabet, qscale=1.0, qoffset=0.0, level=0):
        """Enqueue the basecall of signal at an output level in pipeline slot `slot` (xb_submit_chunks[_q|_ub]); returns n."""
        signal = np.ascontiguousarray(signal, dtype=np.float32).reshape(-1, self.chunk_len)
        fn = (self.lib.xb_submit_chunks, self.lib.xb_submit_chunks_q, self.lib.xb_submit_chunks_ub)[level]
        self._check(fn(self.h, int(slot), signal.ctypes.data, signal.shape[0], "".join(alphabet).encode(),
                       *_calib(level, qscale, qoffset)))
        return signal.shape[0]

    def collect_chunks(self, slot, n, level=0):
        """The outputs of a level (basecall_chunks' tuple) of slot's submission, made at that level or above."""
        out = self._outputs(level, n, self.T)
        fn = (self.lib.xb_collect_chunks, self.lib.xb_collect_chunks_q, self.lib.xb_collect_chunks_ub)[level]
        self._check(fn(self.h, int(slot), *[_ptr(a) for a in out]))
        return out

    # ---- device-pointer operators (pointers are ints, e.g. torch data_ptr()) -----------------
    def encode_dev(self, d_signal, n, expand_blanks, d_scores):
        self._check(self.lib.xb_encode_dev(self.h, _ptr(d_signal), n, int(bool(expand_blanks)), _ptr(d_scores)))

    def decode_dev(self, d_scores, T, n, has_blank, alphabet, d_labels, d_seq, d_len):
        ab = None if alphabet is None else "".join(alphabet).encode()
        self._check(self.lib.xb_decode_dev(self.h, _ptr(d_scores), T, n, int(bool(has_blank)), ab,
                                           _ptr(d_labels), _ptr(d_seq), _ptr(d_len)))

    def basecall_chunks_dev(self, d_signal, n, alphabet, d_seq, d_len):
        self._check(self.lib.xb_basecall_chunks_dev(self.h, _ptr(d_signal), n, "".join(alphabet).encode(),
                                                    _ptr(d_seq), _ptr(d_len)))

    def synchronize(self):
        self._check(self.lib.xb_synchronize(self.h))

    def reserve_pairing(self):
        """Opt in to the co-scheduling of two asynchronous calls in flight (xb_reserve_pairing: allocates the workspaces for a
        pair); returns whether the context pairs calls from now on."""
        self._check(self.lib.xb_reserve_pairing(self.h))
        return self.pairing_active()

    def pairing_active(self):
        return bool(self.lib.xb_pairing_active(self.h))

    def result_stream(self):
        """hipStream_t (int) producing the outputs of the most recent *_dev call (xb_result_stream)."""
        return int(self.lib.xb_result_stream(self.h) or 0)

    def set_profiling(self, on):
        self._check(self.lib.xb_set_profiling(self.h, int(bool(on))))

    def reset_stage_times(self):
        self._check(self.lib.xb_reset_stage_times(self.h))

    def stage_times(self):
        ms = (C.c_float * 5)()
        ln = (C.c_int64 * 5)()
        self._check(self.lib.xb_get_stage_times(self.h, ms, ln))
        return {k: (float(ms[i]), int(ln[i])) for i, k in enumerate(XB_STAGE_NAMES)}


def mapper_context(device=0):
    """A Context for the entry points that need no model (xb_map_templates, xb_ctc_targets, xb_ub_tally, xb_barcode_dist):
    xb_ctx_create wants a model geometry, so this is the smallest one it accepts -- 4 bases, 32 features, one chunk of 200
    samples -- and no weights are ever loaded into it."""
    return Context(device, 4, 3, 32, 19, 5, 5.0, 2.0, 200, 1)


class Comm:
    """xb_comm: the RCCL communicator of the path's one collective (include/xna_basecaller.h, 'multi-GPU').  Rank 0 draws
    the id with Comm.unique_id() and passes it to the other ranks out of band (dist.exchange_comm_id)."""

    def __init__(self, device, rank, world, comm_id):
        self.lib = load()
        if len(comm_id) != XB_COMM_ID_BYTES:
            raise ValueError("communicator id must be %d bytes" % XB_COMM_ID_BYTES)
        h = C.c_void_p()
        rc = self.lib.xb_comm_create(C.byref(h), int(device), int(rank), int(world), bytes(comm_id))
        if rc:
            raise XbError(rc, (self.lib.xb_comm_last_error(None) or b"").decode())
        self.h, self.rank, self.world = h, int(rank), int(world)

    @staticmethod
    def unique_id():
        lib = load()
        buf = C.create_string_buffer(XB_COMM_ID_BYTES)
        rc = lib.xb_comm_unique_id(buf)
        if rc:
            raise XbError(rc, (lib.xb_comm_last_error(None) or b"").decode())
        return buf.raw

    def _check(self, rc):
        if rc:
            raise XbError(rc, (self.lib.xb_comm_last_error(self.h) or b"").decode())

    def gather_called(self, ctx, d_seq, d_len, n, T, d_all_seq, d_all_len):
        """All-gather of one batch on the communicator's stream, behind ctx's result stream (device pointers as ints)."""
        self._check(self.lib.xb_gather_called(self.h, ctx.h if ctx is not None else None, _ptr(d_seq), _ptr(d_len), int(n), int(T),
                                              _ptr(d_all_seq), _ptr(d_all_len)))

    def fence(self, ctx, lag=0):
        self._check(self.lib.xb_comm_fence(self.h, ctx.h, int(lag)))

    def synchronize(self):
        self._check(self.lib.xb_comm_synchronize(self.h))

    def close(self):
        if self.h:
            self.lib.xb_comm_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass
