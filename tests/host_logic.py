"""ctypes view of libxnacall.so's non-public host-logic exports (xb_internal_*, csrc/xb_api.hip): the encoder's planner
(csrc/xb_schedule.h), the weight packer (csrc/xb_pack.h), the decoder of the device status words (csrc/xb_status.h) and the
CTC lattice kernels' column and launch rules (csrc/xb_ctc_lattice.h).  None
of them touches the device or needs a context, so the tests that use this module run without a GPU."""
import ctypes as C

import numpy as np

from xna_basecaller_amd import _lib

# xb::Knobs, field by field, and the environment variable behind each
KNOBS = (("lstm_mode", "XB_LSTM_MODE"), ("lstm_dual", "XB_LSTM_DUAL"), ("lstm_wide", "XB_LSTM_WIDE"),
         ("lstm_local", "XB_LSTM_LOCAL"), ("lstm_signal", "XB_LSTM_SIGNAL"), ("lstm_i8", "XB_LSTM_I8"),
         ("overlap", "XB_OVERLAP"), ("time_slabs", "XB_TIME_SLABS"), ("slab_steps", "XB_SLAB_STEPS"), ("fuse", "XB_FUSE"),
         ("decode_async", "XB_DECODE_ASYNC"), ("in1_layers", "XB_IN1_LAYERS"), ("x3_stages", "XB_X3_STAGES"),
         ("gemm4", "XB_GEMM4"), ("gemm_sn", "XB_GEMM_SN"), ("gemm_shadow_kernel", "XB_GEMM_SHADOW"),
         ("gemm_shadow_wgs", "XB_GEMM_SHADOW_WGS"))
SERIAL, EVENTS, SIGNAL, SLABS_SERIAL_GEMM = 0, 1, 2, 3         # xb::PlanOrdering
ORDERING_TAGS = ("serial", "events", "signal", "slabs-serial-gemm")
LAUNCH_FIELDS = ("n0", "nslab", "s_begin", "s_end", "dual", "grp0", "slab", "xcd_local", "sync_base")   # xb::PlanLaunch
MAX_LAUNCHES = 8192


class Knobs(C.Structure):
    _fields_ = [(f, C.c_int) for f, _ in KNOBS]


class PlanQuery(C.Structure):
    _fields_ = [("F", C.c_int), ("n", C.c_int), ("T", C.c_int), ("cu_count", C.c_int), ("knobs", Knobs),
                ("spread", C.c_int), ("has_next", C.c_int), ("resident1", C.c_int), ("resident2", C.c_int),
                ("signal_ok", C.c_int)]


class LayerPlan(C.Structure):
    _fields_ = [("error", C.c_int), ("message", C.c_char * 160)] + [(f, C.c_int) for f in (
        "mode", "wide", "spread", "dual_batch", "gslab", "slab", "global_groups", "nts", "chunk_slabs", "ordering",
        "rec_launches", "gemm_slabs", "n", "T", "lstm_dual", "dual_ok", "lstm_local")]


_cached = None


def lib():
    global _cached
    if _cached is None:
        so = C.CDLL(_lib.LIB_PATH)
        vp, ip = C.c_void_p, C.c_int
        so.xb_internal_knobs_from_env.argtypes = [C.POINTER(Knobs)]
        so.xb_internal_knobs_from_env.restype = None
        so.xb_internal_pair_capacity.argtypes = [ip, ip, ip]
        so.xb_internal_plan_layer.argtypes = [C.POINTER(PlanQuery), C.POINTER(LayerPlan), vp, ip]
        so.xb_internal_f32_to_e4m3.argtypes = [C.c_float]
        so.xb_internal_split_rows.argtypes = [vp, ip, ip, ip, vp, vp, C.POINTER(ip)]
        so.xb_internal_split_rows.restype = None
        so.xb_internal_fragment_major.argtypes = [vp, vp, ip, ip, ip, ip, vp, C.c_size_t, C.POINTER(C.c_size_t)]
        so.xb_internal_fragment_major.restype = C.c_size_t
        so.xb_internal_gate_interleave.argtypes = [vp, vp, vp, vp, ip, vp, vp, vp]
        so.xb_internal_gate_interleave.restype = None
        so.xb_internal_i8_limbs.argtypes = [vp, ip, ip, vp, vp, vp]
        so.xb_internal_i8_limbs.restype = None
        so.xb_internal_decode_status.argtypes = [C.c_uint, C.c_uint, C.POINTER(C.c_char_p)]
        so.xb_internal_ctc_columns.argtypes = [vp, ip, ip, ip, ip, ip, vp, vp, vp]
        so.xb_internal_ctc_columns.restype = None
        so.xb_internal_ctc_launch.argtypes = [ip, ip, ip, C.POINTER(ip), C.POINTER(C.c_size_t)]
        _cached = so
    return _cached


def knobs_from_env():
    """The library's knobs under the current environment, as a dict by field name."""
    k = Knobs()
    lib().xb_internal_knobs_from_env(C.byref(k))
    return {f: getattr(k, f) for f, _ in KNOBS}


class Planner:
    """xb_internal_plan_layer with its buffers kept between calls: plan(...) -> (LayerPlan, launches) where launches is a
    uint32 array (count, len(LAUNCH_FIELDS)), or (LayerPlan, None) when the planner refuses the query.  Both are views of
    the buffers: the next call overwrites them."""

    def __init__(self):
        self.fn = lib().xb_internal_plan_layer
        self.q, self.p = PlanQuery(), LayerPlan()
        self.recs = np.zeros((MAX_LAUNCHES, len(LAUNCH_FIELDS)), np.uint32)
        self.args = (C.byref(self.q), C.byref(self.p), self.recs.ctypes.data, MAX_LAUNCHES)

    def set_knobs(self, k):
        """k: schedule_plan.knobs(env)."""
        for f, name in KNOBS:
            if name in k:
                setattr(self.q.knobs, f, k[name])
        self.q.spread = k["XB_LSTM_SPREAD"]

    def plan(self, F, n, T, cu_count, dual_ok=True, signal_ok=True, has_next=True, resident1=True):
        q = self.q
        q.F, q.n, q.T, q.cu_count = F, n, T, cu_count
        q.has_next, q.resident1, q.resident2, q.signal_ok = has_next, resident1, dual_ok, signal_ok
        count = self.fn(*self.args)
        if count < 0:
            assert count == self.p.error
            return self.p, None
        assert 0 < count <= MAX_LAUNCHES and self.p.error == 0
        return self.p, self.recs[:count]


def decode_status(sync_word, data_word):
    """What a synchronising call reports for a context's two device status words (csrc/xb_status.h): (code, message), the
    message None with XB_OK."""
    msg = C.c_char_p()
    code = lib().xb_internal_decode_status(sync_word, data_word, C.byref(msg))
    return code, (msg.value.decode() if msg.value is not None else None)


def ctc_columns(labels, nb, sl, has_blank=True):
    """The lattice kernels' column rule (csrc/xb_ctc_lattice.h) over label rows (n, Lt): (stay, move, post), each (n, Lt - sl + 1)
    int32; cell l is position l's stay column, the move column into it and that column in the posteriors' layout."""
    labels = np.ascontiguousarray(labels, dtype=np.uint8)
    n, Lt = labels.shape
    out = [np.full((n, Lt - sl + 1), -1, np.int32) for _ in range(3)]
    lib().xb_internal_ctc_columns(labels.ctypes.data, n, Lt, nb, sl, int(has_blank), *[o.ctypes.data for o in out])
    return tuple(out)


def ctc_launch(positions, override=None, chains=False):
    """The lattice kernels' launch (csrc/xb_ctc_lattice.h) for rows of `positions` positions: (threads, PMAX, LDS bytes)."""
    threads, lds = C.c_int(), C.c_size_t()
    pmax = lib().xb_internal_ctc_launch(positions, 0 if override is None else override, int(chains), C.byref(threads), C.byref(lds))
    return threads.value, pmax, lds.value


def _f32(a):
    return np.ascontiguousarray(a, dtype=np.float32)


def f32_to_e4m3(x):
    return int(lib().xb_internal_f32_to_e4m3(float(x)))


def split_rows(w, ld, q8=False):
    """w (rows, cols) -> (hi (rows, ld) float16, second, exponent): second is the fp16 residual (rows, ld), or with q8 the
    image as bytes (rows, ld / 32, 64) and its exponent."""
    w = _f32(w)
    rows, cols = w.shape
    hi, lo = np.full((rows, ld), 7, np.float16), np.full((rows, ld), 7, np.float16)
    e = C.c_int(99)
    lib().xb_internal_split_rows(w.ctypes.data, rows, cols, ld, hi.ctypes.data, lo.ctypes.data, C.byref(e) if q8 else None)
    return (hi, lo.view(np.uint8).reshape(rows, ld // 32, 64), e.value) if q8 else (hi, lo, None)


def fragment_major(hi, lo, rows, K, nsplit):
    """split_rows outputs (leading dimension hi.shape[1]) -> (image bytes, k-tile stride)."""
    hi, lo = np.ascontiguousarray(hi), np.ascontiguousarray(lo)
    ks = C.c_size_t()
    fn = lib().xb_internal_fragment_major
    need = fn(hi.ctypes.data, lo.ctypes.data, rows, hi.shape[1], K, nsplit, None, 0, C.byref(ks))
    out = np.full(need, 0xa5, np.uint8)
    assert fn(hi.ctypes.data, lo.ctypes.data, rows, hi.shape[1], K, nsplit, out.ctypes.data, need, C.byref(ks)) == need
    return out, ks.value


def gate_interleave(wih, whh, bih, bhh):
    wih, whh, bih, bhh = _f32(wih), _f32(whh), _f32(bih), _f32(bhh)
    F = wih.shape[1]
    wi, wh, bb = np.empty_like(wih), np.empty_like(whh), np.empty_like(bih)
    lib().xb_internal_gate_interleave(wih.ctypes.data, whh.ctypes.data, bih.ctypes.data, bhh.ctypes.data, F, wi.ctypes.data,
                                      wh.ctypes.data, bb.ctypes.data)
    return wi, wh, bb


def i8_limbs(w):
    """w (rows, cols) -> (d1, d0 int8 (rows, cols), scale float32 (rows))."""
    w = _f32(w)
    d1, d0, sc = np.empty(w.shape, np.int8), np.empty(w.shape, np.int8), np.empty(w.shape[0], np.float32)
    lib().xb_internal_i8_limbs(w.ctypes.data, w.shape[0], w.shape[1], d1.ctypes.data, d0.ctypes.data, sc.ctypes.data)
    return d1, d0, sc
