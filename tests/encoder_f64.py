"""A float64 restatement of the inference encoder (torch on the CPU) with defect hooks, and weight sets whose scores are
sensitive to rounding.  Test infrastructure for tests/test_encoder_f64.py and tests/test_gpu_precision.py.

The model (the encoder of crf/model.py as oracle/xna_oracle.c documents it):
  conv(1 -> 4, k 5, pad 2), conv(4 -> 16, k 5, pad 2), conv(16 -> F, k winlen, stride, pad winlen // 2), each + SiLU;
  permute to (T, N, F); five LSTMs run reverse, forward, reverse, forward, reverse, gates i, f, g, o, zero initial state,
  gates = W_ih x + b_ih + W_hh h + b_hh; linear layer, then scale * tanh; blank column (the constant blank_score at
  index 0 of every nb + 1 group) expanded or not, the layouts xb_encode returns.

A defect models one way a kernel can be subtly wrong: the lost correction product of a split-fp16 or FP8 contraction is a
weight or an activation rounded to fp16, the lost low digit of the int8-limb recurrence a weight rounded to 8-bit per-row
fixed point, and so on.  Defect names (`run(defects=...)`):
  "w16:<key>" / "w8:<key>" / "wi8:<key>"  weight tensor <key> rounded to fp16 / to e4m3 with the tensor-wide exponent of
                                          the library's split_rows / to 8-bit per-row fixed point (int8 limbs, low digit dropped)
  "a16:<stage>"    the input activations of a GEMM stage rounded to fp16: conv3 (its im2col input), in<l> (input projection
                   of layer l), rec<l> (the h that recurrence l feeds back), linear
  "conv16:<c>"     conv c (0 or 1) in fp16: its input, weights, bias and output rounded to fp16
  "shift:<l>"      layer l reads its input one time step late (x[t - 1], zeros at t = 0)
  "flip:<l>"       layer l runs in the other direction
  "pad:<c>"        conv c (0 or 2) pads with the neighbouring chunks' samples instead of zeros (nothing at padding 0)
  "win:late"       conv 2 pads pad - 1 samples on the left and pad + 1 on the right: every window starts one sample late
                   (an off-by-one in the tile origin; needs winlen >= 3)
  "bhh:ignore"     bias_hh left out of every layer's gate bias
  "bhh:order"      bias_hh added with the gate order i, f, o, g instead of i, f, g, o
"""
import functools

import numpy as np
import torch

from xna_basecaller_amd.synthetic import peaky_weights

STAGES = ["conv3"] + ["in%d" % l for l in range(5)] + ["rec%d" % l for l in range(5)] + ["linear"]


def rnn(l, p):
    return "encoder.%d.rnn.%s" % (4 + l, p)


def stage_weight(stage):
    """The weight tensor a GEMM stage multiplies its activations with."""
    if stage == "conv3":
        return "encoder.2.conv.weight"
    if stage == "linear":
        return "encoder.9.linear.weight"
    return rnn(int(stage[-1]), "weight_ih_l0" if stage.startswith("in") else "weight_hh_l0")


# ---- roundings -------------------------------------------------------------------------------------------------
def to_f16(a):
    return np.asarray(a, np.float64).astype(np.float16).astype(np.float64)


def to_e4m3(a):
    """OCP e4m3 (fn): 3 mantissa bits, round to nearest even, subnormal steps of 2^-9, saturating at 448."""
    a = np.asarray(a, np.float64)
    m = np.abs(a)
    e = np.floor(np.log2(np.where(m > 0, m, 1.0)))
    step = np.where(m < 2.0 ** -6, 2.0 ** -9, 2.0 ** (e - 3))
    q = np.minimum(np.round(m / step) * step, 448.0)
    return np.copysign(q, a)


def split_rows_exp(w):
    """The tensor-wide e4m3 exponent of split_rows (csrc/xb_pack.h): the largest |value| lands near 224."""
    amax = float(np.abs(np.asarray(w, np.float32)).max())
    e = int(np.floor(np.log2(np.float32(448.0) / np.float32(amax)))) - 1 if amax > 0 and np.isfinite(amax) else 0
    return min(max(e, -16), 32)


def to_e4m3_tensor(w):
    e = split_rows_exp(w)
    return to_e4m3(np.asarray(w, np.float64) * 2.0 ** e) * 2.0 ** -e


def to_i8_rows(w):
    """Per-row 16-bit fixed point q = rint(w / max|row| * 32512) = 256 d1 + d0, balanced digits; only d1 kept."""
    w = np.asarray(w, np.float64)
    rows = w.reshape(w.shape[0], -1)
    s = np.abs(rows).max(axis=1, keepdims=True)
    s = np.where(s > 0, s, 1.0)
    q = np.rint(rows / s * 32512.0).astype(np.int64)
    d0 = ((q + 128) & 255) - 128
    return ((q - d0) * s / 32512.0).reshape(w.shape)


WEIGHT_ROUNDING = {"w16": to_f16, "w8": to_e4m3_tensor, "wi8": to_i8_rows}


# ---- the encoder ---------------------------------------------------------------------------------------------
def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64))


def _r16(x):
    return x.to(torch.float16).to(torch.float64)


def _conv(x, w, b, stride, pad, neighbour, late=False):
    """x (N, C, L); zero padding, or with `neighbour` the last / first `pad` samples of the previous / next chunk; with
    `late` the zero padding is pad - 1 on the left and pad + 1 on the right."""
    if late:
        x = torch.nn.functional.pad(x, (pad - 1, pad + 1))
    elif neighbour and pad == 0:
        pass                                              # [..., -0:] would take the whole neighbour
    elif neighbour:
        short = max(pad - x.shape[2], 0)                  # chunks shorter than the padding: zeros beyond the neighbour
        left = torch.nn.functional.pad(torch.roll(x, 1, dims=0), (short, 0))[..., -pad:]
        right = torch.nn.functional.pad(torch.roll(x, -1, dims=0), (0, short))[..., :pad]
        x = torch.cat([left, x, right], dim=2)
    else:
        x = torch.nn.functional.pad(x, (pad, pad))
    return torch.nn.functional.silu(torch.nn.functional.conv1d(x, w, b, stride=stride))


def _lstm(x, w_ih, w_hh, bias, reverse, round_in, round_h):
    """x (T, N, F) -> (T, N, H); gates i, f, g, o."""
    T, N, _ = x.shape
    H = w_hh.shape[1]
    gin = torch.matmul(_r16(x) if round_in else x, w_ih.t()) + bias
    h = torch.zeros((N, H), dtype=torch.float64)
    c = torch.zeros((N, H), dtype=torch.float64)
    wt = w_hh.t().contiguous()
    y = torch.empty((T, N, H), dtype=torch.float64)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        g = gin[t] + torch.matmul(_r16(h) if round_h else h, wt)
        i, f, gg, o = torch.sigmoid(g[:, :H]), torch.sigmoid(g[:, H:2 * H]), torch.tanh(g[:, 2 * H:3 * H]), torch.sigmoid(g[:, 3 * H:])
        c = f * c + i * gg
        h = o * torch.tanh(c)
        y[t] = h
    return y


def blank_layout(scores, nb, blank_score, expand_blanks):
    """(T, N, S * nb) -> the layout xb_encode returns: with expand_blanks (T, N, S * (nb + 1)), blank_score at index 0."""
    if not expand_blanks:
        return scores
    T, N, C = scores.shape
    S = C // nb
    out = np.empty((T, N, S, nb + 1), scores.dtype)
    out[..., 0] = blank_score
    out[..., 1:] = scores.reshape(T, N, S, nb)
    return out.reshape(T, N, S * (nb + 1))


class Reference:
    """The float64 encoder of one signal batch and one weight set.  The clean stages are computed once; a run with
    defects recomputes from the first stage a defect touches.  Stages: 'conv' (T, N, F) conv3 output, 'lstm<l>' (T, N, F),
    'scores' (T, N, S * nb) without the blank column."""

    def __init__(self, signal, state_dict, n_base, winlen=19, stride=5, scale=5.0, blank_score=2.0):
        self.x = np.asarray(signal, np.float64).reshape(np.shape(signal)[0], -1)
        self.w = {k: np.asarray(v, np.float64) for k, v in state_dict.items()}
        self.nb, self.winlen, self.stride, self.scale, self.blank = n_base, winlen, stride, scale, blank_score
        self._clean = None

    def clean(self):
        if self._clean is None:
            self._clean = self._run(frozenset())
        return self._clean

    def scores(self, expand_blanks=True, defects=()):
        s = self.run(defects)["scores"]
        return blank_layout(s, self.nb, self.blank, expand_blanks)

    def run(self, defects=()):
        defects = frozenset(defects)
        out = self.clean() if not defects else self._run(defects)
        return {k: v.numpy() for k, v in out.items()}

    @staticmethod
    def _first_stage(defects):
        """0 = conv front end, 1 + l = LSTM layer l, 6 = the linear layer."""
        first = 6
        for d in defects:
            kind, arg = d.split(":", 1)
            if kind in ("conv16", "pad", "win"):
                first = 0
            elif kind in ("shift", "flip"):
                first = min(first, 1 + int(arg))
            elif kind == "bhh":
                first = min(first, 1)
            elif kind == "a16":
                first = min(first, 0 if arg == "conv3" else (6 if arg == "linear" else 1 + int(arg[-1])))
            else:
                first = min(first, 0 if ".conv." in arg else (6 if "linear" in arg else int(arg.split(".")[1]) - 3))
        return first

    def _weights(self, defects):
        w = dict(self.w)
        for d in defects:
            kind, arg = d.split(":", 1)
            if kind in WEIGHT_ROUNDING:
                if arg not in w:
                    raise KeyError(d)
                w[arg] = WEIGHT_ROUNDING[kind](w[arg])
        return {k: _t(v) for k, v in w.items()}

    def _run(self, defects):
        threads = torch.get_num_threads()
        torch.set_num_threads(min(threads, 4))        # the recurrence is a chain of small products: more threads only wait
        try:
            return self._stages(defects)
        finally:
            torch.set_num_threads(threads)

    def _stages(self, defects):
        for d in defects:
            kind, arg = d.split(":", 1)
            ok = {"w16": lambda a: a in self.w, "w8": lambda a: a in self.w, "wi8": lambda a: a in self.w,
                  "a16": lambda a: a in STAGES, "conv16": lambda a: a in ("0", "1"), "pad": lambda a: a in ("0", "2"),
                  "shift": lambda a: a in "01234", "flip": lambda a: a in "01234", "bhh": lambda a: a in ("ignore", "order"),
                  "win": lambda a: a == "late" and self.winlen >= 3}
            if kind not in ok or not ok[kind](arg):
                raise ValueError("unknown defect %r" % d)
        first = self._first_stage(defects) if defects else 0
        base = self._clean if (defects and self._clean is not None) else None
        if base is None:
            first = 0
        w = self._weights(defects)
        a16 = {d.split(":", 1)[1] for d in defects if d.startswith("a16:")}
        out = {}
        with torch.no_grad():
            if first == 0:
                h = _t(self.x)[:, None, :]
                for c, (k, pad, stride) in enumerate([(5, 2, 1), (5, 2, 1), (self.winlen, self.winlen // 2, self.stride)]):
                    wc, bc = w["encoder.%d.conv.weight" % c], w["encoder.%d.conv.bias" % c]
                    half = "conv16:%d" % c in defects
                    if half:
                        h, wc, bc = _r16(h), _r16(wc), _r16(bc)
                    if c == 2 and "conv3" in a16:
                        h = _r16(h)
                    h = _conv(h, wc, bc, stride, pad, "pad:%d" % c in defects, c == 2 and "win:late" in defects)
                    if half:
                        h = _r16(h)
                out["conv"] = h.permute(2, 0, 1).contiguous()
            else:
                out["conv"] = base["conv"]
            x = out["conv"]
            for l in range(5):
                key = "lstm%d" % l
                if first > 1 + l:
                    out[key] = base[key]
                else:
                    bhh = w[rnn(l, "bias_hh_l0")]
                    if "bhh:ignore" in defects:
                        bhh = torch.zeros_like(bhh)
                    elif "bhh:order" in defects:
                        bhh = bhh.reshape(4, -1)[[0, 1, 3, 2]].reshape(-1)
                    xin = x
                    if "shift:%d" % l in defects:
                        xin = torch.cat([torch.zeros_like(x[:1]), x[:-1]], dim=0)
                    reverse = (l % 2 == 0) != ("flip:%d" % l in defects)
                    out[key] = _lstm(xin, w[rnn(l, "weight_ih_l0")], w[rnn(l, "weight_hh_l0")], w[rnn(l, "bias_ih_l0")] + bhh,
                                     reverse, "in%d" % l in a16, "rec%d" % l in a16)
                x = out[key]
            if first > 6:
                out["scores"] = base["scores"]
            else:
                xl = _r16(x) if "linear" in a16 else x
                z = torch.matmul(xl, w["encoder.9.linear.weight"].t()) + w["encoder.9.linear.bias"]
                out["scores"] = self.scale * torch.tanh(z)
        return out


def encode(signal, state_dict, n_base, expand_blanks=True, defects=(), **kw):
    """signal (N, L) -> float64 scores (T, N, C) in the layout xb_encode returns."""
    return Reference(signal, state_dict, n_base, **kw).scores(expand_blanks, defects)


# ---- weight sets ---------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _sensitive(features, nb, seed, outlier, state_len=3, winlen=19):
    sd = peaky_weights(features, nb, seed, blank_bias=3.0, state_len=state_len, winlen=winlen)
    rng = np.random.default_rng(1000 + seed)
    F = features
    for l in range(5):
        # gate biases as a trained LSTM has them: small, different in b_ih and b_hh gate by gate, a forget-gate offset
        sd[rnn(l, "bias_ih_l0")] = (0.1 * rng.standard_normal(4 * F)).astype(np.float32)
        sd[rnn(l, "bias_hh_l0")] = (0.1 * rng.standard_normal(4 * F) + np.repeat([0.0, 0.2, 0.0, 0.0], F)).astype(np.float32)
    if outlier:
        for k in sorted(sd):
            a = sd[k].astype(np.float64).reshape(-1)
            norm = np.sqrt((a ** 2).sum())
            hit = rng.random(a.size) < 0.003
            hit[rng.integers(a.size)] = True             # at least one per tensor
            a[hit] *= 8.0
            if norm > 0:
                a *= norm / np.sqrt((a ** 2).sum())      # the same gain as the bulk-only tensor
            sd[k] = a.reshape(sd[k].shape).astype(np.float32)
    return sd


def sensitive_weights(features, nb, seed=25, state_len=3, winlen=19):
    """peaky_weights (signal-dependent, peaky scores: synthetic.peaky_weights) with the CRF blank bias at 3 and non-zero
    LSTM gate biases: b_ih and b_hh ~ N(0, 0.1) differ gate by gate, and b_hh carries a forget-gate offset of +0.2.  A lost
    bias_hh, a bias folded in the wrong gate order or a lost correction product moves the scores visibly; at features 768
    0.55-0.7 bases are called per time step (tests/test_encoder_f64.py checks the regime)."""
    return {k: v.copy() for k, v in _sensitive(features, nb, seed, False, state_len, winlen).items()}


def outlier_weights(features, nb, seed=25, state_len=3, winlen=19):
    """sensitive_weights with 3 per mille of the entries of every tensor (at least one) scaled x 8 against the bulk (the
    tensor then rescaled to its former norm): the largest |w| of a tensor, which sets the tensor-wide e4m3 exponent of
    split_rows and the per-row int8 scale, sits far above the bulk, so the bulk keeps fewer significant bits there."""
    return {k: v.copy() for k, v in _sensitive(features, nb, seed, True, state_len, winlen).items()}


WEIGHTS = {"sensitive": sensitive_weights, "outlier": outlier_weights}
