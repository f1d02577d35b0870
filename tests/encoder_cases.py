"""The encoder precision table: shapes, weight sets and per-precision score bounds against the float64 reference
(tests/encoder_f64.py), and the defect catalogue each precision claims not to have.

tests/test_gpu_precision.py holds every HIP precision to its bound at every case; tests/test_encoder_f64.py checks, on the
CPU, that every defect of a precision's catalogue moves the reference's scores by at least DISCRIMINATION x that bound
(max or rms), so a kernel with such a defect cannot pass.  Pairs that cannot reach it are listed in EXCLUDED with the
reason and the measured ratio."""
from encoder_f64 import STAGES, rnn, stage_weight

DISCRIMINATION = 5.0
GROUP = 64                     # chunks per LSTM group (xb::lstm_group_chunks)

# name: (features, nb, L, N, weights).  L 5 = one time step, L % 5 != 0, one full-size chunk (L 10 000); N 65 / 130 leave
# a ragged last group, N 600 > 512 takes the wide group slots at features 768, N 1030 the two-groups-per-workgroup
# kernel at features 384; features 32 / 64 / 96 are one to three GEMM k-tiles; the int8 limbs run at 64 and F % 128 == 0.
CASES = {
    "f32_nb4_L23_N65": (32, 4, 23, 65, "sensitive"),
    "f64_nb5_L5_N3": (64, 5, 5, 3, "sensitive"),
    "f64_nb6_L2000_N130": (64, 6, 2000, 130, "outlier"),
    "f96_nb6_L1003_N130": (96, 6, 1003, 130, "sensitive"),
    "f128_nb4_L1202_N65": (128, 4, 1202, 65, "outlier"),
    "f256_nb5_L600_N130": (256, 5, 600, 130, "sensitive"),
    "f384_nb6_L300_N1030": (384, 6, 300, 1030, "sensitive"),
    "f512_nb4_L801_N130": (512, 4, 801, 130, "outlier"),
    "f768_nb6_L10000_N600": (768, 6, 10000, 600, "sensitive"),
    "f768_nb5_L1000_N130": (768, 5, 1000, 130, "outlier"),
}

# precision name: (xb_precision name, XB_LSTM_I8)
PRECISIONS = {"f16x3": ("f16x3", "0"), "f16": ("f16", "0"), "f16f8": ("f16f8", "0"), "f16f8i": ("f16f8i", "0"),
              "mixed": ("mixed", "0"), "i8": ("f16f8", "1"), "i8x3": ("f16f8", "2")}


def seed_of(name):
    F, nb, L, N, _ = CASES[name]
    return F + nb


def picks(N):
    """The chunks compared with the reference: first, last and both sides of every group seam that the batch has, the
    last group's first chunk included."""
    p = {0, N - 1}
    for s in range(GROUP, N, GROUP):
        if s in (GROUP, (N - 1) // GROUP * GROUP):
            p |= {s - 1, s}
    return sorted(p)


def i8_active(features):
    return features == 64 or features % 128 == 0


def catalogue(prec, features, winlen=19):
    """The defects a precision claims not to have (names: tests/encoder_f64.py).  A window of 1 has no padding: pad:2 means
    nothing there and win:late does not exist."""
    cat = ["bhh:ignore", "bhh:order", "pad:0"] + (["pad:2", "win:late"] if winlen >= 3 else []) + ["conv16:0", "conv16:1"]
    cat += ["shift:%d" % l for l in range(5)] + ["flip:%d" % l for l in range(5)]
    # the main product is fp16 in every precision: no weight may be used as its e4m3 image alone
    cat += ["w8:" + stage_weight(s) for s in STAGES]
    if prec == "f16":
        return cat
    stages = [s for s in STAGES if not (prec == "f16f8i" and s.startswith("in"))]
    for s in stages:
        if prec in ("i8", "i8x3") and s.startswith("rec") and i8_active(features):
            cat.append("wi8:" + rnn(int(s[-1]), "weight_hh_l0"))           # the int8 limbs' low digit
        else:
            cat += ["w16:" + stage_weight(s), "a16:" + s]                   # the weight- and activation-side correction
    return cat


# Score bounds against the float64 reference: BOUNDS[case][precision] = (max, rms) over the picked chunks, set at 2-3 x the
# largest error measured on the MI355X over both LSTM launch modes (the two modes agree bit for bit).
BOUNDS = {
    "f32_nb4_L23_N65": {"f16x3": (2.1e-05, 1.7e-06), "f16": (2.3e-02, 1.3e-03), "f16f8": (5.3e-04, 3.9e-05), "f16f8i": (1.4e-02, 9.7e-04), "mixed": (1.2e-04, 8.5e-06), "i8": (5.3e-04, 3.9e-05), "i8x3": (5.3e-04, 3.9e-05)},
    "f64_nb5_L5_N3": {"f16x3": (3.0e-06, 1.1e-06), "f16": (6.9e-04, 4.1e-05), "f16f8": (1.6e-05, 1.8e-06), "f16f8i": (2.1e-04, 2.1e-05), "mixed": (3.0e-06, 1.1e-06), "i8": (1.6e-05, 1.8e-06), "i8x3": (1.6e-05, 1.8e-06)},
    "f64_nb6_L2000_N130": {"f16x3": (1.2e-04, 5.5e-06), "f16": (1.4e-01, 8.0e-03), "f16f8": (5.0e-03, 2.3e-04), "f16f8i": (1.1e-01, 7.8e-03), "mixed": (1.9e-03, 1.1e-04), "i8": (9.2e-03, 5.2e-04), "i8x3": (1.6e-02, 6.6e-04)},
    "f96_nb6_L1003_N130": {"f16x3": (8.0e-05, 5.7e-06), "f16": (1.2e-01, 8.8e-03), "f16f8": (3.6e-03, 2.6e-04), "f16f8i": (1.0e-01, 7.8e-03), "mixed": (1.4e-03, 1.1e-04), "i8": (3.6e-03, 2.6e-04), "i8x3": (3.6e-03, 2.6e-04)},
    "f128_nb4_L1202_N65": {"f16x3": (3.1e-04, 1.1e-05), "f16": (2.3e-01, 8.5e-03), "f16f8": (8.5e-03, 3.0e-04), "f16f8i": (2.5e-01, 7.5e-03), "mixed": (2.2e-03, 8.7e-05), "i8": (1.3e-02, 5.0e-04), "i8x3": (1.5e-02, 7.2e-04)},
    "f256_nb5_L600_N130": {"f16x3": (8.1e-05, 6.1e-06), "f16": (9.9e-02, 7.5e-03), "f16f8": (2.9e-03, 2.0e-04), "f16f8i": (9.3e-02, 7.0e-03), "mixed": (9.5e-04, 6.3e-05), "i8": (5.0e-03, 3.8e-04), "i8x3": (5.9e-03, 4.7e-04)},
    "f384_nb6_L300_N1030": {"f16x3": (1.6e-04, 1.1e-05), "f16": (1.5e-01, 1.1e-02), "f16f8": (3.5e-03, 2.9e-04), "f16f8i": (1.1e-01, 7.7e-03), "mixed": (1.3e-03, 8.7e-05), "i8": (7.4e-03, 5.8e-04), "i8x3": (8.5e-03, 6.7e-04)},
    "f512_nb4_L801_N130": {"f16x3": (1.1e-04, 1.1e-05), "f16": (9.7e-02, 7.7e-03), "f16f8": (2.3e-03, 2.1e-04), "f16f8i": (6.5e-02, 5.9e-03), "mixed": (7.7e-04, 7.1e-05), "i8": (1.1e-02, 8.8e-04), "i8x3": (1.9e-02, 1.3e-03)},
    "f768_nb6_L10000_N600": {"f16x3": (1.8e-04, 1.2e-05), "f16": (1.2e-01, 8.3e-03), "f16f8": (2.9e-03, 2.2e-04), "f16f8i": (7.8e-02, 6.6e-03), "mixed": (1.3e-03, 8.2e-05), "i8": (6.9e-03, 5.2e-04), "i8x3": (9.0e-03, 6.2e-04)},
    "f768_nb5_L1000_N130": {"f16x3": (1.8e-04, 1.5e-05), "f16": (1.1e-01, 9.7e-03), "f16f8": (2.9e-03, 2.6e-04), "f16f8i": (9.3e-02, 7.6e-03), "mixed": (1.4e-03, 9.4e-05), "i8": (1.8e-02, 1.4e-03), "i8x3": (2.3e-02, 1.8e-03)},
}

# LSTM layer 3 / 4 outputs (debug_layer_output) against the reference's, max |error|: hi + fp16 residual where the consumer
# reads a residual, hi alone (fp16 rounding of h included) where it reads a q8 image or nothing.
LAYER_BOUNDS = {"f16x3": 7.7e-06, "f16": 8.6e-03, "f16f8": 7.1e-04, "f16f8i": 6.0e-03, "mixed": 6.7e-05, "i8": 9.1e-04, "i8x3": 1.3e-03}

# (case, precision, defect): (reason key, measured ratio) -- pairs left out of the discrimination check
from encoder_excluded import EXCLUDED, REASONS  # noqa: E402,F401
