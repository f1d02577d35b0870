"""The table behind the refusal tests (tests/test_refusals_host.py, tests/test_gpu_refusals.py): what the entry points that take
signal chunks or a (T, n, C) score tensor refuse, with the exact status and the exact text of xb_last_error, on ONE small context.

  SIGNATURES   entry point -> its parameters after the context, in the C ABI's order.  A `_dev` form has its host form's.
  ROWS         Row(fn, fault, args, code, message, ctx).  args overrides the good call's arguments (good()); message is the text,
               or for a double fault the two texts of which one is named -- which, the header does not promise.  ctx: "bare" (no
               weights), "loaded", or "both".
  EXCLUDED     exported names that match FAMILIES and have no rows, with the reason.

The context: 6 bases, state length 3 (216 states), features 32, window 19, stride 5, chunks of 200 samples (T = 40), at most 4
chunks.  Every row returns before any kernel is launched, except xb_basecall_chunks_beam's beam (width and cut) and alphabet
rows: that call checks what its beam search needs after its encoder pass (of valid chunks) has been launched.

The symbolic argument values: None is a null pointer; SHORT_LENGTH and HIGH_LABEL are the label batch with its first length
below the state length, or its first label above n_base; every pointer not named is a buffer large enough for the call."""
import collections

NB, SL, F, WIN, STRIDE, SCALE, BLANK, CHUNK, T, MAX_BATCH, LT = 6, 3, 32, 19, 5, 5.0, 2.0, 200, 40, 4, 8
ALPHABET = b"NACGTXY"
INVALID, STATE = -1, -4
SLOTS = 4
SHORT_LENGTH, HIGH_LABEL = "first length below the state length", "first label above n_base"

_DECODE = ("scores", "T", "n", "has_blank", "alphabet")
_CALIB = ("qscale", "qoffset")
_BEAM = ("beam_width", "beam_cut", "qscale", "qoffset", "sequence", "qstring", "moves", "score")
_LABELS = ("targets", "Lt", "lengths")
SIGNATURES = {
    "xb_encode": ("signal", "n", "expand_blanks", "out_scores"),
    "xb_decode": _DECODE + ("labels", "seq", "seq_len"),
    "xb_decode_q": _DECODE + _CALIB + ("seq", "qstring", "moves", "seq_len"),
    "xb_decode_ub": _DECODE + _CALIB + ("seq", "qstring", "moves", "probs", "seq_len"),
    "xb_crf_scans": ("scores", "T", "n", "has_blank", "alpha", "beta", "logz", "post"),
    "xb_crf_logz": ("scores", "T", "n", "has_blank", "logz"),
    "xb_ctc_logz": ("scores", "T", "n") + _LABELS + ("logz", "gstay", "gmove"),
    "xb_ctc_alignments": ("scores", "T", "n") + _LABELS + ("alignments", "max_score"),
    "xb_beam_search": _DECODE + _BEAM,
    "xb_basecall_chunks_beam": ("signal", "n", "alphabet") + _BEAM,
    "xb_basecall_chunks": ("signal", "n", "alphabet", "seq", "seq_len"),
    "xb_basecall_chunks_q": ("signal", "n", "alphabet") + _CALIB + ("seq", "qstring", "moves", "seq_len"),
    "xb_basecall_chunks_ub": ("signal", "n", "alphabet") + _CALIB + ("seq", "qstring", "moves", "probs", "seq_len"),
    "xb_submit_chunks": ("slot", "signal", "n", "alphabet"),
    "xb_submit_chunks_q": ("slot", "signal", "n", "alphabet") + _CALIB,
    "xb_submit_chunks_ub": ("slot", "signal", "n", "alphabet") + _CALIB,
    "xb_collect_chunks": ("slot", "seq", "seq_len"),
    "xb_collect_chunks_q": ("slot", "seq", "seq_len", "qstring", "moves"),
    "xb_collect_chunks_ub": ("slot", "seq", "seq_len", "qstring", "moves", "probs"),
    "xb_ctc_loss": ("scores", "T", "n", "has_blank") + _LABELS + ("loss", "logz"),
    "xb_ctc_loss_grad": ("scores", "T", "n", "has_blank") + _LABELS + ("loss_clip", "mean", "loss", "grad"),
    "xb_validate_chunks": ("signal", "n", "alphabet") + _LABELS + ("seq", "seq_len", "loss"),
}
for _fn in ("xb_encode", "xb_decode", "xb_decode_q", "xb_decode_ub", "xb_crf_scans", "xb_crf_logz", "xb_beam_search",
            "xb_basecall_chunks", "xb_ctc_loss", "xb_ctc_loss_grad"):
    SIGNATURES[_fn + "_dev"] = SIGNATURES[_fn]

# the arguments that are no pointers, with the good call's value
SCALARS = {"T": T, "n": 2, "has_blank": 1, "expand_blanks": 1, "alphabet": ALPHABET, "qscale": 1.0, "qoffset": 0.0, "Lt": LT,
           "beam_width": 4, "beam_cut": 100.0, "slot": 0, "loss_clip": 0.0, "mean": 1}
FLOATS = ("qscale", "qoffset", "beam_cut", "loss_clip")
INT32_LABELS = ("xb_ctc_logz", "xb_ctc_alignments")        # their targets are int32 rows; the losses' are uint8

# the exported names these prefixes match are the families of this table (test_refusals_host.py)
FAMILIES = ("xb_encode", "xb_decode", "xb_crf_", "xb_ctc_logz", "xb_ctc_alignments", "xb_ctc_loss", "xb_beam_search",
            "xb_basecall_chunks", "xb_submit_chunks", "xb_collect_chunks", "xb_validate_chunks")
EXCLUDED = {"xb_encode_bottom_dev": "a training call on layer outputs (tests/test_gpu_toptrainer.py), not on chunks to scores"}

Row = collections.namedtuple("Row", "fn fault args code message ctx")
ROWS = []

NO_WEIGHTS = "weights not loaded: call xb_load_weights for all 28 tensors, then xb_weights_ready"
ALPHABET_SHORT = "alphabet needs %d symbols" % (NB + 1)
ALPHABET_MISSING = "alphabet is required when seq is requested"
NO_OUTPUT = "no output requested"
BAD_SLOT = "bad slot / null argument"
BEAM_CUT = "beam_cut 0.5 inside (0, 1): no candidate can reach it"


def batch(n, who=""):
    return "%sbatch %d outside [1, max_batch=%d]" % (who, n, MAX_BATCH)


def steps(t, who=""):
    return "%sT=%d outside [1, %d]" % (who, t, T)


def width(lt, who=""):
    return "%starget width %d gives %d positions, supported: 1..2048" % (who, lt, lt - (SL - 1))


def short_length(who=""):
    return "%starget_lengths[0] = %d outside [state_len = %d, %d]" % (who, SL - 1, SL, LT)


def high_label(who=""):
    return "%stargets[0][0] = %d outside [0, n_base = %d]" % (who, NB + 1, NB)


def row(fn, fault, args, code, message, ctx="both"):
    assert set(args) <= set(SIGNATURES[fn]), (fn, fault)
    ROWS.append(Row(fn, fault, args, code, message, ctx))


def ranges(fn, who="", ctx="both", with_T=True):
    for n in (0, MAX_BATCH + 1):
        row(fn, "n=%d" % n, {"n": n}, INVALID, batch(n, who), ctx)
    for t in (0, T + 1) if with_T else ():
        row(fn, "T=%d" % t, {"T": t}, INVALID, steps(t, who), ctx)


def nulls(fn, names, message, ctx="both"):
    for name in names:
        row(fn, "null " + name, {name: None}, INVALID, message, ctx)


def null_word(fn):
    return "null device pointer" if fn.endswith("_dev") else "null host pointer"


def needs_weights(fn):
    row(fn, "no weights", {}, STATE, NO_WEIGHTS, "bare")


# ---- single faults: one thing wrong in the call ----------------------------------------------------------------------------------
for fn in ("xb_encode", "xb_encode_dev"):
    needs_weights(fn)
    ranges(fn, ctx="loaded", with_T=False)
    nulls(fn, ("signal", "out_scores"), null_word(fn), "loaded")

for fn in ("xb_decode", "xb_decode_dev"):
    ranges(fn)
    nulls(fn, ("scores",), null_word(fn))
    row(fn, "alphabet short", {"alphabet": ALPHABET[:-1]}, INVALID, ALPHABET_SHORT)
    row(fn, "alphabet missing", {"alphabet": None}, INVALID, ALPHABET_MISSING)
for level, fn in ((1, "xb_decode_q"), (2, "xb_decode_ub")):
    for fn in (fn, fn + "_dev"):
        ranges(fn)
        nulls(fn, ("scores", "seq", "qstring", "alphabet") + (("probs",) if level == 2 else ()), "null argument")
        row(fn, "alphabet short", {"alphabet": ALPHABET[:-1]}, INVALID, ALPHABET_SHORT)

for fn in ("xb_crf_scans", "xb_crf_scans_dev"):
    ranges(fn)
    nulls(fn, ("scores",), null_word(fn))
    row(fn, "no output", {"alpha": None, "beta": None, "logz": None, "post": None}, INVALID, NO_OUTPUT)
for fn in ("xb_crf_logz", "xb_crf_logz_dev"):
    ranges(fn)
    nulls(fn, ("scores",), null_word(fn))
    row(fn, "no output", {"logz": None}, INVALID, NO_OUTPUT)

for fn in ("xb_ctc_logz", "xb_ctc_alignments"):
    ranges(fn)
    nulls(fn, ("scores", "targets", "lengths") + (("alignments",) if fn == "xb_ctc_alignments" else ()), "null host pointer")
    row(fn, "no positions", {"Lt": SL - 1}, INVALID, width(SL - 1))
    row(fn, "short length", {"lengths": SHORT_LENGTH}, INVALID, short_length())
    row(fn, "high label", {"targets": HIGH_LABEL}, INVALID, high_label())
row("xb_ctc_logz", "no output", {"logz": None, "gstay": None, "gmove": None}, INVALID, NO_OUTPUT)

for fn in ("xb_beam_search", "xb_beam_search_dev"):
    ranges(fn)
    nulls(fn, ("scores", "sequence", "qstring", "moves"), null_word(fn))
    for w in (0, 33):
        row(fn, "beam width %d" % w, {"beam_width": w}, INVALID, "beam_width %d outside [1, 32]" % w)
    row(fn, "beam cut inside (0, 1)", {"beam_cut": 0.5}, INVALID, BEAM_CUT)
    row(fn, "alphabet short", {"alphabet": ALPHABET[:-1]}, INVALID, ALPHABET_SHORT)
    row(fn, "alphabet missing", {"alphabet": None}, INVALID, ALPHABET_SHORT)

fn = "xb_basecall_chunks_beam"
needs_weights(fn)
ranges(fn, ctx="loaded", with_T=False)
nulls(fn, ("signal", "sequence", "qstring", "moves", "alphabet"), "null argument", "loaded")
for w in (0, 33):
    row(fn, "beam width %d" % w, {"beam_width": w}, INVALID, "beam_width %d outside [1, 32]" % w, "loaded")
row(fn, "beam cut inside (0, 1)", {"beam_cut": 0.5}, INVALID, BEAM_CUT, "loaded")
row(fn, "alphabet short", {"alphabet": ALPHABET[:-1]}, INVALID, ALPHABET_SHORT, "loaded")

for fn, planes in (("xb_basecall_chunks", ()), ("xb_basecall_chunks_dev", ()), ("xb_basecall_chunks_q", ("qstring",)),
                   ("xb_basecall_chunks_ub", ("qstring", "probs"))):
    needs_weights(fn)
    ranges(fn, ctx="loaded", with_T=False)
    nulls(fn, ("signal", "seq", "alphabet") + planes, "null argument", "loaded")
    row(fn, "alphabet short", {"alphabet": ALPHABET[:-1]}, INVALID, ALPHABET_SHORT, "loaded")

for fn in ("xb_submit_chunks", "xb_submit_chunks_q", "xb_submit_chunks_ub"):
    needs_weights(fn)
    ranges(fn, ctx="loaded", with_T=False)
    for slot in (-1, SLOTS):
        row(fn, "slot %d" % slot, {"slot": slot}, INVALID, BAD_SLOT, "loaded")
    nulls(fn, ("signal", "alphabet"), BAD_SLOT, "loaded")
    row(fn, "alphabet short", {"alphabet": ALPHABET[:-1]}, INVALID, ALPHABET_SHORT, "loaded")
for fn, planes, idle in (("xb_collect_chunks", (), "slot 0 has nothing in flight"),
                         ("xb_collect_chunks_q", ("qstring",), "slot 0 has no submission with qualities in flight"),
                         ("xb_collect_chunks_ub", ("qstring", "probs"), "slot 0 has no submission with letter probabilities in flight")):
    for slot in (-1, SLOTS):
        row(fn, "slot %d" % slot, {"slot": slot}, INVALID, BAD_SLOT)
    nulls(fn, ("seq",) + planes, BAD_SLOT)
    row(fn, "nothing in flight", {}, STATE, idle)

for fn in ("xb_ctc_loss", "xb_ctc_loss_dev", "xb_ctc_loss_grad", "xb_ctc_loss_grad_dev"):
    who = fn[:-4] + ": " if fn.endswith("_dev") else fn + ": "
    ranges(fn, who)
    nulls(fn, ("scores", "targets", "lengths", "loss") + (("grad",) if "grad" in fn else ()), who + null_word(fn))
    row(fn, "no positions", {"Lt": SL - 1}, INVALID, width(SL - 1, who))
    if not fn.endswith("_dev"):            # the _dev forms' rows are validated by the kernel, on the device
        row(fn, "short length", {"lengths": SHORT_LENGTH}, INVALID, short_length(who))
        row(fn, "high label", {"targets": HIGH_LABEL}, INVALID, high_label(who))

fn, who = "xb_validate_chunks", "xb_validate_chunks: "
needs_weights(fn)
ranges(fn, ctx="loaded", with_T=False)             # (refused by the check for weights and room: no prefix)
nulls(fn, ("signal", "alphabet", "targets", "lengths", "seq", "seq_len", "loss"), who + "null argument", "loaded")
row(fn, "alphabet short", {"alphabet": ALPHABET[:-1]}, INVALID, ALPHABET_SHORT, "loaded")
row(fn, "no positions", {"Lt": SL - 1}, INVALID, width(SL - 1, who), "loaded")
row(fn, "short length", {"lengths": SHORT_LENGTH}, INVALID, short_length(who), "loaded")
row(fn, "high label", {"targets": HIGH_LABEL}, INVALID, high_label(who), "loaded")

SINGLE = len(ROWS)

# ---- double faults: two things wrong; the status is exact, the text is one of the two single faults' ------------------------------
for fn in ("xb_decode", "xb_decode_dev", "xb_crf_scans", "xb_crf_scans_dev", "xb_beam_search", "xb_beam_search_dev"):
    row(fn, "n and T", {"n": 0, "T": T + 1}, INVALID, (batch(0), steps(T + 1)))
    row(fn, "T and null scores", {"T": T + 1, "scores": None}, INVALID, (steps(T + 1), null_word(fn)))
for fn in ("xb_decode_q", "xb_decode_ub_dev"):
    row(fn, "T and null seq", {"T": 0, "seq": None}, INVALID, (steps(0), "null argument"))
for fn in ("xb_crf_scans", "xb_crf_logz_dev"):
    row(fn, "T and no output", {"T": 0, "alpha": None, "beta": None, "logz": None, "post": None} if fn == "xb_crf_scans" else
        {"T": 0, "logz": None}, INVALID, (steps(0), NO_OUTPUT))
row("xb_ctc_logz", "T and null targets", {"T": 0, "targets": None}, INVALID, (steps(0), "null host pointer"))
row("xb_ctc_logz", "n and no positions", {"n": MAX_BATCH + 1, "Lt": SL - 1}, INVALID, (batch(MAX_BATCH + 1), width(SL - 1)))
row("xb_beam_search", "T and beam width", {"T": 0, "beam_width": 0}, INVALID, (steps(0), "beam_width 0 outside [1, 32]"))
for fn in ("xb_ctc_loss", "xb_ctc_loss_dev", "xb_ctc_loss_grad", "xb_ctc_loss_grad_dev"):
    who = fn[:-4] + ": " if fn.endswith("_dev") else fn + ": "
    row(fn, "n and T", {"n": 0, "T": 0}, INVALID, (batch(0, who), steps(0, who)))
    row(fn, "T and null loss", {"T": T + 1, "loss": None}, INVALID, (steps(T + 1, who), who + null_word(fn)))
    row(fn, "T and no positions", {"T": T + 1, "Lt": SL - 1}, INVALID, (steps(T + 1, who), width(SL - 1, who)))
row("xb_basecall_chunks", "n and null seq", {"n": 0, "seq": None}, INVALID, (batch(0), "null argument"), "loaded")
row("xb_submit_chunks", "n and slot", {"n": 0, "slot": SLOTS}, INVALID, (batch(0), BAD_SLOT), "loaded")


def good(fn):
    """The arguments of a call of `fn` that is accepted: name -> a scalar of SCALARS, or "buffer" for a pointer."""
    return collections.OrderedDict((name, SCALARS.get(name, "buffer")) for name in SIGNATURES[fn])


def row_id(r):
    return "%s-%s" % (r.fn, r.fault.replace(" ", "_"))
