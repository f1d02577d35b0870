"""Test infrastructure: seeded cases that take xb_map_templates to the limits of its kernels and of its contract, one family per
limit, and the condition under which a family really is at the limit it is named for.  Both tiers import this module:
tests/test_map_host.py evaluates every condition on the restatement's outputs (tests/map_ref.py) alone, tests/test_gpu_map.py
runs the same cases on the device against those outputs.  A condition is never evaluated on what the device returns, so a GPU
pass cannot come from a case that missed its edge.

A family is a function that returns a tuple of Case(reads, templates, scoring, width, lens): reads are str (or bytes where a
row holds bytes that are no letters), width is the row width W (None: the longest read), lens overrides seq_len where a case
is about lengths the rows do not have.  expected(family, arg) is the restatement's output for every case of the family,
computed once per process (functools.lru_cache) and never written to by a test.

replay() checks one mapped row on its own: it walks the reported columns and adds up their score.  It shares the letter table
with map_ref and nothing else."""
import collections
import functools
import os

import numpy as np

import map_ref

Case = collections.namedtuple("Case", "reads templates scoring width lens", defaults=(None,))
LETTERS = np.array(list("ACGT"))
DEFAULT = map_ref.DEFAULT_SCORING
CHUNK_BYTES = 16384                    # the score pass's chunk of whole templates (MAP_CHUNK_BYTES)
STRIPE = 256                           # columns of one stripe at four columns a lane, the widest: templates past it take several


def revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTXYacgt", "TGCAYXtgca"))


def random_letters(rng, n, ambiguous=0.0):
    p = [(1.0 - ambiguous) / 4] * 4 + [ambiguous]
    return "".join(rng.choice(np.array(list("ACGTN")), int(n), p=p))


def mutate(rng, t, sub=0.03, dele=0.015, ins=0.015, keep=8):
    """A noisy copy of t: substitutions, deletions, insertions of one to three letters; the template's N called X, Y or a natural
    letter; the first and last `keep` letters stay as they are, so the copy's ends are the template's."""
    out = []
    for k, c in enumerate(t):
        if c == "N":
            c = str(rng.choice(["X", "Y", "A", "G"], p=[0.6, 0.2, 0.1, 0.1]))
        v = rng.random()
        if keep <= k < len(t) - keep:
            if v < sub:
                c = str(rng.choice(LETTERS))
            elif v < sub + dele:
                c = ""
            elif v < sub + dele + ins:
                c = c + "".join(rng.choice(LETTERS, rng.integers(1, 4)))
        out.append(c)
    return "".join(out)


def mutated_reads(templates, count, rng):
    """Seeded reads off the templates: substitutions, indels, the unnatural base (the template's N) called X / Y / a natural
    letter / dropped, both strands, random flanks; 5 % unrelated sequences, empty rows, rows of one base."""
    letters = LETTERS
    reads = []
    for k in range(count):
        u = rng.random()
        if u < 0.05:
            reads.append("".join(rng.choice(letters, rng.integers(20, 140))))
            continue
        if u < 0.07:
            reads.append("")
            continue
        if u < 0.09:
            reads.append(str(rng.choice(list("ACGTXY"))))
            continue
        out = []
        for c in templates[rng.integers(len(templates))]:
            if c == "N":
                c = str(rng.choice(["X", "Y", "A", "G", ""], p=[0.5, 0.2, 0.1, 0.1, 0.1]))
            v = rng.random()
            if v < 0.04:
                c = str(rng.choice(letters))
            elif v < 0.06:
                c = ""
            elif v < 0.08:
                c = c + "".join(rng.choice(letters, rng.integers(1, 4)))
            out.append(c)
        s = "".join(rng.choice(letters, rng.integers(0, 12))) + "".join(out) + "".join(rng.choice(letters, rng.integers(0, 12)))
        lo, hi = rng.integers(0, 15), len(s) - rng.integers(0, 15)
        s = s[lo:max(hi, lo + 1)] if rng.random() < 0.3 else s
        reads.append(revcomp(s) if rng.random() < 0.5 else s)
    return reads


def poc_templates():
    from conftest import GOLDEN
    from xna_basecaller_amd.aligner import read_fasta
    return [s for _, s in read_fasta(os.path.join(GOLDEN, "poc_refdb_short.fasta"))]


def library(templates):
    """The library as the C ABI takes it: the letters concatenated (bytes) and the offsets (R + 1)."""
    off = np.zeros(len(templates) + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in templates])
    return b"".join(t if isinstance(t, bytes) else t.encode("latin-1") for t in templates), off


def pack(case):
    """(rows (n, W) int8 left-packed and zero-padded, seq_len (n) int32) of a case."""
    raw = [r if isinstance(r, bytes) else r.encode("latin-1") for r in case.reads]
    W = max(1, max(len(r) for r in raw)) if case.width is None else case.width
    rows = np.zeros((len(raw), W), np.uint8)
    for k, r in enumerate(raw):
        rows[k, :len(r)] = np.frombuffer(r, np.uint8)
    lens = np.array([len(r) for r in raw] if case.lens is None else case.lens, np.int32)
    return rows.view(np.int8), lens


def chunk_of(templates):
    """The packing rule of the library image restated: whole templates in order, a new chunk when the next one does not fit
    CHUNK_BYTES letters -> the chunk of every template."""
    out, used, chunk = [], 0, 0
    for t in templates:
        if used + len(t) > CHUNK_BYTES:
            chunk, used = chunk + 1, 0
        used += len(t)
        out.append(chunk)
    return out


# ---- one mapped row on its own ---------------------------------------------------------------------------------------------

def replay(row, length, template, out, scoring):
    """One mapped row checked against the contract's words without an alignment: row (W) int8 and its seq_len, the winning
    template's letters, out = the row's ten outputs (ops the row's (W + Lmax) bytes), the scoring.  The columns walked from
    (q_st, r_st) on the aligned strand end exactly at (q_en, r_en), '=' stands on equal codes below 4 and 'X' on nothing else,
    the columns' scores and the gap runs' costs (gap_open + k gap_extend) add up to score, 0 <= second <= score, ops is zero
    behind n_ops and strand is +1 or -1.  Raises AssertionError."""
    match, mismatch, go, ge, amb = (int(v) for v in scoring)
    strand, score, second = int(out["strand"]), int(out["score"]), int(out["second"])
    assert strand in (1, -1), ("strand", strand)
    assert score > 0 and 0 <= second <= score, ("score, second", score, second)
    row = np.asarray(row).astype(np.int8).view(np.uint8)
    n = min(max(int(length), 0), row.shape[0])
    q = map_ref._CODE[row[:n]]
    if strand == -1:
        q = q[::-1]
        q = np.where(q < 4, 3 - q, 4)
    t = map_ref._CODE[np.frombuffer(template if isinstance(template, bytes) else template.encode("latin-1"), np.uint8)]
    ops = np.asarray(out["ops"], np.uint8)
    n_ops = int(out["n_ops"])
    assert 0 < n_ops <= ops.shape[0] and not ops[n_ops:].any(), ("n_ops", n_ops, ops.shape)
    i, j = int(out["q_st"]), int(out["r_st"])
    assert 0 <= i <= n and 0 <= j <= len(t), ("start", i, j)
    total, prev = 0, ""
    for k, op in enumerate(ops[:n_ops].tobytes().decode("latin-1")):
        if op in "=X":
            assert i < n and j < len(t), ("column past an end", k, i, j)
            equal = bool(q[i] < 4 and q[i] == t[j])
            assert equal == (op == "="), ("column", k, op, int(q[i]), int(t[j]))
            total += match if equal else (-amb if (q[i] == 4 or t[j] == 4) else -mismatch)
            i, j = i + 1, j + 1
        elif op == "I":
            assert i < n, ("insertion past the row's end", k, i)
            total -= ge + (go if prev != "I" else 0)
            i += 1
        elif op == "D":
            assert j < len(t), ("deletion past the template's end", k, j)
            total -= ge + (go if prev != "D" else 0)
            j += 1
        else:
            raise AssertionError(("byte that is no column", k, op))
        prev = op
    assert (i, j) == (int(out["q_en"]), int(out["r_en"])), ("end", (i, j), (int(out["q_en"]), int(out["r_en"])))
    assert total == score, ("score", total, score)


def replay_all(case, out):
    """replay() on every mapped row of `out` (the ten arrays for the case's rows); the number of mapped rows."""
    rows, lens = pack(case)
    mapped = np.flatnonzero(out["tmpl"] >= 0)
    for r in mapped:
        try:
            replay(rows[r], lens[r], case.templates[int(out["tmpl"][r])], {k: out[k][r] for k in out}, case.scoring)
        except AssertionError as e:
            raise AssertionError(("row", int(r)) + tuple(e.args)) from None
    return mapped.size


def d_runs(ops, r_st):
    """The runs of D of one row's columns as (first, last) template columns (0-based, inclusive)."""
    out, j, start = [], int(r_st), None
    for op in bytes(ops).rstrip(b"\0").decode("latin-1"):
        if op == "D":
            start = j if start is None else start
        elif start is not None:
            out.append((start, j - 1))
            start = None
        j += op in "=XD"
    return out


# ---- the families ----------------------------------------------------------------------------------------------------------

STRIPE_LENGTHS = (127, 128, 255, 256, 257, 512, 513)
GAP_SCORING = (2, 4, 24, 1, 1)         # extending a gap across the stripe boundary beats opening a second one


@functools.lru_cache(maxsize=None)
def stripes(length):
    """A last stripe exactly full and one column into a new one, at two and at four columns a lane.  Past one stripe (length
    >= 257): reads that equal a template without its letters 250..262 (a D run over the boundary between columns 255 and 256,
    which only the E handed from stripe to stripe carries) and with 12 letters inserted after letter 255."""
    rng = np.random.default_rng(1000 + length)
    templates = [random_letters(rng, length) for _ in range(3)] + [random_letters(rng, length // 2)]
    reads = []
    for k in range(20):
        s = mutate(rng, templates[k % 4], keep=4 if k % 3 else 0)
        s = random_letters(rng, rng.integers(0, 10)) + s + random_letters(rng, rng.integers(0, 10)) if k % 5 == 0 else s
        reads.append(revcomp(s) if k % 2 else s)
    if length > STRIPE:
        for k in range(2):
            t = templates[k]
            s = t[:250] + t[263:]
            reads.append(revcomp(s) if k else s)
        for k in range(2):
            t = templates[2 - k]
            s = t[:256] + random_letters(rng, 12) + t[256:]
            reads.append(revcomp(s) if k else s)
    return tuple(Case(reads, templates, sc, None) for sc in (DEFAULT, GAP_SCORING))


def stripes_condition(length, cases, wants):
    """Every length: some winner ends in the template's last column and some starts in its first.  Past one stripe: some
    winner spans the boundary (r_st < 256 < r_en) under both scorings.  A D run that holds the columns 256 and 257 (E goes from
    one stripe to the next inside it) needs template letters behind it to end on, since a local alignment never ends in a gap:
    lengths 512 and 513 have one on each strand under both scorings (the run 250..262 holds the two columns counted from 0 and
    counted from 1); at 257, where the first column of the second stripe is the last of all, no optimal alignment can have one."""
    for case, w in zip(cases, wants):
        won = w["tmpl"] >= 0
        ends = np.array([len(case.templates[t]) for t in w["tmpl"][won]])
        assert (w["r_en"][won] == ends).any() and (w["r_st"][won] == 0).any()
        if length <= STRIPE:
            continue
        assert ((w["r_st"] < STRIPE) & (w["r_en"] > STRIPE) & won).any()
        if length > STRIPE + 1:
            over = [r for r in np.flatnonzero(won) if any(a <= 255 and b >= 257 for a, b in d_runs(w["ops"][r], w["r_st"][r]))]
            assert len(over) >= 2, "no D run across the stripe boundary"
            assert {int(w["strand"][r]) for r in over} == {1, -1}


MIXED_LENGTHS = (300, 256, 255, 129, 128, 65, 64, 3, 1)


def _without(rng, n, banned):
    """n random letters in which no three in a row are one of `banned`."""
    s = ""
    while len(s) < n:
        c = str(rng.choice(LETTERS))
        if (s[-2:] + c) not in banned:
            s += c
    return s


@functools.lru_cache(maxsize=None)
def mixed_lengths():
    """One library whose longest template (300) puts every template on four columns a lane and two stripes: templates of 1,
    64, 65 and 128 letters run on a plan made for another length.  The long templates hold neither TTT nor AAA, so the
    3-letter template TTT is the only home of a read TTT on either strand."""
    rng = np.random.default_rng(77)
    templates = [_without(rng, L, ("TTT", "AAA")) for L in MIXED_LENGTHS[:-2]] + ["TTT", "T"]
    reads = []
    for t in templates[:-2]:
        for k in range(4):
            s = mutate(rng, t, keep=3)
            reads.append(revcomp(s) if k % 2 else s)
    reads += ["TTT", "AAA", "T", "GTTTG"]
    return (Case(reads, templates, DEFAULT, None),)


def mixed_lengths_condition(_, cases, wants):
    (case,), (w,) = cases, wants
    for t, tpl in enumerate(case.templates):
        if len(tpl) >= 64:
            for strand in (1, -1):
                assert ((w["tmpl"] == t) & (w["strand"] == strand)).any(), (t, strand)
    assert (w["tmpl"] >= len(case.templates) - 2).any()
    assert ((w["tmpl"] == len(case.templates) - 2) & (w["strand"] == -1)).any()      # AAA: the 3-letter template's minus strand


# The widths at which map_score_waves (xb_align.hip) changes the score workgroup's size for a library past one stripe, as it
# is now: fit = 32768 / (8 (W + 1)) waves, at most four -- four up to W = 1023, three up to 1364, two up to 2047, one from
# 2048; 4096 is the widest row.  They must be recomputed if map_score_waves changes.
WAVE_WIDTHS = (1023, 1024, 1364, 1365, 2047, 2048, 4096)


@functools.lru_cache(maxsize=None)
def wave_counts(W):
    """Twelve templates (24 pairs: several for every wave at every workgroup size), the longest of 257 letters so that every
    wave needs its stripe hand-off column; short reads in rows of width W, and two reads of exactly W letters with a template's
    copy at the far end of the aligned strand."""
    rng = np.random.default_rng(2000 + W)
    templates = [random_letters(rng, 257)] + [random_letters(rng, rng.integers(100, 258)) for _ in range(11)]
    reads = []
    for k in range(16):
        s = mutate(rng, templates[(5 * k) % 12])
        n = int(rng.integers(100, min(400, W) + 1))
        if len(s) < n:
            a = int(rng.integers(0, n - len(s) + 1))
            s = random_letters(rng, a) + s + random_letters(rng, n - len(s) - a)
        else:
            s = s[:n]
        reads.append(revcomp(s) if k % 2 else s)
    for k, t in enumerate((templates[3], templates[0])):
        copy = mutate(rng, t[-200:])
        s = random_letters(rng, W - len(copy)) + copy          # plus strand: the copy is the row's last letters
        reads.append(revcomp(s) if k else s)                    # minus strand: its reverse complement opens the row
    return (Case(reads, templates, DEFAULT, W),)


def wave_counts_condition(W, cases, wants):
    (case,), (w,) = cases, wants
    assert len(case.reads[-2]) == len(case.reads[-1]) == W
    assert (w["tmpl"][-2], w["strand"][-2]) == (3, 1) and w["q_en"][-2] >= W - 5 and w["r_en"][-2] == len(case.templates[3])
    assert (w["tmpl"][-1], w["strand"][-1]) == (0, -1) and w["q_en"][-1] >= W - 5 and w["r_en"][-1] == 257
    assert (w["tmpl"][:16] >= 0).sum() >= 14 and len(set(w["tmpl"][:16].tolist())) >= 8


# The widths on either side of map_trace_in_lds (xb_align.hip) at Lmax = 64, as it is now: the trace workgroup's fixed LDS
# (the row, the template and the ops, each rounded up to 16 bytes) and W * 64 direction bytes are 65536 bytes at W = 991, the
# whole of the 64 KiB, and 65600 at W = 992, which goes to the context's scratch.  They must be recomputed if it changes.
TRACE_WIDTHS = (991, 992)


@functools.lru_cache(maxsize=None)
def trace_boundary(W):
    rng = np.random.default_rng(3000)                  # the same letters at both widths
    templates = [random_letters(rng, L) for L in (64, 40, 17)]
    far = [random_letters(rng, 992) for _ in range(2)]
    reads = []
    for k, t in enumerate(templates[:2]):
        s = far[k][:W - len(t)] + t                    # the copy in the last 70 letters of the aligned strand
        reads.append(revcomp(s) if k else s)
    for k, t in enumerate(templates[:2]):
        s = t + far[1 - k][:W - len(t)]                # the copy in the first 70
        reads.append(revcomp(s) if k else s)
    for k in range(4):
        s = mutate(rng, templates[k % 3], keep=2)
        reads.append(revcomp(s) if k % 2 else s)
    return (Case(reads, templates, DEFAULT, W),)


def trace_boundary_condition(W, cases, wants):
    (case,), (w,) = cases, wants
    assert all(len(r) == W for r in case.reads[:4])
    assert w["tmpl"][:4].tolist() == [0, 1, 0, 1] and w["strand"][:4].tolist() == [1, -1, 1, -1]
    assert (w["q_en"][:4] == W).sum() == 2 and (w["q_st"][:4] == 0).sum() == 2
    assert (w["n_ops"][:4] >= 40).all()


@functools.lru_cache(maxsize=None)
def full_size():
    """The widest row against the longest templates: direction bytes in the context's scratch, one score wave, 16 stripes; 24
    rows are more than the 16 trace workgroups the scratch bound leaves at this size, so rows take turns on a workgroup's
    scratch."""
    rng = np.random.default_rng(4096)
    templates = [random_letters(rng, 4096, 0.02), random_letters(rng, 4095, 0.02)]
    reads = []
    for k in range(4):
        s = mutate(rng, templates[k % 2], sub=0.02, dele=0.015, ins=0.015)[-4096:]      # the template's end is the read's end
        reads.append(revcomp(s) if k >= 2 else s)
    for k in range(20):
        t = templates[k % 2]
        a = len(t) - 300 + int(rng.integers(0, 60))
        s = mutate(rng, t[a:a + int(rng.integers(200, 301))], keep=3)
        s = random_letters(rng, rng.integers(0, 50)) + s + random_letters(rng, rng.integers(0, 50))
        reads.append(revcomp(s) if k % 4 >= 2 else s)
    return (Case(reads, templates, DEFAULT, 4096),)


def full_size_condition(_, cases, wants):
    (case,), (w,) = cases, wants
    assert len(case.reads) == 24 and all(len(r) == 4096 for r in case.reads[:4]) and all(200 <= len(r) <= 400 for r in case.reads[4:])
    assert w["tmpl"][:4].tolist() == [0, 1, 0, 1] and w["strand"][:4].tolist() == [1, 1, -1, -1]
    assert (w["n_ops"] > 4096).any()
    assert ((w["tmpl"] == 0) & (w["r_en"] == 4096)).any() and ((w["tmpl"] == 1) & (w["r_en"] == 4095)).any()
    assert (w["r_st"][4:] > 3700).any() and (w["strand"][4:] == -1).any() and (w["strand"][4:] == 1).any()


@functools.lru_cache(maxsize=None)
def chunking():
    """Four libraries: (a) a chunk exactly full, (b) a template that misses the space left by one letter, (c) five chunks with a
    template repeated five chunks on and a runner-up in another chunk than the winner, (d) a template that is its own reverse
    complement, whose two strands go to different waves."""
    rng = np.random.default_rng(16384)
    out = []
    for lengths in ((4096, 4096, 4096, 4096, 1), (4096, 4096, 4096, 4095, 2)):
        templates = [random_letters(rng, L) for L in lengths]
        reads = []
        for k in range(4):
            a = int(rng.integers(0, 3900))
            s = mutate(rng, templates[k][a:a + 90], keep=2)
            reads.append(revcomp(s) if k % 2 else s)
        reads += [mutate(rng, templates[3][-80:], keep=2), templates[4], revcomp(templates[4])]
        out.append(Case(reads, templates, DEFAULT, None))
    # (c)
    templates = [random_letters(rng, 2000) for _ in range(40)]
    templates[39] = templates[1]
    templates[3] = mutate(rng, templates[38], sub=0.10, dele=0.0, ins=0.0, keep=0)
    reads = []
    for k in range(3):
        a = 300 + 500 * k
        s = mutate(rng, templates[1][a:a + 100], keep=2)
        reads.append(revcomp(s) if k == 1 else s)
    for k in range(3):
        a = 200 + 600 * k
        s = mutate(rng, templates[38][a:a + 100], sub=0.01, dele=0.01, ins=0.01, keep=2)
        reads.append(revcomp(s) if k == 1 else s)
    out.append(Case(reads, templates, DEFAULT, None))
    # (d)
    templates = [random_letters(rng, 120) for _ in range(12)]
    half = random_letters(rng, 60)
    templates[5] = half + revcomp(half)
    reads = [templates[5], mutate(rng, templates[5], keep=2)]
    for k in (0, 4, 6, 11):
        s = mutate(rng, templates[k], keep=2)
        reads.append(revcomp(s) if k % 4 else s)
    out.append(Case(reads, templates, DEFAULT, None))
    return tuple(out)


def chunking_condition(_, cases, wants):
    a, b, c, d = cases
    assert chunk_of(a.templates) == [0, 0, 0, 0, 1] and sum(len(t) for t in a.templates[:4]) == CHUNK_BYTES
    assert chunk_of(b.templates) == [0, 0, 0, 0, 1] and sum(len(t) for t in b.templates) == CHUNK_BYTES + 1
    for case, w in ((a, wants[0]), (b, wants[1])):
        assert w["tmpl"][:5].tolist() == [0, 1, 2, 3, 3] and (w["tmpl"][5:] >= 0).all()
    chunks = chunk_of(c.templates)
    assert chunks == [k // 8 for k in range(40)]
    w = wants[2]
    assert w["tmpl"][:3].tolist() == [1, 1, 1] and np.array_equal(w["second"][:3], w["score"][:3]) and (w["strand"][:3] == -1).any()
    assert w["tmpl"][3:].tolist() == [38, 38, 38]
    for r in range(3, 6):                                   # the runner-up is template 3, in chunk 0; the winner is in chunk 4
        alone = map_ref.map_read(c.reads[r], [c.templates[3]])
        assert alone["score"] == w["second"][r] > 0 and chunks[3] != chunks[38]
        rest = [t for k, t in enumerate(c.templates) if k not in (3, 38)]
        assert map_ref.map_read(c.reads[r], rest)["score"] < w["second"][r]
    w = wants[3]
    t5 = d.templates[5]
    assert revcomp(t5) == t5
    for r in range(2):
        assert w["tmpl"][r] == 5 and w["strand"][r] == 1 and w["second"][r] < w["score"][r] // 2
        for s in (d.reads[r], revcomp(d.reads[r])):          # both strands of template 5 reach the winner's score
            assert map_ref.map_read(s, [t5])["score"] == w["score"][r] and map_ref.map_read(s, [t5])["strand"] == 1
        others = [t for k, t in enumerate(d.templates) if k != 5]
        assert map_ref.map_read(d.reads[r], others)["score"] == w["second"][r]
    assert (w["tmpl"][2:] == [0, 4, 6, 11]).all()


ZERO_PENALTIES = ((1, 0, 0, 0, 0), (2, 0, 0, 0, 0))
SCORINGS = ZERO_PENALTIES + ((0, 4, 4, 2, 1), (2, 4, 0, 2, 1), (2, 4, 4, 0, 1), (2, 4, 4, 2, 0), (1000, 1000, 1000, 1000, 1000))


@functools.lru_cache(maxsize=None)
def scorings():
    """The corners of the scoring's range on the POC library: no penalties at all (every cell ties, every tie rule of the trace
    fires), each value 0 in turn, every value 1000; and 1000 a match over 4096 letters, the largest score there is."""
    templates = poc_templates()
    reads = mutated_reads(templates, 60, np.random.default_rng(23))
    out = [Case(reads, templates, sc, None) for sc in SCORINGS]
    own = random_letters(np.random.default_rng(24), 4096)
    out.append(Case([own], [own], (1000, 0, 0, 0, 0), None))
    return tuple(out)


def scorings_condition(_, cases, wants):
    for case, w in zip(cases, wants):
        if case.scoring in ZERO_PENALTIES:
            seen = set(w["ops"][w["tmpl"] >= 0].tobytes())
            assert seen >= set(b"=XID"), (case.scoring, seen)
        if case.scoring[0] == 0:
            assert (w["tmpl"] == -1).all() and not w["ops"].any() and not w["score"].any()
        elif len(case.reads) > 1:
            assert (w["tmpl"] >= 0).sum() >= 50
    assert wants[-1]["score"].tolist() == [4096000] and wants[-1]["n_ops"].tolist() == [4096]


@functools.lru_cache(maxsize=None)
def letters_and_lengths():
    """What the header says of bytes and lengths: lower case is the same letter in rows and templates, every other byte is
    ambiguous (NUL, '-', bytes with the top bit set), and a seq_len outside [0, W] is clamped -- up to W, the row's zero
    padding is then aligned as ambiguous letters."""
    rng = np.random.default_rng(99)
    templates = [random_letters(rng, 90, 0.03) for _ in range(4)]
    reads = [mutate(rng, templates[k % 4], keep=2) for k in range(8)]
    reads = [revcomp(s) if k % 2 else s for k, s in enumerate(reads)]
    mixed = ["".join(c.lower() if rng.random() < 0.5 else c for c in s) for s in reads]
    out = [Case([s.lower() for s in reads] + mixed, templates, DEFAULT, None),
           Case(reads + mixed, [t.lower() for t in templates[:2]] + templates[2:], DEFAULT, None)]
    odd = []
    for k, s in enumerate(reads):
        b = bytearray(s.encode("ascii"))
        for at, v in zip((11, 23, 37, 52), (0, ord("-"), 0x80, 0xff)):
            b[at + k] = v
        odd.append(bytes(b))
    odd += [bytes([0, 0x80, 0xff, 0x2d] * 5), b"\0" * 30 + reads[0].encode("ascii")]
    out.append(Case(odd, templates, DEFAULT, None))
    W = 120
    short = [s[:60] for s in reads[:4]]                    # 60 letters and 60 bytes of zero padding in a row of 120
    rows = [short[0], short[1], short[2], short[2]] + short + [reads[4][:W].ljust(W, "A")] * 2
    lens = [-5, 0, W, W + 9, 60, 59, 61, 1, W, W + 9]
    out.append(Case(rows, templates, DEFAULT, W, tuple(lens)))
    return tuple(out)


def letters_and_lengths_condition(_, cases, wants):
    lower, tl, odd, lengths = wants
    assert (lower["tmpl"] >= 0).all() and (tl["tmpl"] >= 0).all()
    for k in KEYS:                                          # case changes nothing
        assert np.array_equal(lower[k][:8], lower[k][8:]) and np.array_equal(lower[k], tl[k]), k
    assert (odd["tmpl"][:8] >= 0).all() and odd["tmpl"][8] == -1 and odd["q_st"][9] == 30
    assert (odd["ops"][:8] == ord("X")).any()
    w = lengths
    assert w["tmpl"][:2].tolist() == [-1, -1] and (w["tmpl"][2:] >= 0).all()
    for k in KEYS:                                          # W + 9 is W
        assert np.array_equal(w[k][2], w[k][3]) and np.array_equal(w[k][8], w[k][9]), k
    assert w["q_en"][8] > 60


KEYS = ("tmpl", "strand", "score", "second", "q_st", "q_en", "r_st", "r_en", "n_ops", "ops")

# family name -> (generator, its arguments (None: it takes none), its condition)
FAMILIES = {
    "stripes": (stripes, STRIPE_LENGTHS, stripes_condition),
    "mixed_lengths": (mixed_lengths, (None,), mixed_lengths_condition),
    "wave_counts": (wave_counts, WAVE_WIDTHS, wave_counts_condition),
    "trace_boundary": (trace_boundary, TRACE_WIDTHS, trace_boundary_condition),
    "full_size": (full_size, (None,), full_size_condition),
    "chunking": (chunking, (None,), chunking_condition),
    "scorings": (scorings, (None,), scorings_condition),
    "letters_and_lengths": (letters_and_lengths, (None,), letters_and_lengths_condition),
}


def cases(family, arg=None):
    make = FAMILIES[family][0]
    return make() if arg is None else make(arg)


@functools.lru_cache(maxsize=None)
def expected(family, arg=None):
    """The restatement's outputs for every case of the family, computed once; read-only (the arrays refuse writes)."""
    out = []
    for case in cases(family, arg):
        rows, lens = pack(case)
        want = map_ref.map_rows(rows, lens, case.templates, case.scoring)
        for v in want.values():
            v.setflags(write=False)
        out.append(want)
    return tuple(out)


def condition(family, arg=None):
    FAMILIES[family][2](arg, cases(family, arg), expected(family, arg))
