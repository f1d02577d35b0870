"""GPU: xb_barcode_dist through the C ABI against the CPU restatement of its contract (tests/bcdist_ref.py): the four outputs
equal, integer for integer.  The mapper's outputs are built by hand where a clamp, a clipped window or a tie has to be hit, or
come from xb_map_templates itself on seeded calls.  The per-row function is pinned to the reference by tests/golden/bcdist.json
(tests/test_bcdist_host.py); the mapping is this package's own."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import bcdist_ref
import map_ref
import ubtally_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

LETTERS = np.array(list("ACGT"))
P5 = "GATTACAGGCTTAACGTCTGAGTCC"                # 25 letters
P3 = "CATGNCAAGTTGCATGCCAGTTGAC"


def _ctx():
    from xna_basecaller_amd import _lib
    _lib.require_gpu()
    return _lib.mapper_context(0)


def _library(templates):
    off = np.zeros(len(templates) + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in templates])
    return "".join(templates).encode("latin-1"), off


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTXY", "TGCAYX"))


def _check(ctx, rows, lens, got, templates, bc_pos, bc_len, relax):
    lib, off = _library(templates)
    out = ctx.barcode_dist(rows, lens, got, lib, off, bc_pos, bc_len, relax)
    want = bcdist_ref.dist(rows, lens, got, templates, bc_pos, bc_len, relax)
    for k in bcdist_ref.OUTPUTS:
        assert out[k].dtype == np.int32 and out[k].shape == (rows.shape[0],)
        bad = np.flatnonzero(out[k] != want[k])
        assert bad.size == 0, (k, bad[:5], out[k][bad[:5]], want[k][bad[:5]], bc_pos, bc_len, relax)
    return out


def _family(rng, bc_pos, bc_len, count=4):
    """Templates that share their primers and differ in the barcode at bc_pos, of unequal lengths, and three odd ones: the
    barcode clipped by the template's end, a template that ends where the barcode would start, one of a single letter."""
    head = "".join(rng.choice(LETTERS, bc_pos))
    out = []
    for k in range(count):
        out.append(head + "".join(rng.choice(LETTERS, bc_len)) + P3 + "ACGT" * k)
    out.append(head + "".join(rng.choice(LETTERS, bc_len))[:max(bc_len // 2, 1)])
    out.append(head if head else "A")
    out.append("G")
    return out


def _noisy(rng, tpl, rate=0.06):
    out = []
    for c in tpl:
        if c == "N":
            c = str(rng.choice(["X", "Y", "A", ""]))
        v = rng.random()
        if v < rate:
            c = str(rng.choice(LETTERS))
        elif v < 2 * rate:
            c = ""
        elif v < 2.5 * rate:
            c = c + str(rng.choice(LETTERS))
        out.append(c)
    return "".join(out)


def _by_hand(rng, templates, n, width, q_far=False):
    """n rows of `width` with mapper outputs made up: a noisy call off a template on either strand, q_st and r_st anywhere
    near the ends, some rows unmapped or empty.  q_far: the call sits at the far end of the row behind filler letters."""
    reads, got = [], {k: np.zeros(n, np.int32) for k in ("tmpl", "q_st", "r_st")}
    got["strand"] = np.zeros(n, np.int8)
    for r in range(n):
        t = int(rng.integers(len(templates)))
        call = _noisy(rng, templates[t])
        q_st = int(rng.integers(0, 6))
        if q_far:
            q_st = width - len(templates[t]) - int(rng.integers(0, 12))
        call = ("".join(rng.choice(LETTERS, q_st)) + call)[:width]
        u = rng.random()
        got["tmpl"][r] = -1 if u < 0.05 else t
        got["strand"][r] = -1 if rng.random() < 0.5 else 1
        got["q_st"][r] = q_st + int(rng.integers(-2, 3))
        got["r_st"][r] = int(rng.choice([0, 0, 0, 3, 12, 30, 60]))
        reads.append("" if 0.05 <= u < 0.08 else (_revcomp(call) if got["strand"][r] < 0 else call))
    rows, lens = map_ref.pack_rows(reads, width)
    return rows, lens, got


# ---- the geometry of the barcode -------------------------------------------------------------------------------------------
@pytest.mark.parametrize("relax", [0, 3, 8])
@pytest.mark.parametrize("bc_len", [1, 24, 30, 63, 64])
def test_barcode_lengths_and_relax(bc_len, relax):
    ctx = _ctx()
    rng = np.random.default_rng(100 * bc_len + relax)
    bc_pos = 25
    templates = _family(rng, bc_pos, bc_len)
    rows, lens, got = _by_hand(rng, templates, 65, 160)
    out = _check(ctx, rows, lens, got, templates, bc_pos, bc_len, relax)
    mapped = got["tmpl"] >= 0
    assert (out["bc_dist"][~mapped] == -1).all() and (out["bc_dist"][mapped] >= 0).all()
    assert (out["bc_end"][mapped] - out["bc_start"][mapped] == bc_len).all()
    # the templates whose barcode is clipped and empty were hit, and an empty barcode's distance is what was observed
    assert set(np.unique(got["tmpl"][mapped])) == set(range(len(templates)))
    empty = mapped & (got["tmpl"] >= len(templates) - 2)
    assert (out["bc_dist"][empty] == out["bc_obs_len"][empty]).all()
    ctx.close()


# ---- mapper outputs built by hand -------------------------------------------------------------------------------------------
BC = "ACGTTGCAAGCTTCGATCCGATAG"
HAND_TEMPLATES = [P5 + BC + P3,                                            # 0: the POC shape
                  P5 + "ACGTTGCAXGCTTCGATCYGATAG" + P3,                     # 1: X and Y spelled out inside the barcode
                  P5 + "A" * 24 + P3,                                       # 2: a homopolymer barcode
                  (P5 + BC).lower() + P3,                                   # 3: lower case
                  P5 + "ACGT\xe9TGCAAGCTTCGATCCGATAG"[:24] + P3]           # 4: a byte outside ASCII inside the barcode
HAND_W = 96


def _hand(cases):
    n = len(cases)
    rows = np.zeros((n, HAND_W), np.int8)
    lens = np.zeros(n, np.int32)
    got = {k: np.zeros(n, np.int32) for k in ("tmpl", "q_st", "r_st")}
    got["strand"] = np.zeros(n, np.int8)
    for k, c in enumerate(cases):
        seq = c["seq"].encode("latin-1")
        rows[k, :len(seq)] = np.frombuffer(seq, np.int8)
        lens[k] = c.get("seq_len", len(seq))
        for f in ("tmpl", "strand", "q_st", "r_st"):
            got[f][k] = c[f]
    return rows, lens, got


def _row(seq, tmpl=0, strand=1, q_st=0, r_st=0, **more):
    return dict(seq=seq, tmpl=tmpl, strand=strand, q_st=q_st, r_st=r_st, **more)


def test_hand_built_rows():
    ctx = _ctx()
    t0, t1, t2 = (HAND_TEMPLATES[k].replace("N", "X") for k in range(3))
    cases = [
        _row(t0),                                                           # 0 exact: (0, 25, 49, 24)
        _row(_revcomp(t0), strand=-1),                                      # 1
        _row(t0[31:], r_st=31),                                             # 2 r_st > q_st + bc_pos: start clamped to 0
        _row(t0[24:], r_st=24),                                             # 3 start 1: windows 0 .. 4, fewer than 7
        _row(t0[25:], r_st=25, strand=0),                                   # 4 start 0: windows 0 .. 3; strand 0 is forward
        _row(t0[:40]),                                                      # 5 obs short: 15 letters at the best window
        _row(t0[:22]),                                                      # 6 obs empty at every window
        _row(t0[:23]),                                                      # 7 one letter (a T) in the first window, then none
        _row(_revcomp(t1), tmpl=1, strand=-1),                              # 8 X / Y in the window, reverse strand: 0
        _row(_revcomp(t1).translate(str.maketrans("XY", "YX")), tmpl=1, strand=-1),     # 9 ... swapped: 2
        _row(t1, tmpl=1),                                                   # 10
        _row(P5 + "A" * 34 + P3, tmpl=2),                                   # 11 windows 25 .. 28 tie at 0: 25 wins
        _row("A" * 70, tmpl=2, strand=-1),                                  # 12 (all T on the aligned strand) every window ties
        _row("A" * 70, tmpl=2),                                             # 13 every window ties at 0: the first, 22
        _row(t0, tmpl=-1),                                                  # 14 unmapped
        _row(t0, tmpl=len(HAND_TEMPLATES)),                                 # 15
        _row(t0, tmpl=-70000),                                              # 16
        _row("", tmpl=0),                                                   # 17 an empty row
        _row(t0, q_st=400),                                                 # 18 q_st beyond seq_len: clamped to it
        _row(t0, q_st=-7),                                                  # 19 ... below 0
        _row(t0, seq_len=4000),                                             # 20 seq_len beyond the width
        _row(t0, seq_len=-3),                                               # 21 ... below 0
        _row(t0, r_st=-4),                                                  # 22 r_st below 0
        _row(t0, r_st=5000),                                                # 23 ... beyond the template
        _row(t0.lower()),                                                   # 24 a lower-case call
        _row(t0, tmpl=3),                                                   # 25 a lower-case template
        _row(HAND_TEMPLATES[4].replace("N", "X"), tmpl=4),                  # 26 the byte outside ASCII on both sides: equal
        _row(_revcomp(HAND_TEMPLATES[4].replace("N", "X")), tmpl=4, strand=-1),        # 27 ... and it has no complement
        _row("GG" + t0[:10] + t0[12:], q_st=2),                             # 28 a deletion before the barcode: window 23
        _row(t0[:25] + BC[:10] + "T" + BC[10:] + t0[49:]),                  # 29 an insertion inside pushes the last letter out: 2
    ]
    rows, lens, got = _hand(cases)
    out = _check(ctx, rows, lens, got, HAND_TEMPLATES, 25, 24, 3)
    four = lambda k: [int(out[f][k]) for f in bcdist_ref.OUTPUTS]            # noqa: E731
    assert four(0) == [0, 25, 49, 24] and four(1) == [0, 25, 49, 24]
    assert four(2)[1] == 0 and four(3)[:2] == [0, 1] and four(4) == [0, 0, 24, 24]
    assert four(5) == [9, 25, 49, 15] and four(6) == [24, 22, 46, 0] and four(7) == [23, 22, 46, 1]
    assert four(8) == [0, 25, 49, 24] and four(9)[0] == 2 and four(10)[0] == 0
    assert four(11) == [0, 25, 49, 24] and four(13) == [0, 22, 46, 24] and four(12) == [24, 22, 46, 24]
    assert four(14) == four(15) == four(16) == [-1, 0, 0, 0]
    assert four(17) == [24, 22, 46, 0]
    assert four(24) == [0, 25, 49, 24] and four(25) == [0, 25, 49, 24] and four(26)[0] == 0 and four(27)[0] == 0
    assert four(28) == [0, 25, 49, 24] and four(29)[0] == 2
    ctx.close()


# ---- batch shapes ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 65, 257])
@pytest.mark.parametrize("width", [37, 4096])
def test_batch_shapes(width, n):
    ctx = _ctx()
    rng = np.random.default_rng(width + n)
    bc_pos, bc_len = (5, 24) if width == 37 else (23, 30)
    templates = _family(rng, bc_pos, bc_len)
    assert len({len(t) for t in templates}) == len(templates)                 # the offsets matter
    rows, lens, got = _by_hand(rng, templates, n, width, q_far=width == 4096)
    out = _check(ctx, rows, lens, got, templates, bc_pos, bc_len, 3)
    if width == 4096 and n > 1:                                              # the barcode was looked for at the row's far end
        assert out["bc_start"].max() > 3900 and (out["bc_obs_len"] < bc_len)[got["tmpl"] >= 0].any()
    ctx.close()


# ---- through the mapper -----------------------------------------------------------------------------------------------------
def test_through_the_mapper_and_the_dev_form():
    import torch
    ctx = _ctx()
    rng = np.random.default_rng(9)
    templates = [P5 + "".join(rng.choice(LETTERS, 24)) + P3 + "TTGACA"[:k] for k in range(6)]
    reads = []
    for k in range(130):
        call = _noisy(rng, templates[k % len(templates)], rate=0.05)
        if k % 7 == 0:                                                      # the barcode itself garbled
            call = call[:25] + "".join(rng.choice(LETTERS, 24)) + call[49:]
        if k % 11 == 0:
            call = call[int(rng.integers(1, 30)):]                          # the mapping starts inside the template
        reads.append(_revcomp(call) if k % 2 else call)
    reads += ["", "".join(rng.choice(LETTERS, 9))]
    rows, lens = map_ref.pack_rows(reads)
    lib, off = _library(templates)
    got = ctx.map_templates(rows, lens, lib, off)
    assert (got["tmpl"] >= 0).sum() >= 128 and (got["r_st"] > 0).any() and (got["strand"] < 0).any()
    out = _check(ctx, rows, lens, got, templates, 25, 24, 3)
    mapped = got["tmpl"] >= 0
    assert (out["bc_dist"][mapped] <= 5).sum() > 60 and (out["bc_dist"][mapped] > 5).sum() > 5
    dev = torch.device("cuda:0")
    d_rows, d_lens = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
    d_got = {k: torch.from_numpy(got[k]).to(dev) for k in ctx.BC_INPUTS}
    d_out = {k: torch.full((len(reads),), 77, dtype=torch.int32, device=dev) for k in ctx.BC_OUTPUTS}
    torch.cuda.synchronize()
    ctx.barcode_dist_dev(d_rows.data_ptr(), d_lens.data_ptr(), len(reads), rows.shape[1], {k: t.data_ptr() for k, t in d_got.items()},
                         lib, off, 25, 24, 3, {k: t.data_ptr() for k, t in d_out.items()})
    ctx.synchronize()
    for k in ctx.BC_OUTPUTS:
        assert np.array_equal(d_out[k].cpu().numpy(), out[k]), k
    ctx.close()


# ---- invalid arguments: argument checking only ------------------------------------------------------------------------------
def test_invalid_arguments_are_refused_and_the_context_survives():
    from xna_basecaller_amd import _lib
    ctx = _ctx()
    rows, lens, got = _hand([_row(HAND_TEMPLATES[0].replace("N", "X"))])
    lib, off = _library(HAND_TEMPLATES)
    for bad in (dict(bc_len=0), dict(bc_len=65), dict(relax=9), dict(bc_pos=-1), dict(relax=-1)):
        arg = dict(dict(bc_pos=25, bc_len=24, relax=3), **bad)
        with pytest.raises(_lib.XbError) as e:
            ctx.barcode_dist(rows, lens, got, lib, off, **arg)
        assert e.value.code == _lib.XB_ERR_INVALID and "xb_barcode_dist" in str(e.value), bad
        assert ("%s = %d" % next(iter(bad.items()))) in str(e.value), (bad, str(e.value))
        out = ctx.barcode_dist(rows, lens, got, lib, off, 25, 24, 3)        # the next valid call works
        assert [int(out[f][0]) for f in bcdist_ref.OUTPUTS] == [0, 25, 49, 24]
    long_lib, long_off = _library([HAND_TEMPLATES[0], "A" * 4097])
    with pytest.raises(_lib.XbError) as e:
        ctx.barcode_dist(rows, lens, got, long_lib, long_off, 25, 24, 3)
    assert e.value.code == _lib.XB_ERR_INVALID and "4097" in str(e.value) and "xb_barcode_dist" in str(e.value)
    _check(ctx, rows, lens, got, HAND_TEMPLATES, 25, 24, 3)
    ctx.close()


# ---- the command line: analyze -d over a PAF written here ---------------------------------------------------------------------
TODAY = ["num_aligned_reads", "target_acc", "read_acc", "err_far_ub", "err_close_ub", "err_only_ub", "err_ub_d_1", "err_ub_d_2",
         "err_ub_d_3", "err_ub_d_4", "acc_xna", "acc_pc", "specificity", "precision", "f1_score", "f2_score", "true_pos", "false_neg",
         "false_pos", "true_neg"]


def _paf_line(read_id, call, name, template, strand):
    """A full-length alignment without gaps of `call` (as it was made) to `template`, as `basecaller --paf` writes it."""
    from xna_basecaller_amd.aligner import Mapping
    q = bcdist_ref.query_letters(call, strand)
    assert len(q) == len(template)
    ops = "".join("=" if a == b.upper() and b.upper() in "ACGT" else "X" for a, b in zip(q, template))
    m = Mapping(name, template, call, strand, 0, 0, ops)
    return "\t".join(str(v) for v in (read_id, len(call), m.q_st, m.q_en, "+" if strand > 0 else "-", name, len(template), m.r_st,
                                      m.r_en, m.mlen, m.blen, 60, "cs:Z:" + m.cs)) + "\n", ops


def test_analyze_with_and_without_d(tmp_path):
    from xna_basecaller_amd import _lib, ubreport
    t0 = P5 + BC + P3
    t1 = P5 + BC[:5] + "T" + BC[6:12] + "A" + BC[13:20] + "C" + BC[21:] + P3    # its barcode three substitutions from t0's
    names, templates = ["T0", "T1"], [t0, t1]
    x0, x1 = t0.replace("N", "X"), t1.replace("N", "X")
    garbled = x0[:25] + "TTTTTTTTTTGGGGGGGGGGCCCC" + x0[49:]
    reads = {"rA": x0, "rB": garbled, "rC": _revcomp(x1), "rU": "ACGTACGTACGTTTGACA"}
    lib, paf, fq = tmp_path / "lib.fasta", tmp_path / "calls.paf", tmp_path / "calls.fastq"
    lib.write_text("".join(">%s\n%s\n" % (n, t) for n, t in zip(names, templates)))
    fq.write_text("".join("@%s\n%s\n+\n%s\n" % (k, s, "O" * len(s)) for k, s in reads.items()))
    table = [("rA", 1, 1), ("rA", 0, 1), ("rB", 0, 1), ("rC", 1, -1)]            # (read, template, strand): rA twice, T1 first
    lines = [_paf_line(r, reads[r], names[t], templates[t], s) for r, t, s in table]
    paf.write_text("".join(line for line, _ in lines))
    base = [sys.executable, "-m", "xna_basecaller_amd", "analyze", str(lib), str(paf), "-R", str(fq), "--save_perf_per_read", "-D",
            "--save_confusion_matrix"]
    prefix = str(tmp_path / "results_summ-calls")

    # without -d: what Report writes today for those rows -- the same bytes as a Report filled here, today's keys, a row per alignment
    r = subprocess.run(base, cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    rep = ubreport.Report(names, templates)
    ctx = _lib.mapper_context(0)
    ubreport.tally_paf(rep, ctx, ubreport.read_paf(str(paf)), ubreport.read_sequences(str(fq)))
    ctx.close()
    rep.write(str(tmp_path / "here"))
    suffixes = [".csv", "-by_tar.csv", "-by_read.csv.gz", "-confusion_matrix.npy"]
    for sfx in suffixes:
        assert open(prefix + sfx, "rb").read() == open(str(tmp_path / "here") + sfx, "rb").read(), sfx
    head, row = open(prefix + ".csv").read().strip().split("\n")
    assert head.split(",") == TODAY and row.split(",")[0] == "3"
    plain = gzip.open(prefix + "-by_read.csv.gz", "rt").read().strip().split("\n")
    assert len(plain) == 1 + 4 and plain[0].split(",")[-1] == "true_neg" and [l.split(",")[0] for l in plain[1:]] == ["rA", "rA", "rB", "rC"]
    for sfx in suffixes:
        os.remove(prefix + sfx)

    # with -d 5: rA keeps its alignment to T0 (0 against 3), rB is over the limit, rC stays, rU was never aligned
    r = subprocess.run(base + ["-d", "5"], cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    head, row = (l.split(",") for l in open(prefix + ".csv").read().strip().split("\n"))
    at = TODAY.index("specificity")
    assert head == TODAY[:at] + ["demux", "align"] + TODAY[at:]
    summ = dict(zip(head, row))
    assert float(summ["demux"]) == pytest.approx(50.0) and float(summ["align"]) == pytest.approx(75.0) and summ["num_aligned_reads"] == "2"
    by_read = [l.split(",") for l in gzip.open(prefix + "-by_read.csv.gz", "rt").read().strip().split("\n")]
    assert by_read[0][:-3] == plain[0].split(",") and by_read[0][-3:] == ["barcode_distance", "barcode_start", "barcode_end"]
    assert [(l[0], l[1], l[2]) for l in by_read[1:]] == [("rA", "T0", "F"), ("rC", "T1", "R")]
    assert [l[-3:] for l in by_read[1:]] == [["0", "25", "49"], ["0", "25", "49"]]
    # the tallies are those of the survivors alone
    keep = [1, 3]
    rows, lens = map_ref.pack_rows([reads[table[k][0]] for k in keep], 96)
    lmax = max(len(t) for t in templates)
    mapped = {"tmpl": np.array([table[k][1] for k in keep], np.int32), "strand": np.array([table[k][2] for k in keep], np.int8),
              "q_st": np.zeros(2, np.int32), "r_st": np.zeros(2, np.int32), "r_en": np.array([len(templates[table[k][1]]) for k in keep], np.int32),
              "n_ops": np.array([len(lines[k][1]) for k in keep], np.int32), "ops": np.zeros((2, 96 + lmax), np.uint8)}
    for j, k in enumerate(keep):
        mapped["ops"][j, :len(lines[k][1])] = np.frombuffer(lines[k][1].encode(), np.uint8)
    want_counts, want_acc = ubtally_ref.tally(rows, lens, mapped, templates)
    assert np.array_equal(np.load(prefix + "-confusion_matrix.npy"), want_acc["cm"])
    cols = by_read[0]
    for j in range(2):
        assert [int(by_read[1 + j][cols.index(c)]) for c in ubtally_ref.COUNTS] == want_counts[j].tolist()
    by_tar = [l.split(",") for l in open(prefix + "-by_tar.csv").read().strip().split("\n")[1:]]
    assert [(l[0], l[1], int(l[-1])) for l in by_tar] == [("T0", "F", 1), ("T1", "R", 1)] and want_acc["reads"].tolist() == [[1, 0], [0, 1]]
    for sfx in suffixes:
        os.remove(prefix + sfx)

    # nothing left after the filter (a window that holds the template's N, which no call spells, and no edit allowed): the
    # "no read left" line, no file
    r = subprocess.run(base + ["-d", "0", "--barcode-start", "45", "--barcode-relax", "0"], cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0 and b"no read left" in r.stderr, r.stderr.decode()
    assert not any(os.path.exists(prefix + sfx) for sfx in suffixes)
