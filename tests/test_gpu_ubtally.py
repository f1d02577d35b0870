"""GPU: xb_ub_tally through the C ABI against the CPU restatement of its contract (tests/ubtally_ref.py): counts, reads, err and
cm equal, integer for integer.  The mapper's outputs come from xb_map_templates itself on seeded calls, or are built by hand
where a polish branch or a clamp has to be hit.  minimap2 is in no image: parity unpinned, the contract is the header's."""
import gzip
import os
import subprocess
import sys

import numpy as np
import pytest

import map_ref
import ubtally_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu

LETTERS = np.array(list("ACGT"))


def _ctx():
    from xna_basecaller_amd import _lib
    _lib.require_gpu()
    return _lib.Context(0, 6, 3, 64, 19, 5, 5.0, 2.0, 1000, 4)


def _library(templates):
    off = np.zeros(len(templates) + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in templates])
    return "".join(templates).encode("ascii"), off


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTXY", "TGCAYX"))


def _equal(counts, acc, want_counts, want_acc):
    bad = np.flatnonzero((counts != want_counts).any(axis=1))
    assert bad.size == 0, (bad[:5], counts[bad[:3]], want_counts[bad[:3]])
    assert np.array_equal(acc.reads, want_acc["reads"]), (acc.reads, want_acc["reads"])
    assert np.array_equal(acc.err, want_acc["err"]), np.flatnonzero((acc.err != want_acc["err"]).ravel())[:8]
    assert np.array_equal(acc.cm, want_acc["cm"]), (acc.cm, want_acc["cm"])


def _check(ctx, rows, lens, got, templates):
    lib, off = _library(templates)
    counts, acc = ctx.ub_tally(rows, lens, got, lib, off)
    want_counts, want_acc = ubtally_ref.tally(rows, lens, got, templates)
    assert acc.cm.dtype == np.int64 and counts.dtype == np.int32
    _equal(counts, acc, want_counts, want_acc)
    return counts, acc


def _template(rng, length, ubs):
    t = list(rng.choice(LETTERS, length))
    for u in ubs:
        t[u] = "N"
    return "".join(t)


def _family(rng, L):
    """Templates of L letters: a UB at 0, at L-1, within 5 of each end, two adjacent, none."""
    sets = [[0], [L - 1], sorted({min(3, L - 1), max(L - 4, 0)}), sorted({L // 2, min(L // 2 + 1, L - 1)}), []]
    return [_template(rng, L, u) for u in sets]


def _calls(templates, count, rng, each=False):
    """Seeded calls off the templates: substitutions, insertions, deletions; the UB called X, Y, a natural letter, dropped, or
    X moved one letter to either side; both strands; empty rows and unrelated rows mixed in.  each: call k comes off template
    k % len(templates), and no empty or unrelated rows take a place."""
    reads = []
    for k in range(count):
        u = rng.random()
        if u < 0.04 and not each:
            reads.append("")
            continue
        if u < 0.08 and not each:
            reads.append("".join(rng.choice(LETTERS, rng.integers(1, 30))))
            continue
        tpl = templates[k % len(templates) if each else rng.integers(len(templates))]
        out = []
        for c in tpl:
            if c == "N":
                c = str(rng.choice(["X", "Y", "A", "", "AX", "XA", "XX"], p=[0.4, 0.1, 0.1, 0.1, 0.1, 0.1, 0.1]))
            v = rng.random()
            if v < 0.04:
                c = str(rng.choice(LETTERS))
            elif v < 0.08:
                c = ""
            elif v < 0.11:
                c = c + "".join(rng.choice(LETTERS, rng.integers(1, 3)))
            out.append(c)
        s = "".join(out)
        if rng.random() < 0.3 and len(s) > 8:
            s = s[rng.integers(0, 4):len(s) - rng.integers(0, 4)]
        reads.append(_revcomp(s) if rng.random() < 0.5 else s)
    return reads


def _mapped(ctx, reads, templates, width=None):
    rows, lens = map_ref.pack_rows(reads, width)
    lib, off = _library(templates)
    return rows, lens, ctx.map_templates(rows, lens, lib, off)


@pytest.mark.parametrize("length,n", [(1, 65), (11, 65), (63, 65), (64, 65), (65, 65), (100, 65), (4096, 5)])
def test_template_lengths_and_ub_places(length, n):
    ctx = _ctx()
    rng = np.random.default_rng(length)
    templates = _family(rng, length) if length > 1 else ["A", "C", "N", "G", "T"]
    reads = [r[:4096] for r in _calls(templates, n, rng, each=length == 4096)]
    rows, lens, got = _mapped(ctx, reads, templates, width=4096 if length == 4096 else None)
    assert (got["tmpl"] >= 0).any()
    if length == 4096:                  # at the LDS limit every placement of the family is tallied: one call per template
        assert sorted(got["tmpl"].tolist()) == list(range(len(templates)))
    _check(ctx, rows, lens, got, templates)
    ctx.close()


def test_width_16_one_row():
    ctx = _ctx()
    templates = ["ACGTANGTCAG", "TTGACNNCATG"]
    for reads in (["ACGTAXGTCAG"], [_revcomp("TTGACXXCATG")]):
        rows, lens, got = _mapped(ctx, reads, templates, width=16)
        assert rows.shape == (1, 16) and got["tmpl"][0] >= 0
        counts, _ = _check(ctx, rows, lens, got, templates)
        assert counts[0, 0] == 11 and counts[0, 1] == counts[0, 2]          # every letter right, every UB called
    ctx.close()


def test_contended_atomics_300_rows_two_templates():
    ctx = _ctx()
    rng = np.random.default_rng(300)
    templates = [_template(rng, 100, [30, 31, 70]), _template(rng, 100, [50])]
    reads = _calls(templates, 300, rng)
    rows, lens, got = _mapped(ctx, reads, templates)
    counts, acc = _check(ctx, rows, lens, got, templates)
    assert acc.reads.sum() == (got["tmpl"] >= 0).sum() > 250 and (acc.reads > 20).all()
    assert (got["tmpl"] < 0).sum() >= 5 and not counts[got["tmpl"] < 0].any()
    ctx.close()


# ---- rows built by hand: ops fed directly ------------------------------------------------------------------------------
HAND_TEMPLATES = ["ACGTANACGTAC", "".join("ACGT"[(k * 7 + k // 5) % 4] for k in range(100)) + "N" + "".join("ACGT"[(k * 3) % 4] for k in range(99)),
                  "ACGT", "N"]
HAND_W = 32


def _hand(cases):
    """cases: [dict(seq, tmpl, strand, q_st, r_st, r_en, ops[, seq_len, n_ops])] -> rows, lens, got."""
    lmax = max(len(t) for t in HAND_TEMPLATES)
    n = len(cases)
    rows = np.zeros((n, HAND_W), np.int8)
    lens = np.zeros(n, np.int32)
    got = {k: np.zeros(n, np.int32) for k in ("tmpl", "score", "second", "q_st", "q_en", "r_st", "r_en", "n_ops")}
    got["strand"] = np.zeros(n, np.int8)
    got["ops"] = np.zeros((n, HAND_W + lmax), np.uint8)
    for k, c in enumerate(cases):
        seq = c["seq"].encode("latin-1")
        rows[k, :len(seq)] = np.frombuffer(seq, np.int8)
        lens[k] = c.get("seq_len", len(seq))
        ops = c["ops"].encode("latin-1")
        got["ops"][k, :len(ops)] = np.frombuffer(ops, np.uint8)
        got["n_ops"][k] = c.get("n_ops", len(ops))
        for f in ("tmpl", "strand", "q_st", "r_st", "r_en"):
            got[f][k] = c[f]
        got["q_en"][k] = len(seq)
    return rows, lens, got


def _row(seq, ops, tmpl=0, strand=1, q_st=0, r_st=0, r_en=None, **more):
    return dict(seq=seq, ops=ops, tmpl=tmpl, strand=strand, q_st=q_st, r_st=r_st,
                r_en=len(HAND_TEMPLATES[tmpl]) if r_en is None else r_en, **more)


POLISH = {
    "a": ("ACGTAXACGTAC", "=====X======"),
    "b_left": ("ACGTXACGTAC", "====XD======"),
    "b_right": ("ACGTAXCGTAC", "=====DX====="),
    "c": ("ACGTGXCGTAC", "====DXX====="),
    "d": ("ACGTXGCGTAC", "====XXD====="),
    "untouched": ("ACGTAGACGTAC", "=====X======"),
}


def test_hand_built_polish_branches_both_strands():
    ctx = _ctx()
    cases = []
    for seq, ops in POLISH.values():
        cases.append(_row(seq, ops))
        cases.append(_row(_revcomp(seq), ops, strand=-1))
    rows, lens, got = _hand(cases)
    counts, acc = _check(ctx, rows, lens, got, HAND_TEMPLATES)
    # what each branch must come to on this template (L = 12, the UB at 5): (n_match, ub_matches, ubs_detected)
    want = {"a": (12, 1, 1), "b_left": (11, 1, 1), "b_right": (11, 1, 1), "c": (10, 1, 1), "d": (10, 1, 1), "untouched": (11, 0, 0)}
    for k, name in enumerate(POLISH):
        for s in (0, 1):
            assert (counts[2 * k + s, 0], counts[2 * k + s, 1], counts[2 * k + s, 7]) == want[name], (name, s, counts[2 * k + s])
    assert acc.reads[0].tolist() == [6, 6] and acc.cm[4, 4] == 5 and acc.cm[5, 5] == 5      # X row on +, Y row on -
    ctx.close()


def test_hand_built_long_gap_runs_and_clamps():
    ctx = _ctx()
    long_t = 1
    cases = [
        # a '-' run of 79 (more than one step of 64) to the left of the UB at 100, an X before it: branch (b) left
        _row("X", "X", tmpl=long_t, r_st=20, r_en=21),
        # ... and of 60 and 99 to the right, an X behind it: branch (b) right
        _row("X", "X", tmpl=long_t, r_st=161, r_en=162),
        _row("X", "X", tmpl=long_t, r_st=199, r_en=200),
        # nothing called at all, no letters in the row
        _row("", "", tmpl=long_t, r_st=0, r_en=0),
        _row("", "", tmpl=3, r_st=0, r_en=0),
        # clamps: seq_len beyond the width and below zero, n_ops beyond the row and below zero
        _row("ACGTAXACGTAC", "=====X======", seq_len=4000),
        _row("ACGTAXACGTAC", "=====X======", seq_len=-3),
        _row("ACGTAXACGTAC", "=====X======", n_ops=100000),
        _row("ACGTAXACGTAC", "=====X======", n_ops=-1),
        # r_st below zero, r_en beyond the template, r_en before r_st, q_st outside the row
        _row("ACGTAXACGTAC", "=====X======", r_st=-4),
        _row("ACGTAXACGTAC", "=====X======", r_en=4000),
        _row("ACGTAXACGTAC", "=====X======", r_st=6, r_en=2),
        _row("ACGTAXACGTAC", "=====X======", q_st=-2),
        _row("ACGTAXACGTAC", "=====X======", q_st=40),
        _row("GGACGTAXACGTAC", "=====X======", q_st=2),
        # the walk ends: the row runs out, the template range runs out, an unknown column byte
        _row("ACGTAX", "=====X======"),
        _row("ACGTAXACGTAC", "=====X======", r_en=7),
        _row("ACGTAXACGTAC", "=====X==?==="),
        _row("ACG", "===III======"),
        _row("ACGTAXACGTAC", "===DDDDDDDDDDDD==="),
        # unmapped rows: tmpl -1, R, far outside; strand 0 counts as +
        _row("ACGTAXACGTAC", "=====X======", tmpl=-1, r_en=12),
        _row("ACGTAXACGTAC", "=====X======", tmpl=len(HAND_TEMPLATES), r_en=12),
        _row("ACGTAXACGTAC", "=====X======", tmpl=-70000, r_en=12),
        _row("ACGTAXACGTAC", "=====X======", strand=0),
        # lower case, a called N, a byte outside ASCII; a template without a UB; a one-letter template that is a UB
        _row("acgtaxacgtac", "=====X======"),
        _row("acgtayacgtac"[::-1].translate(str.maketrans("acgt", "tgca")), "=====X======", strand=-1),
        _row("ACGTANAC\xe9TAC", "=====X======"),
        _row("ACGT", "====", tmpl=2),
        _row("AXGT", "=X==", tmpl=2),
        _row("X", "X", tmpl=3),
        _row("Y", "X", tmpl=3, strand=-1),
        _row("A", "X", tmpl=3),
    ]
    rows, lens, got = _hand(cases)
    counts, acc = _check(ctx, rows, lens, got, HAND_TEMPLATES)
    assert counts[0, 1] == counts[1, 1] == counts[2, 1] == 1 and counts[0, 0] == 1       # the X found its UB, nothing else is right
    assert not counts[20:23].any() and counts[23, 0] == 12
    assert counts[29].tolist() == [1, 1, 1, 0, 0, 0, 0, 1] and counts[30].tolist() == counts[29].tolist()
    ctx.close()


def test_two_calls_accumulate_like_one():
    ctx = _ctx()
    rng = np.random.default_rng(77)
    templates = _family(rng, 63)
    reads = _calls(templates, 90, rng)
    rows, lens, got = _mapped(ctx, reads, templates)
    lib, off = _library(templates)
    counts, acc = ctx.ub_tally(rows, lens, got, lib, off)
    first = {k: v[:40] for k, v in got.items()}
    second = {k: v[40:] for k, v in got.items()}
    c1, part = ctx.ub_tally(rows[:40], lens[:40], first, lib, off)
    reads_after_one = part.reads.copy()
    c2, part = ctx.ub_tally(rows[40:], lens[40:], second, lib, off, part)
    assert reads_after_one.sum() < part.reads.sum()
    _equal(np.concatenate([c1, c2]), part, counts, {"reads": acc.reads, "err": acc.err, "cm": acc.cm})
    want_counts, want_acc = ubtally_ref.tally(rows, lens, got, templates)
    _equal(counts, acc, want_counts, want_acc)
    ctx.close()


def test_dev_form_equals_host_form():
    import torch
    ctx = _ctx()
    rng = np.random.default_rng(5)
    templates = _family(rng, 100)
    reads = _calls(templates, 65, rng)
    rows, lens, got = _mapped(ctx, reads, templates)
    lib, off = _library(templates)
    counts, acc = ctx.ub_tally(rows, lens, got, lib, off)
    dev = torch.device("cuda:0")
    d_rows, d_lens = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
    d_got = {k: torch.from_numpy(got[k]).to(dev) for k in ctx.UB_INPUTS}
    d_counts = torch.full(counts.shape, 77, dtype=torch.int32, device=dev)
    d_reads = torch.zeros(acc.reads.shape, dtype=torch.int32, device=dev)
    d_err = torch.zeros(acc.err.shape, dtype=torch.int32, device=dev)
    d_cm = torch.zeros(acc.cm.shape, dtype=torch.int64, device=dev)
    torch.cuda.synchronize()
    ctx.ub_tally_dev(d_rows.data_ptr(), d_lens.data_ptr(), len(reads), rows.shape[1], {k: t.data_ptr() for k, t in d_got.items()},
                     lib, off, d_counts.data_ptr(), d_reads.data_ptr(), d_err.data_ptr(), d_cm.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_counts.cpu().numpy(), counts)
    assert np.array_equal(d_reads.cpu().numpy(), acc.reads) and np.array_equal(d_err.cpu().numpy(), acc.err)
    assert np.array_equal(d_cm.cpu().numpy(), acc.cm)
    ctx.close()


def test_template_of_4097_letters_is_refused_and_the_context_survives():
    from xna_basecaller_amd import _lib
    ctx = _ctx()
    templates = ["ACGTANACGTAC", "A" * 4097]
    rows, lens, got = _hand([_row("ACGTAXACGTAC", "=====X======")])
    lmax = 4097
    got["ops"] = np.zeros((1, HAND_W + lmax), np.uint8)
    got["ops"][0, :12] = np.frombuffer(b"=====X======", np.uint8)
    lib, off = _library(templates)
    with pytest.raises(_lib.XbError) as e:
        ctx.ub_tally(rows, lens, got, lib, off)
    assert e.value.code == _lib.XB_ERR_INVALID and "4097" in str(e.value) and "xb_ub_tally" in str(e.value)
    # the _dev form refuses the same library before it touches a pointer, and names itself
    import torch
    d = torch.zeros(64, dtype=torch.int64, device="cuda:0")
    for bad in (dict(n=1, width=HAND_W, off=off), dict(n=0, width=HAND_W, off=_library(HAND_TEMPLATES)[1]),
                dict(n=1, width=4097, off=_library(HAND_TEMPLATES)[1])):
        with pytest.raises(_lib.XbError) as e:
            ctx.ub_tally_dev(d.data_ptr(), d.data_ptr(), bad["n"], bad["width"], {k: d.data_ptr() for k in ctx.UB_INPUTS},
                             lib if bad["off"] is off else _library(HAND_TEMPLATES)[0], bad["off"], d.data_ptr(), d.data_ptr(),
                             d.data_ptr(), d.data_ptr())
        assert e.value.code == _lib.XB_ERR_INVALID and "xb_ub_tally" in str(e.value) and "xb_map_templates" not in str(e.value)
    rows, lens, got = _hand([_row("ACGTAXACGTAC", "=====X======")])
    counts, _ = _check(ctx, rows, lens, got, HAND_TEMPLATES)
    assert counts[0].tolist() == [12, 1, 1, 10, 10, 1, 1, 1]
    ctx.close()


# ---- the command line: --ub-report, and analyze over the same run's PAF and FASTQ -------------------------------------------
def test_cli_ub_report_and_analyze_agree(tmp_path):
    from test_gpu_cli import _make_model_dir, _make_reads
    model_dir = str(tmp_path / "xna_test@v1")
    reads_dir = str(tmp_path / "reads")
    _make_model_dir(model_dir, 64, list("NACGTXY"), seed=21)
    _make_reads(reads_dir, 6)
    # a library the seeded model's calls map to: pieces of a first run's calls, with a UB site put in
    first = tmp_path / "first.fastq"
    with open(first, "w") as fh:
        r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "basecaller", model_dir, reads_dir, "--batch", "7"], cwd=ROOT,
                           stdout=fh, stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    calls = first.read_text().strip().split("\n")[1::4]
    lib = tmp_path / "lib.fasta"
    with open(lib, "w") as fh:
        for k, s in enumerate(calls[:4]):
            piece = s[10:130]
            piece = piece if k == 3 else piece[:60] + "N" + piece[61:]
            fh.write(">T%d\n%s\n" % (k, piece if k % 2 == 0 else _revcomp(piece).replace("X", "N").replace("Y", "N")))
    out, paf, prefix = tmp_path / "calls.fastq", tmp_path / "calls.paf", str(tmp_path / "rep")
    with open(out, "w") as fh:
        r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "basecaller", model_dir, reads_dir, "--batch", "7",
                            "--reference", str(lib), "--paf", str(paf), "--ub-report", prefix], cwd=ROOT, stdout=fh,
                           stderr=subprocess.PIPE, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    names = [".csv", "-by_tar.csv", "-by_read.csv.gz", "-confusion_matrix.npy"]
    for n in names:
        assert os.path.getsize(prefix + n) > 0, n
    head, row = open(prefix + ".csv").read().strip().split("\n")
    assert head.split(",")[0] == "num_aligned_reads" and int(row.split(",")[0]) >= 4
    cm = np.load(prefix + "-confusion_matrix.npy")
    assert cm.shape == (6, 7) and cm.dtype == np.int64 and cm.sum() > 400
    assert gzip.open(prefix + "-by_read.csv.gz", "rt").read().count("\n") == int(row.split(",")[0]) + 1
    r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "analyze", str(lib), str(paf), "-R", str(out), "-D",
                        "--save_perf_per_read", "--save_confusion_matrix"], cwd=ROOT, capture_output=True, timeout=600)
    assert r.returncode == 0, r.stderr.decode()
    again = str(tmp_path / "results_summ-calls")
    for n in names:
        assert open(again + n, "rb").read() == open(prefix + n, "rb").read(), n
