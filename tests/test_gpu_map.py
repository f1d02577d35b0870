"""GPU: xb_map_templates through the C ABI against the CPU restatement of its contract (tests/map_ref.py): every output array
bit-equal, and every mapped row of the device's output replayed column by column (map_cases.replay).  The second half takes the
kernels to their limits with the families of tests/map_cases.py -- stripe hand-off, score workgroup sizes, the LDS / scratch trace
boundary, the widest row against the longest templates, chunk packing, the scoring's range, odd bytes and lengths -- and the
library cache through a sequence of libraries and consumers.  minimap2 is in no image: parity unpinned, the contract is the
header's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import map_cases
import map_ref
from conftest import GOLDEN, ROOT, make_config

pytestmark = pytest.mark.gpu

POC = os.path.join(GOLDEN, "poc_refdb_short.fasta")
KEYS = ("tmpl", "strand", "score", "second", "q_st", "q_en", "r_st", "r_en", "n_ops", "ops")


def _ctx():
    from xna_basecaller_amd import _lib
    _lib.require_gpu()
    return _lib.Context(0, 6, 3, 64, 19, 5, 5.0, 2.0, 1000, 4)


def _library(templates):
    off = np.zeros(len(templates) + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in templates])
    return "".join(templates).encode("ascii"), off


def _plan(templates):
    """What the kernels make of the library's longest template: Lmax, columns per lane K, stripes of 64 K columns."""
    lmax = max(len(t) for t in templates)
    k = 1 if lmax <= 64 else (2 if lmax <= 128 else 4)
    return "Lmax %d, K %d, %d stripe(s)" % (lmax, k, -(-lmax // (64 * k)))


def _equal(got, want, case, lens):
    """Every output array bit-equal; the first differing rows printed with their length, the winner in both outputs and the
    kernels' plan for the library."""
    for k in KEYS:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        bad = np.flatnonzero((got[k] != want[k]).reshape(len(case.reads), -1).any(axis=1))
        if bad.size:
            rows = [dict(row=int(b), seq_len=int(lens[b]), read=case.reads[b][:80],
                         device={x: got[x][b].tolist() for x in KEYS[:9]}, restatement={x: want[x][b].tolist() for x in KEYS[:9]},
                         device_ops=got["ops"][b].tobytes().rstrip(b"\0")[:200], restatement_ops=want["ops"][b].tobytes().rstrip(b"\0")[:200])
                    for b in bad[:2]]
            raise AssertionError((k, bad[:5].tolist(), _plan(case.templates), "scoring %s" % (case.scoring,), rows))


def _check(ctx, reads, templates, scoring=map_ref.DEFAULT_SCORING, width=None, lens=None, want=None):
    """The host form on the device against the restatement (want: its outputs when they are at hand), bit-equal on all ten
    outputs; then every mapped row of the device's output on its own through map_cases.replay."""
    case = map_cases.Case(reads, templates, tuple(scoring), width, lens)
    rows, lens = map_cases.pack(case)
    lib, off = map_cases.library(templates)
    got = ctx.map_templates(rows, lens, lib, off, scoring)
    want = map_ref.map_rows(rows, lens, templates, scoring) if want is None else want
    _equal(got, want, case, lens)
    map_cases.replay_all(case, got)
    return got


def _dev_form(ctx, rows, lens, lib, off, scoring, like):
    """xb_map_templates_dev on device copies of the rows -> the ten outputs as numpy arrays (shapes and types of `like`)."""
    import torch
    n, W = rows.shape
    dev = torch.device("cuda:0")
    d_seq, d_len = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
    d_out = {k: torch.full(like[k].shape, 77, dtype=getattr(torch, str(like[k].dtype)), device=dev) for k in KEYS}
    torch.cuda.synchronize()
    ctx.map_templates_dev(d_seq.data_ptr(), d_len.data_ptr(), n, W, lib, off, scoring, {k: v.data_ptr() for k, v in d_out.items()})
    ctx.synchronize()
    return {k: v.cpu().numpy() for k, v in d_out.items()}


def _family(family, arg=None, dev_form=False):
    """Every case of a family of tests/map_cases.py on one context against the restatement's outputs for it."""
    ctx = _ctx()
    for case, want in zip(map_cases.cases(family, arg), map_cases.expected(family, arg)):
        got = _check(ctx, case.reads, case.templates, case.scoring, case.width, case.lens, want)
        if dev_form:
            rows, lens = map_cases.pack(case)
            lib, off = map_cases.library(case.templates)
            dev = _dev_form(ctx, rows, lens, lib, off, case.scoring, got)
            for k in KEYS:
                assert np.array_equal(dev[k], got[k]), k
    ctx.close()


_revcomp = map_cases.revcomp
_mutated_reads = map_cases.mutated_reads


def _poc():
    from xna_basecaller_amd.aligner import read_fasta
    return [s for _, s in read_fasta(POC)]


def test_poc_library_mutated_reads():
    ctx = _ctx()
    templates = _poc()
    assert len(templates) == 20 and min(len(t) for t in templates) == 106
    reads = _mutated_reads(templates, 600, np.random.default_rng(11))
    got = _check(ctx, reads, templates)
    assert (got["tmpl"] >= 0).sum() > 500 and (got["strand"] == -1).sum() > 200 and (got["strand"] == 1).sum() > 200
    assert (got["tmpl"] < 0).sum() >= 5
    ctx.close()


def test_large_short_library():
    """1024 templates of 89: six chunks of templates per read in the score pass."""
    ctx = _ctx()
    rng = np.random.default_rng(5)
    letters = np.array(list("ACGTN"))
    templates = ["".join(rng.choice(letters, 89, p=[0.245, 0.245, 0.245, 0.245, 0.02])) for _ in range(1024)]
    reads = _mutated_reads(templates, 256, rng)
    got = _check(ctx, reads, templates)
    assert len(set(got["tmpl"].tolist())) > 150
    ctx.close()


@pytest.mark.parametrize("length", [1, 63, 64, 65, 129, 1000])
def test_template_lengths(length):
    """One, two and four columns per lane, a stripe exactly full, one column into the next stripe, several stripes."""
    ctx = _ctx()
    rng = np.random.default_rng(length)
    letters = np.array(list("ACGT"))
    templates = ["".join(rng.choice(letters, length)) for _ in range(3)] + ["".join(rng.choice(letters, max(1, length // 2)))]
    reads = _mutated_reads(templates, 24, rng)
    reads += ["".join(rng.choice(letters, 3 * length + 7)), templates[0][:max(1, length // 3)], _revcomp(templates[1]), "A", ""]
    _check(ctx, reads, templates)
    ctx.close()


def test_all_ambiguous_and_unmapped():
    ctx = _ctx()
    got = _check(ctx, ["NNNNNNNN", "XYXYXY", "", "AAAA", "CCGGXCCGG"], ["CCCCGGGG", "CCGGNCCGG"])
    assert got["tmpl"].tolist() == [-1, -1, -1, -1, 1]
    ctx.close()


def test_engineered_ties():
    """Duplicate templates (lowest index wins, second = the winner's score), a palindromic template (+ before -), equal-score
    end cells (first in row-major order), and a gap that can sit in two places."""
    ctx = _ctx()
    t = "ACGGTCATTGCA"
    got = _check(ctx, [t, _revcomp(t)], ["TTTTTTTT", t, t])
    assert got["tmpl"].tolist() == [1, 1] and got["second"].tolist() == got["score"].tolist()
    pal = "ACGTTGCATGCAACGT"
    assert _revcomp(pal) == pal
    got = _check(ctx, [pal, "GG" + pal], [pal])
    assert got["strand"].tolist() == [1, 1]
    got = _check(ctx, ["ACGT", "TTACGTTT"], ["ACGTCCCCACGTCCCCACGT"])           # three equal end cells, the first is taken
    assert got["r_en"].tolist() == [4, 4]
    got = _check(ctx, ["ACGTAC"], ["GGGGACGTACGTACGGGG"])
    _check(ctx, ["ACGATCGATTTTTCGATCGAAGCT", "ACGATCGATTTCGATCGAAGCT"], ["ACGATCGATTTTCGATCGAAGCT"])   # homopolymer indel
    ctx.close()


def test_forms_batch_splits_and_scoring():
    """Host and _dev forms agree; two batch splits give the same bytes; a scoring other than the default stays bit-equal."""
    import torch
    ctx = _ctx()
    templates = _poc()
    reads = _mutated_reads(templates, 96, np.random.default_rng(3))
    whole = _check(ctx, reads, templates, scoring=(5, 4, 8, 4, 1))
    rows, lens = map_ref.pack_rows(reads)
    lib, off = _library(templates)
    parts = [ctx.map_templates(rows[a:b], lens[a:b], lib, off, (5, 4, 8, 4, 1)) for a, b in ((0, 7), (7, 64), (64, 96))]
    for k in KEYS:
        assert np.array_equal(np.concatenate([p[k] for p in parts]), whole[k]), k
    n, W = rows.shape
    dev = torch.device("cuda:0")
    d_seq, d_len = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
    d_out = {k: torch.zeros(whole[k].shape, dtype=getattr(torch, str(whole[k].dtype)), device=dev) for k in KEYS}
    torch.cuda.synchronize()
    ctx.map_templates_dev(d_seq.data_ptr(), d_len.data_ptr(), n, W, lib, off, (5, 4, 8, 4, 1), {k: v.data_ptr() for k, v in d_out.items()})
    ctx.synchronize()
    for k in KEYS:
        assert np.array_equal(d_out[k].cpu().numpy(), whole[k]), k
    ctx.close()


def test_over_budget_library_is_refused_and_the_context_survives():
    from xna_basecaller_amd import _lib
    ctx = _ctx()
    rng = np.random.default_rng(0)
    big = ["".join(rng.choice(np.array(list("ACGT")), 4096)) for _ in range(300)]          # 1.2 M letters
    rows, lens = map_ref.pack_rows(["ACGTACGT"])
    lib, off = _library(big)
    with pytest.raises(_lib.XbError) as e:
        ctx.map_templates(rows, lens, lib, off)
    assert e.value.code == _lib.XB_ERR_INVALID and "1228800 letters" in str(e.value)
    with pytest.raises(_lib.XbError) as e:                                                  # within the library bound, over the cells
        lib2, off2 = _library(big[:200])
        ctx.map_templates(np.zeros((4096, 4096), np.int8), np.zeros(4096, np.int32), lib2, off2)
    assert e.value.code == _lib.XB_ERR_INVALID and "cells" in str(e.value)
    _check(ctx, ["ACGTTGCA"], ["ACGTTGCA"])
    ctx.close()


def test_cli_reference_end_to_end(tmp_path):
    """`basecaller MODEL READS --reference poc_refdb_short.fasta --paf out.paf > out.sam` on synthetic reads (whatever the
    seeded model calls): every SAM record and PAF row is what map_ref and the host formatters give for the FASTQ of the same
    run without --reference; sequence, quality and tags are untouched by the flag; the summary has 27 columns."""
    from test_gpu_cli import _make_model_dir
    from xna_basecaller_amd import io as xio
    from xna_basecaller_amd import reads as xreads
    from xna_basecaller_amd.aligner import read_fasta
    model_dir, reads_dir = str(tmp_path / "xna_map@v1"), str(tmp_path / "reads")
    _make_model_dir(model_dir, 64, list("NACGTXY"), seed=21)
    rng = np.random.default_rng(4)
    recs = []
    for i in range(12):
        length = int(rng.integers(1500, 5000))
        raw = np.round(rng.normal(90.0, 12.0, length) * 8.0).astype(np.int16)
        recs.append((raw, dict(read_id="read-%02d" % i, range=1443.03, digitisation=8192.0, offset=10, sampling_rate=4000.0,
                               run_id="runX", channel_number=str(100 + i), start_mux=1 + i % 4, read_number=i,
                               start_time=4000 * i, duration=length, exp_start_time="2021-06-01T10:00:00Z")))
    os.makedirs(reads_dir)
    xreads.write_bundle(os.path.join(reads_dir, "batch0.xsig.npz"), recs)
    base = [sys.executable, "-m", "xna_basecaller_amd", "basecaller", model_dir, reads_dir, "--batch", "7"]
    fq, sam, paf = tmp_path / "calls.fastq", tmp_path / "out.sam", tmp_path / "out.paf"
    for target, extra in ((fq, []), (sam, ["--reference", POC, "--paf", str(paf)])):
        with open(target, "w") as fh:
            r = subprocess.run(base + extra, cwd=ROOT, stdout=fh, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()
    assert "> outputting aligned sam" in r.stderr.decode()
    lines = fq.read_text().strip().split("\n")
    heads, seqs, quals = lines[0::4], lines[1::4], lines[3::4]
    assert len(seqs) == 12 and all(0 < len(s) <= 4096 for s in seqs)
    names, templates = zip(*read_fasta(POC))
    text = sam.read_text().split("\n")
    header = [l for l in text if l.startswith("@")]
    body = [l for l in text if l and not l.startswith("@")]
    assert any(l.startswith("@PG\tID:aligner\tPN:xnacall-map\t") for l in header) and "minimap2" not in "".join(header)
    want_paf, mapped = [], 0
    assert len(body) == 12
    for head, seq, qual, line in zip(heads, seqs, quals, body):
        read_id, tags = head[1:].split(" ", 1)
        m = map_ref.to_mapping(map_ref.map_read(seq, templates), names, templates, seq)
        assert line == xio.sam_record(read_id, seq, qual, m, tags=tags.split("\t")), read_id
        f = line.split("\t")
        assert f[9] == (seq if m is None or m.strand == 1 else xio.revcomp(seq)) and f[10] == qual and f[13:] == tags.split("\t")
        if m is not None:
            mapped += 1
            out = []
            xio.write_paf(type("L", (), {"write": out.append})(), read_id, len(seq), m)
            want_paf += out
    assert mapped >= 6 and paf.read_text() == "".join(want_paf)
    summary = (tmp_path / "out_summary.tsv").read_bytes().decode().strip().split("\r\n")
    assert len(summary) == 13 and all(len(l.split("\t")) == 27 for l in summary)
    assert len((tmp_path / "calls_summary.tsv").read_bytes().decode().split("\r\n")[0].split("\t")) == 11


# ---- the mapper at its limits: the families of tests/map_cases.py, whose conditions tests/test_map_host.py holds on the
# restatement's outputs -------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("length", map_cases.STRIPE_LENGTHS)
def test_stripes(length):
    _family("stripes", length)


def test_mixed_lengths():
    _family("mixed_lengths")


@pytest.mark.parametrize("W", map_cases.WAVE_WIDTHS)
def test_wave_counts(W):
    _family("wave_counts", W, dev_form=W == 4096)


@pytest.mark.parametrize("W", map_cases.TRACE_WIDTHS)
def test_trace_boundary(W):
    _family("trace_boundary", W)


def test_full_size():
    _family("full_size", dev_form=True)


def test_chunking():
    _family("chunking")


def test_scorings():
    _family("scorings")


def test_letters_and_lengths():
    _family("letters_and_lengths")


def test_scoring_out_of_range_is_refused_and_the_context_survives():
    from xna_basecaller_amd import _lib
    ctx = _ctx()
    templates = _poc()
    reads = _mutated_reads(templates, 12, np.random.default_rng(29))
    case = map_cases.Case(reads, templates, map_ref.DEFAULT_SCORING, None)
    rows, lens = map_cases.pack(case)
    lib, off = map_cases.library(templates)
    want = map_ref.map_rows(rows, lens, templates)
    for at in range(5):
        for value in (-1, 1001):
            scoring = list(map_ref.DEFAULT_SCORING)
            scoring[at] = value
            with pytest.raises(_lib.XbError) as e:
                ctx.map_templates(rows, lens, lib, off, scoring)
            assert e.value.code == _lib.XB_ERR_INVALID and "[0, 1000]" in str(e.value), (at, value)
            _check(ctx, reads, templates, want=want)
    for at in range(5):                                    # the ends of the range are inside it
        scoring = list(map_ref.DEFAULT_SCORING)
        scoring[at] = 1000
        _check(ctx, reads[:4], templates, scoring)
    ctx.close()


def test_library_cache_follows_letters_offsets_and_the_consumers():
    """One context: POC; POC with one letter changed at equal offsets; the same letters with one boundary moved; POC again.
    Then xb_ctc_targets, xb_ub_tally and xb_barcode_dist, which share the library image, each put another library in its place
    between two mapper calls on POC.  The restatement keeps no image: a stale one shows as a mismatch."""
    import bcdist_ref
    import savectc_ref
    import ubtally_ref
    ctx = _ctx()
    poc = _poc()
    rng = np.random.default_rng(41)
    reads = [map_cases.mutate(rng, poc[7], keep=6), poc[3], poc[4], map_cases.revcomp(poc[4])] + _mutated_reads(poc, 20, rng)
    case = map_cases.Case(reads, poc, map_ref.DEFAULT_SCORING, None)
    rows, lens = map_cases.pack(case)
    W = rows.shape[1]
    want1 = map_ref.map_rows(rows, lens, poc)
    _check(ctx, reads, poc, want=want1)
    # one letter of the template that wins read 0, under an '=' column of its alignment
    t0, r_st = int(want1["tmpl"][0]), int(want1["r_st"][0])
    ops0 = want1["ops"][0][:want1["n_ops"][0]].tobytes().decode()
    run = max(ops0.replace("I", "X").replace("D", "X").split("X"), key=len)
    col = ops0.index(run) + len(run) // 2                   # the middle of the longest run of '='
    pos = r_st + sum(ops0[k] in "=XD" for k in range(col))
    assert t0 == 7 and want1["strand"][0] == 1
    letters2 = list(poc[t0])
    letters2[pos] = "A" if letters2[pos] != "A" else "C"
    lib2 = poc[:t0] + ["".join(letters2)] + poc[t0 + 1:]
    assert [len(t) for t in lib2] == [len(t) for t in poc]
    want2 = map_ref.map_rows(rows, lens, lib2)
    assert want2["score"][0] < want1["score"][0]
    got2 = _check(ctx, reads, lib2, want=want2)
    # the same letters, the boundary between templates 3 and 4 one letter on
    lib3 = lib2[:3] + [lib2[3] + lib2[4][:1], lib2[4][1:]] + lib2[5:]
    assert "".join(lib3) == "".join(lib2)
    want3 = map_ref.map_rows(rows, lens, lib3)
    assert want3["score"][2] == want2["score"][2] - 2 and want3["score"][3] == want2["score"][3] - 2
    _check(ctx, reads, lib3, want=want3)
    _check(ctx, reads, poc, want=want1)
    # the consumers on the library of step 2 with the mapper's outputs for it, the mapper on POC behind each
    lib, off = map_cases.library(lib2)
    rule = dict(min_accuracy=0.8, min_coverage=0.5)
    got = ctx.ctc_targets(lens, W, got2, lib, off, **rule)
    want = savectc_ref.targets(lens, W, got2, lib2, **rule)
    for k in ("mlen", "blen", "verdict", "target", "target_len"):
        assert np.array_equal(got[k], want[k]), k
    assert not np.array_equal(want["target"], savectc_ref.targets(lens, W, got2, poc, **rule)["target"])      # the two libraries differ here
    _check(ctx, reads, poc, want=want1)
    counts, acc = ctx.ub_tally(rows, lens, got2, lib, off)
    want_counts, want_acc = ubtally_ref.tally(rows, lens, got2, lib2)
    assert np.array_equal(counts, want_counts)
    for k in ("reads", "err", "cm"):
        assert np.array_equal(getattr(acc, k), want_acc[k]), k
    assert not np.array_equal(want_acc["err"], ubtally_ref.tally(rows, lens, got2, poc)[1]["err"])
    _check(ctx, reads, poc, want=want1)
    bc = (pos - 8, 20, 3)
    out = ctx.barcode_dist(rows, lens, got2, lib, off, *bc)
    want = bcdist_ref.dist(rows, lens, got2, lib2, *bc)
    for k in bcdist_ref.OUTPUTS:
        assert np.array_equal(out[k], want[k]), k
    assert any(not np.array_equal(want[k], bcdist_ref.dist(rows, lens, got2, poc, *bc)[k]) for k in bcdist_ref.OUTPUTS)
    _check(ctx, reads, poc, want=want1)
    ctx.close()
