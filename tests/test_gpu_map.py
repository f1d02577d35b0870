"""GPU: xb_map_templates through the C ABI against the CPU restatement of its contract (tests/map_ref.py): every output array
bit-equal.  minimap2 is in no image: parity unpinned, the contract is the header's."""
import os
import subprocess
import sys

import numpy as np
import pytest

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


def _check(ctx, reads, templates, scoring=map_ref.DEFAULT_SCORING, width=None):
    rows, lens = map_ref.pack_rows(reads, width)
    lib, off = _library(templates)
    got = ctx.map_templates(rows, lens, lib, off, scoring)
    want = map_ref.map_rows(rows, lens, templates, scoring)
    for k in KEYS:
        bad = np.flatnonzero((got[k] != want[k]).reshape(len(reads), -1).any(axis=1))
        assert bad.size == 0, (k, bad[:5], [(reads[b], got[k][b], want[k][b]) for b in bad[:2]])
    return got


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTXY", "TGCAYX"))


def _mutated_reads(templates, count, rng):
    """Seeded reads off the templates: substitutions, indels, the unnatural base (the template's N) called X / Y / a natural
    letter / dropped, both strands, random flanks; 5 % unrelated sequences, empty rows, rows of one base."""
    letters = np.array(list("ACGT"))
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
        reads.append(_revcomp(s) if rng.random() < 0.5 else s)
    return reads


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
