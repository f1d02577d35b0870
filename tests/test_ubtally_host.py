"""CPU: the UB report's host side.  tests/ubtally_ref.py (the restatement of xb_ub_tally's contract) against what the
reference's own functions returned (tests/golden/ubtally.json, made by tests/golden/make_ubtally_golden.py); the cs string
round trip; ubreport's figures on a case computed by hand; the refusals of `analyze` and `--ub-report`."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import ubtally_ref
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "ubtally.json")) as fh:
        return json.load(fh)


def test_fixture_covers_what_it_must(golden):
    cases = golden["cases"]
    assert {c["strand"] for c in cases} == {"+", "-"}
    assert any(c["ub_len"] == 0 for c in cases) and any(c["ub_len"] == 2 and c["ub_area_len"] < 20 for c in cases)
    assert any(c["target_start"] > 0 and c["target_end"] < c["target_length"] for c in cases)
    branches = set()
    for c in cases:
        T = ubtally_ref.target_letters(golden["templates"][c["target_id"]])
        q = ubtally_ref.query_letters(c["call"], 1 if c["strand"] == "+" else -1)
        C = ubtally_ref.called_letters(len(T), q, c["q_st_aligned"], c["target_start"], c["target_end"], c["ops"].encode())
        for u in (j for j, t in enumerate(T) if t == "X"):
            assert 6 <= u < len(T) - 6
            if C[u] == "X":
                branches.add("a")
            elif C[u] == "-":
                branches.add("b")
            elif C[u - 1] == "-" and C[u + 1] == "X":
                branches.add("c")
            elif C[u + 1] == "-" and C[u - 1] == "X":
                branches.add("d")
    assert branches == {"a", "b", "c", "d"}


def test_restatement_equals_the_reference(golden):
    templates = golden["templates"]
    for c in golden["cases"]:
        strand = 1 if c["strand"] == "+" else -1
        counts, e, T, P = ubtally_ref.row(templates[c["target_id"]], c["call"], strand, c["q_st_aligned"], c["target_start"],
                                          c["target_end"], c["ops"].encode())
        name = c["read_id"]
        assert "".join(P) == c["polished"], name
        assert (e[::-1] if strand < 0 else e) == c["errors"], name
        got = dict(zip(ubtally_ref.COUNTS, counts))
        assert got["n_match"] == c["n_matches"], name
        for k in ("ub_matches", "ub_len", "ub_area_matches", "ub_area_len", "non_ub_area_matches", "non_ub_area_len", "ubs_detected"):
            assert got[k] == c[k], (name, k)
        if c["confusion"] is not None:
            assert ubtally_ref.confusion(T, P, strand).tolist() == c["confusion"], name


def test_report_figures_equal_the_reference(golden):
    """ubreport's per-read metrics and error-rate vectors from the restatement's integers against the reference's floats."""
    from xna_basecaller_amd import ubreport
    names, templates = list(golden["templates"]), list(golden["templates"].values())
    n = len(golden["cases"])
    rows = np.zeros((n, 64), np.int8)
    lens = np.zeros(n, np.int32)
    mapped = {k: np.zeros(n, np.int32) for k in ("tmpl", "q_st", "r_st", "r_en", "n_ops")}
    mapped["strand"] = np.zeros(n, np.int8)
    mapped["ops"] = np.zeros((n, 64 + max(len(t) for t in templates)), np.uint8)
    for k, c in enumerate(golden["cases"]):
        call = c["call"].encode()
        rows[k, :len(call)] = np.frombuffer(call, np.int8)
        lens[k] = len(call)
        mapped["tmpl"][k], mapped["strand"][k] = c["tmpl"], 1 if c["strand"] == "+" else -1
        mapped["q_st"][k], mapped["r_st"][k], mapped["r_en"][k] = c["q_st_aligned"], c["target_start"], c["target_end"]
        mapped["ops"][k, :len(c["ops"])] = np.frombuffer(c["ops"].encode(), np.uint8)
        mapped["n_ops"][k] = len(c["ops"])
    counts, acc = ubtally_ref.tally(rows, lens, mapped, templates)
    ral = [c["read_end"] - c["read_start"] for c in golden["cases"]]
    m = ubreport.per_read_metrics(counts, ral, [c["target_length"] for c in golden["cases"]])
    for k, c in enumerate(golden["cases"]):
        for key in ("ub_acc", "ub_area_acc", "ub_area_acc_plus", "non_ub_area_acc", "fdr", "fpr"):
            if c[key] is None:
                assert np.isnan(m[key][k]), (c["read_id"], key)
            else:
                assert m[key][k] == c[key], (c["read_id"], key)            # one float64 division of the same integers
        for key in ("true_pos", "false_neg", "false_pos", "true_neg"):
            assert m[key][k] == c[key], (c["read_id"], key)
    off = np.concatenate([[0], np.cumsum([len(t) for t in templates])])
    box = types.SimpleNamespace(**acc)
    for r in golden["error_rates"]:
        vec = ubreport.error_rate(box, off, names.index(r["target_id"]), 0 if r["strand"] == "+" else 1)
        assert np.allclose(vec, r["error_rate"], rtol=0, atol=1e-12), (r["target_id"], r["strand"])      # a mean against a quotient


def test_cs_round_trip(golden):
    from xna_basecaller_amd import ubreport
    from xna_basecaller_amd.aligner import Mapping
    names, templates = list(golden["templates"]), golden["templates"]
    for c in golden["cases"]:
        ops = ubreport.cs_to_ops(c["cs"])
        assert ops == c["ops"], c["read_id"]
        m = Mapping(c["target_id"], templates[c["target_id"]], c["call"], 1 if c["strand"] == "+" else -1, c["target_start"],
                    c["q_st_aligned"], ops)
        assert m.cs == c["cs"] and (m.q_st, m.q_en, m.r_en) == (c["read_start"], c["read_end"], c["target_end"])
    assert ubreport.cs_to_ops("=ACG*ag+tt-c:2") == "===XIID=="
    for bad in ("~ac12gt", ":", "*a", "?3", "+"):
        with pytest.raises(ValueError):
            ubreport.cs_to_ops(bad)


def test_paf_and_reads_parsers(tmp_path):
    from xna_basecaller_amd import ubreport
    paf = tmp_path / "x.paf"
    paf.write_text("r1\t12\t0\t12\t-\tT1\t12\t0\t12\t11\t12\t60\ttp:A:P\ts1:i:20\tcs:Z:=ACGTA*nn:6\n")
    a = ubreport.read_paf(str(paf))
    assert a == [dict(read_id="r1", read_length=12, q_st=0, q_en=12, strand=-1, target_id="T1", r_st=0, r_en=12, ops="=====X======")]
    paf.write_text("r1\t12\t0\t12\t-\tT1\t12\t0\t12\t11\t12\t60\ttp:A:P\n")
    with pytest.raises(ValueError):
        ubreport.read_paf(str(paf))
    paf.write_text("r1\t12\t0\t12\t-\tT1\t12\t0\n")                      # a truncated line is an error, not a smaller report
    with pytest.raises(ValueError):
        ubreport.read_paf(str(paf))
    fq = tmp_path / "x.fastq"
    fq.write_text("@r1 tag\nACGT\n+\n@@@@\n@r2\nXY\n+\nOO\n")
    assert ubreport.read_sequences(str(fq)) == {"r1": "ACGT", "r2": "XY"}
    fa = tmp_path / "x.fasta"
    fa.write_text(">r1 d\nAC\nGT\n>r2\nXY\n")
    assert ubreport.read_sequences(str(fa)) == {"r1": "ACGT", "r2": "XY"}


def test_summary_of_three_reads_by_hand():
    """Template T = ACGTACNACGTAC (L = 13, the UB at 6, its area 1 .. 11 without 6) and a plain one P = ACGT.  Three reads:
         r1  +  T  everything right                          n_match 13, ub 1 / 1, area 10 / 10, outside 2 / 2, detected 1
         r2  -  T  the UB called A, one more X at (forward) position 0: 11 right, ub 0 / 1, area 10 / 10, outside 1 / 2, detected 1
         r3  +  P  everything right                          n_match 4, no UB
       so   target_acc = mean(13 / 13, 11 / 13) * 100, fpr = (0, 1 / 12, 0), fdr = (0, 1, nan), tp 1, fn 1, fp 1, tn 12 + 11 + 4,
       the error-rate vectors: T + all zero; T - (reversed) 100 at positions 6 and 12; F1 = 2 / (2 + 1 + 1), F2 = 5 p r / (4 p + r),
       p = r = 1 / 2."""
    from xna_basecaller_amd import ubreport
    rep = ubreport.Report(["T", "P"], ["ACGTACNACGTAC", "ACGT"])
    counts = np.array([[13, 1, 1, 10, 10, 2, 2, 1], [11, 0, 1, 10, 10, 1, 2, 1], [4, 0, 0, 0, 0, 4, 4, 0]], np.int32)
    rep.read_ids, rep.tmpl, rep.strand, rep.counts = ["r1", "r2", "r3"], [0, 0, 1], [0, 1, 0], list(counts)
    rep.ral, rep.mlen, rep.blen = [13, 13, 4], [12, 11, 4], [13, 13, 4]
    rep.acc.reads[:] = [[1, 1], [1, 0]]
    rep.acc.err[1, 6] = rep.acc.err[1, 12] = 1
    s = rep.summary()
    assert s["num_aligned_reads"] == 3
    assert s["target_acc"] == pytest.approx(100 * (1 + 11 / 13) / 2) and s["read_acc"] == pytest.approx(100 * (1 + 11 / 13) / 2)
    assert s["err_only_ub"] == pytest.approx(50.0)                       # the UB: 0 on +, 100 on -
    assert s["err_far_ub"] == pytest.approx(100.0 / 4)                   # positions 0 and 12 of both strands: one of four wrong
    assert s["err_close_ub"] == 0.0 and s["err_ub_d_1"] == 0.0 and s["err_ub_d_4"] == 0.0
    assert s["acc_xna"] == pytest.approx(100 * (12 / 13 + 11 / 13) / 2) and s["acc_pc"] == pytest.approx(100.0)
    assert s["specificity"] == pytest.approx(100 * (1 - (1 / 12) / 3))
    assert s["precision"] == pytest.approx(100 * (1 - 0.5))             # the mean of (0, 1), the nan left out
    assert (s["true_pos"], s["false_neg"], s["false_pos"], s["true_neg"]) == (1, 1, 1, 27)
    assert s["f1_score"] == pytest.approx(50.0) and s["f2_score"] == pytest.approx(50.0)
    rows = rep.by_target()
    assert [(r[0], r[1], r[2], r[4]) for r in rows] == [("P", "F", "PC", 1), ("T", "F", "XNA", 1), ("T", "R", "XNA", 1)]
    labels = ubreport.position_labels(13, [6])
    assert labels["only_ub"].tolist() == [6] and labels["outside_ub_area"].tolist() == [0, 12]
    assert labels["dist_ub_d-6"].tolist() == [0, 12] and labels["dist_ub_d-11+"].size == 0
    assert ubreport.position_labels(4, [])["no_ub"].tolist() == [0, 1, 2, 3]


def _args(**kw):
    from xna_basecaller_amd.cli import basecaller
    args = basecaller.argparser().parse_args(["model", "reads"])
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def test_ub_report_refusals():
    from xna_basecaller_amd.cli import basecaller
    assert basecaller.ub_report_refusal(_args()) is None
    assert basecaller.ub_report_refusal(_args(ub_report="p", reference="lib.fasta")) is None
    assert "--reference" in basecaller.ub_report_refusal(_args(ub_report="p"))
    assert "one GPU" in basecaller.ub_report_refusal(_args(ub_report="p", reference="lib.fasta"), world=2)
    assert "--save-ctc" in basecaller.ub_report_refusal(_args(ub_report="p", reference="lib.fasta", save_ctc=True))
    r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "basecaller", "nomodel", "noreads", "--ub-report", "p"], cwd=ROOT,
                       capture_output=True, timeout=120)
    assert r.returncode == 1 and b"--ub-report tallies the mappings of --reference" in r.stderr


def test_analyze_arguments(tmp_path):
    from xna_basecaller_amd.cli import analyze
    p = analyze.argparser()
    a = p.parse_args(["lib.fasta", "calls.paf", "-R", "reads-run1.fastq", "-u", "Y", "-D", "--save_perf_per_read"])
    assert a.ubs == "Y" and a.save_detailed_perf and a.save_perf_per_read and not a.save_confusion_matrix
    assert analyze.output_prefix("/x/calls.paf", "/y/reads-run1.fastq") == "/x/results_summ-run1"
    rows = [dict(strand=1, k=0), dict(strand=-1, k=1)]
    assert analyze.select(rows) == rows and analyze.select(rows, ubs="X") == rows[:1] and analyze.select(rows, ubs="Y") == rows[1:]
    assert analyze.select(rows, only_strand="R") == rows[1:] and analyze.select(rows, only_strand="+") == rows[:1]
    for bad in (["lib.fasta", "calls.paf"], ["lib.fasta", "calls.paf", "-R", "r.fastq", "-u", "Z"],
                ["lib.fasta", "calls.paf", "-R", "r.fastq", "-S", "Q"]):
        with pytest.raises(SystemExit):
            p.parse_args(bad)
    r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "analyze", str(tmp_path / "no.fasta"), str(tmp_path / "no.paf"),
                        "-R", str(tmp_path / "no.fastq")], cwd=ROOT, capture_output=True, timeout=120)
    assert r.returncode != 0 and b"no file" in r.stderr
