"""CPU: the host side of demultiplexing by barcode.  tests/bcdist_ref.py (the restatement of xb_barcode_dist's contract) against
what the reference's own get_barcode_match_score returned (tests/golden/bcdist.json, made by tests/golden/make_bcdist_golden.py);
the two-step filter and the demux / align figures on a table made by hand; the summary's column order with and without the
setting; the refusals of `basecaller --max-bc-dist`; the new flags of `analyze`."""
import gzip
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import bcdist_ref
from conftest import GOLDEN, ROOT


@pytest.fixture(scope="module")
def golden():
    with open(os.path.join(GOLDEN, "bcdist.json")) as fh:
        return json.load(fh)


def test_fixture_covers_what_it_must(golden):
    cases = {c["read_id"]: c for c in golden["cases"]}
    rows = list(cases.values())
    assert {c["strand"] for c in rows} == {"+", "-"}
    assert {c["bc_len"] for c in rows} == {24, 30} and {c["bc_pos"] for c in rows} == {25, 23}
    assert any(c["target_start"] > c["bc_pos"] for c in rows) and any(0 < c["target_start"] < c["bc_pos"] for c in rows)
    assert any(c["q_st_aligned"] + c["bc_pos"] - c["target_start"] < 0 for c in rows)                      # start clamped to 0
    assert any(0 < max(c["q_st_aligned"] + c["bc_pos"] - c["target_start"], 0) < c["relax"] for c in rows)  # windows clipped at 0
    assert any(c["barcode_detected_len"] < c["bc_len"] for c in rows)                                      # off the read's end
    assert any(c["strand"] == "-" and set("XY") & set(c["barcode_detected"]) for c in rows)
    assert cases["xy_letters_minus"]["barcode_distance"] == 0 and cases["xy_letters_swapped_minus"]["barcode_distance"] == 2
    # the tie: every window from the winner on reads the same letters, and the first of them is reported
    tie = cases["homopolymer_tie"]
    assert tie["barcode_distance"] == 0 and tie["barcode_start"] == 25 and tie["call"][26:26 + 24] == tie["call"][25:25 + 24]
    assert cases["homopolymer_tie_minus"]["barcode_start"] == 25 - 3
    assert {c["relax"] for c in rows} >= {0, 3, 5}
    assert all(c["barcode_detected_len"] > 0 for c in rows)                                                # the reference's len(None)


def test_restatement_equals_the_reference(golden):
    templates = golden["templates"]
    for c in golden["cases"]:
        strand = 1 if c["strand"] == "+" else -1
        d, start, end, obs_len = bcdist_ref.row(templates[c["target_id"]], c["call"], strand, c["q_st_aligned"], c["target_start"],
                                                c["bc_pos"], c["bc_len"], c["relax"])
        assert (d, start, end, obs_len) == (c["barcode_distance"], c["barcode_start"], c["barcode_end"], c["barcode_detected_len"]), \
            c["read_id"]
        q = bcdist_ref.query_letters(c["call"], strand)
        assert "".join(q[start:end]) == c["barcode_detected"], c["read_id"]


def test_restatement_through_arrays_and_its_edges(golden):
    templates = list(golden["templates"].values())
    names = list(golden["templates"])
    cases = [c for c in golden["cases"] if c["bc_len"] == 24 and c["relax"] == 3]
    n = len(cases) + 2
    rows = np.zeros((n, 96), np.int8)
    lens = np.zeros(n, np.int32)
    mapped = {k: np.zeros(n, np.int32) for k in ("tmpl", "q_st", "r_st")}
    mapped["strand"] = np.zeros(n, np.int8)
    for k, c in enumerate(cases):
        call = c["call"].encode()
        rows[k, :len(call)] = np.frombuffer(call, np.int8)
        lens[k] = len(call)
        mapped["tmpl"][k], mapped["strand"][k] = names.index(c["target_id"]), 1 if c["strand"] == "+" else -1
        mapped["q_st"][k], mapped["r_st"][k] = c["q_st_aligned"], c["target_start"]
    mapped["tmpl"][n - 2] = -1                                           # unmapped
    mapped["tmpl"][n - 1] = 0                                            # mapped, but the row is empty
    out = bcdist_ref.dist(rows, lens, mapped, templates, 25, 24, 3)
    for k, c in enumerate(cases):
        assert [int(out[f][k]) for f in bcdist_ref.OUTPUTS] == [c["barcode_distance"], c["barcode_start"], c["barcode_end"],
                                                                 c["barcode_detected_len"]], c["read_id"]
    assert [int(out[f][n - 2]) for f in bcdist_ref.OUTPUTS] == [-1, 0, 0, 0]
    assert [int(out[f][n - 1]) for f in bcdist_ref.OUTPUTS] == [24, 22, 46, 0]       # nothing observed: 24 deletions, the first window
    # an empty barcode (bc_pos beyond the template): the distance is what was observed
    assert bcdist_ref.row("ACGT", "ACGTACGTAC", 1, 0, 0, 4, 3, 1) == (3, 3, 6, 3)
    assert bcdist_ref.row("ACGT", "ACGTACGTAC", 1, 0, 0, 9, 3, 1) == (0, 10, 13, 0)  # windows of 2, 1 and 0 letters: the empty one
    assert bcdist_ref.levenshtein("kitten", "sitting") == 3 and bcdist_ref.levenshtein("", "abc") == 3


# ---- the filter, by hand ---------------------------------------------------------------------------------------------------
TABLE = [                   # (read id, distance)
    ("r1", 2), ("r1", 0), ("r1", 5),        # three alignments: the one at 0 stays
    ("r2", 6),                              # over the limit
    ("r3", 4), ("r3", 4),                   # a tie at the read's minimum: both stay
    ("r4", 7), ("r4", 5),                   # the smaller one is within the limit, the other is not
    ("r5", -1),                             # never mapped
    ("r6", 5),                              # exactly the limit
]


def test_filter_two_steps_by_hand():
    from xna_basecaller_amd import ubreport
    ids, dist = [r for r, _ in TABLE], [d for _, d in TABLE]
    keep = ubreport.demux_filter(dist, ids, 5)
    assert keep == [1, 4, 5, 7, 9]
    assert keep == bcdist_ref.demux(dist, ids, 5)
    assert ubreport.demux_filter(dist, ids, 0) == [1] and ubreport.demux_filter(dist, ids, 7) == [1, 3, 4, 5, 7, 9]
    assert ubreport.demux_filter(np.asarray(dist, np.int32), ids, 5) == keep
    assert ubreport.demux_filter([], [], 5) == []


class _FakeContext:
    """Stands in for the device: barcode_dist returns what the test planted, ub_tally counts a row per mapped row."""

    def __init__(self, dist):
        self.dist = np.asarray(dist, np.int32)
        self.tallied = []

    def barcode_dist(self, rows, lens, got, library, offsets, bc_pos, bc_len, relax=3):
        self.asked = (bc_pos, bc_len, relax)
        n = len(lens)
        return {"bc_dist": self.dist[:n], "bc_start": np.full(n, 25, np.int32), "bc_end": np.full(n, 25 + bc_len, np.int32),
                "bc_obs_len": np.full(n, bc_len, np.int32)}

    def ub_tally(self, rows, lens, got, library, offsets, acc=None):
        self.tallied.append(np.asarray(got["tmpl"]).copy())
        counts = np.tile(np.array([13, 1, 1, 10, 10, 2, 2, 1], np.int32), (len(lens), 1))
        for t, s in zip(got["tmpl"], got["strand"]):
            if t >= 0:
                acc.reads[t, 1 if s < 0 else 0] += 1
        return counts, acc


def _got(tmpl):
    n = len(tmpl)
    got = {k: np.zeros(n, np.int32) for k in ("q_st", "r_st", "r_en")}
    got["tmpl"] = np.asarray(tmpl, np.int32)
    got["q_en"] = np.full(n, 13, np.int32)
    got["n_ops"] = np.full(n, 13, np.int32)
    got["strand"] = np.ones(n, np.int8)
    got["ops"] = np.full((n, 32), ord("="), np.uint8)
    return got


def test_report_masks_failed_rows_and_counts_demux_and_align():
    from xna_basecaller_amd import ubreport
    rep = ubreport.Report(["T"], ["ACGTACNACGTAC"], demux=(5, 3, 4, 2))
    ctx = _FakeContext([0, 6, 5, -1, 3])
    ids = ["a", "b", "c", "d", "e"]
    rep.add(ctx, np.zeros((5, 16), np.int8), np.full(5, 13, np.int32), _got([0, 0, 0, -1, 0]), ids)
    assert ctx.asked == (3, 4, 2)
    assert ctx.tallied[0].tolist() == [0, -1, 0, -1, 0]                  # what xb_ub_tally was shown: the failed rows unmapped
    assert rep.read_ids == ["a", "c", "e"] and rep.barcode == [(0, 25, 29), (5, 25, 29), (3, 25, 29)]
    rep.shown.update(["f", "g", "h"])                                   # reads that never reached the mapper still count
    s = rep.summary()
    assert s["demux"] == pytest.approx(100 * 3 / 8) and s["align"] == pytest.approx(100 * 4 / 8)
    assert s["num_aligned_reads"] == 3
    rep.n_reads = 16                                                    # the reads on file, when the caller knows them
    s = rep.summary()
    assert s["demux"] == pytest.approx(100 * 3 / 16) and s["align"] == pytest.approx(100 * 4 / 16)


TODAY = ["num_aligned_reads", "target_acc", "read_acc", "err_far_ub", "err_close_ub", "err_only_ub", "err_ub_d_1", "err_ub_d_2",
         "err_ub_d_3", "err_ub_d_4", "acc_xna", "acc_pc", "specificity", "precision", "f1_score", "f2_score", "true_pos", "false_neg",
         "false_pos", "true_neg"]


def test_summary_columns_with_and_without_the_setting(tmp_path):
    from xna_basecaller_amd import ubreport
    plain = ubreport.Report(["T"], ["ACGTACNACGTAC"])
    ctx = _FakeContext([0, 9])
    plain.add(ctx, np.zeros((2, 16), np.int8), np.full(2, 13, np.int32), _got([0, 0]), ["a", "b"])
    assert ctx.tallied[0].tolist() == [0, 0] and not hasattr(ctx, "asked")          # no barcode call, nothing masked
    assert list(plain.summary()) == TODAY
    with_d = ubreport.Report(["T"], ["ACGTACNACGTAC"], demux=(5, 25, 24, 3))
    with_d.add(_FakeContext([0, 9]), np.zeros((2, 16), np.int8), np.full(2, 13, np.int32), _got([0, 0]), ["a", "b"])
    at = TODAY.index("specificity")
    assert list(with_d.summary()) == TODAY[:at] + ["demux", "align"] + TODAY[at:]
    # the files: the per-read table ends in the three barcode columns with the setting, and is today's without
    for rep, name in ((plain, "plain"), (with_d, "demux")):
        rep.write(str(tmp_path / name), by_tar=False, by_read=True, confusion=False)
    head = gzip.open(str(tmp_path / "plain-by_read.csv.gz"), "rt").read().split("\n")[0].split(",")
    assert head[-1] == "true_neg" and "barcode_distance" not in head
    lines = gzip.open(str(tmp_path / "demux-by_read.csv.gz"), "rt").read().strip().split("\n")
    assert lines[0].split(",")[-3:] == ["barcode_distance", "barcode_start", "barcode_end"] and lines[0].split(",")[:-3] == head
    assert len(lines) == 2 and lines[1].split(",")[0] == "a" and lines[1].split(",")[-3:] == ["0", "25", "49"]
    assert open(str(tmp_path / "demux.csv")).read().split("\n")[0].split(",") == list(with_d.summary())


# ---- the command lines -----------------------------------------------------------------------------------------------------
def _args(**kw):
    from xna_basecaller_amd.cli import basecaller
    args = basecaller.argparser().parse_args(["model", "reads"])
    for k, v in kw.items():
        setattr(args, k, v)
    return args


def test_max_bc_dist_refusals():
    from xna_basecaller_amd.cli import basecaller
    a = basecaller.argparser().parse_args(["model", "reads"])
    assert a.max_bc_dist is None and (a.barcode_start, a.barcode_len, a.barcode_relax) == (25, 24, 3)
    assert basecaller.max_bc_dist_refusal(_args()) is None
    assert basecaller.max_bc_dist_refusal(_args(max_bc_dist=5, ub_report="p", reference="lib.fasta")) is None
    assert "--ub-report" in basecaller.max_bc_dist_refusal(_args(max_bc_dist=5))
    assert "--ub-report" in basecaller.max_bc_dist_refusal(_args(max_bc_dist=5, reference="lib.fasta"))
    for bad in (dict(max_bc_dist=-1), dict(barcode_len=0), dict(barcode_len=65), dict(barcode_relax=9), dict(barcode_start=-1)):
        why = basecaller.max_bc_dist_refusal(_args(**dict(dict(max_bc_dist=5, ub_report="p", reference="lib.fasta"), **bad)))
        assert why is not None and "1 .. 64" in why, bad
    # the refusals of --ub-report itself stay what they were
    assert "--reference" in basecaller.ub_report_refusal(_args(ub_report="p", max_bc_dist=5))
    r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "basecaller", "nomodel", "noreads", "--max-bc-dist", "5"], cwd=ROOT,
                       capture_output=True, timeout=120)
    assert r.returncode == 1 and b"--max-bc-dist filters the reads of --ub-report" in r.stderr


def test_analyze_flags():
    from xna_basecaller_amd.cli import analyze
    p = analyze.argparser()
    a = p.parse_args(["lib.fasta", "calls.paf", "-R", "calls.fastq"])
    assert a.max_bc_dist is None and analyze.demux_setting(a) is None
    a = p.parse_args(["lib.fasta", "calls.paf", "-R", "calls.fastq", "-d", "5"])
    assert analyze.demux_setting(a) == (5, 25, 24, 3)
    a = p.parse_args(["lib.fasta", "calls.paf", "-R", "calls.fastq", "--max_bc_dist", "8", "--barcode-start", "23", "--barcode-len", "30",
                      "--barcode-relax", "2"])
    assert analyze.demux_setting(a) == (8, 23, 30, 2)
    with pytest.raises(SystemExit):
        p.parse_args(["lib.fasta", "calls.paf", "-R", "calls.fastq", "-d", "five"])


def test_exports_name_the_new_entry_points():
    from xna_basecaller_amd import _lib
    header = open(os.path.join(ROOT, "include", "xna_basecaller.h")).read()
    for name in ("xb_barcode_dist", "xb_barcode_dist_dev"):
        assert name in _lib.EXPORTS and ("XB_API int %s(" % name) in header
    assert "PARITY UNPINNED for the mapping, the per-row function pinned by tests/golden/bcdist.json" in " ".join(header.split())
