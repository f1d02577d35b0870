"""CPU: the template mapper's contract restated (tests/map_ref.py) against brute force, the host formatters that turn
alignment columns into what a mappy.Alignment carries, and the writers with and without an aligner."""
import io as pyio
import itertools
import json
import os
import types

import numpy as np

import pytest

import evalloop_metrics as em
import map_cases
import map_ref
from conftest import GOLDEN
from xna_basecaller_amd import io as xio
from xna_basecaller_amd.aligner import MAP_ONT, Mapping, TemplateAligner, align_map, mapq, read_fasta


def _ops_score(ops, q, t, qi, ti, scoring):
    """Score of the alignment columns `ops` from (qi, ti) under the contract: affine gaps cost open + k * extend."""
    match, mismatch, go, ge, amb = scoring
    total, prev = 0, ""
    for op in ops:
        if op == "M":
            total += -amb if (q[qi] == 4 or t[ti] == 4) else (match if q[qi] == t[ti] else -mismatch)
            qi, ti = qi + 1, ti + 1
        else:
            total -= ge + (go if prev != op else 0)
            qi, ti = qi + (op == "I"), ti + (op == "D")
        prev = op
    return total, qi, ti


def _brute(q, t, scoring):
    """Every local alignment of q against t: best score and the set of its end cells (1-based)."""
    best, ends = 0, set()

    def walk(qi, ti, ops, start):
        nonlocal best, ends
        if ops and ops[-1] == "M":                       # an optimal local alignment ends (and starts) on a column
            s, _, _ = _ops_score(ops, q, t, start[0], start[1], scoring)
            if s > best:
                best, ends = s, {(qi, ti)}
            elif s == best and s > 0:
                ends.add((qi, ti))
        if qi < len(q) and ti < len(t):
            walk(qi + 1, ti + 1, ops + "M", start)
        if ops:
            if qi < len(q):
                walk(qi + 1, ti, ops + "I", start)
            if ti < len(t):
                walk(qi, ti + 1, ops + "D", start)

    for a in range(len(q)):
        for b in range(len(t)):
            walk(a, b, "", (a, b))
    return best, ends


def test_restatement_against_brute_force_on_tiny_cases():
    rng = np.random.default_rng(2)
    letters = "ACGTN"
    seen_tie = 0
    for trial in range(60):
        scoring = MAP_ONT if trial % 2 == 0 else (5, 4, 1, 1, 1)
        read = "".join(rng.choice(list(letters), rng.integers(1, 6), p=[.3, .3, .17, .17, .06]))
        templates = ["".join(rng.choice(list(letters), rng.integers(1, 6), p=[.3, .3, .17, .17, .06])) for _ in range(2)]
        got = map_ref.map_read(read, templates, scoring)
        cand = []
        for t, tpl in enumerate(templates):
            for s in (0, 1):
                qa = map_ref.codes(read) if s == 0 else map_ref.revcomp_codes(map_ref.codes(read))
                score, ends = _brute(list(qa), list(map_ref.codes(tpl)), scoring)
                cand.append((score, t, s, ends))
        top = max(c[0] for c in cand)
        assert got["score"] == top, (read, templates)
        if top == 0:
            assert got["tmpl"] == -1
            continue
        winners = [c for c in cand if c[0] == top]
        seen_tie += len(winners) > 1 or len(winners[0][3]) > 1
        _, t, s, ends = winners[0]                                         # lowest template, + before -
        assert (got["tmpl"], got["strand"]) == (t, -1 if s else 1), (read, templates)
        assert (got["q_en"], got["r_en"]) == min(ends), (read, templates, ends)       # first end cell in row-major order
        others = [c[0] for c in cand if c[1] != t]
        assert got["second"] == max(others)
        # the reported columns are an alignment of exactly that score
        qa = map_ref.codes(read) if s == 0 else map_ref.revcomp_codes(map_ref.codes(read))
        ops = got["ops"].decode().replace("=", "M").replace("X", "M")
        sc, qe, re_ = _ops_score(ops, list(qa), list(map_ref.codes(templates[t])), got["q_st"], got["r_st"], scoring)
        assert (sc, qe, re_) == (top, got["q_en"], got["r_en"])
    assert seen_tie >= 5
    # the cell-by-cell matrices and the row recurrence agree
    for _ in range(10):
        q, t = rng.integers(0, 5, rng.integers(1, 20)), rng.integers(0, 5, rng.integers(1, 20))
        for a, b in zip(map_ref.matrices(q, t), map_ref.matrices_by_rows(q, t)):
            assert np.array_equal(a[1:, 1:], b[1:, 1:])


def test_cell_by_cell_matrices_equal_the_row_recurrence_at_every_scoring():
    """The row recurrence (what map_read runs) against the cell-by-cell matrices at the corners of the scoring's range: open = 0,
    extend = 0, no penalties at all, every value 1000 -- H, E and F, cell for cell, on pairs with ambiguous letters."""
    rng = np.random.default_rng(8)
    pairs = [(rng.integers(0, 5, rng.integers(1, 22)), rng.integers(0, 5, rng.integers(1, 22))) for _ in range(36)]
    pairs += [(np.array([0, 0, 1, 1, 4, 2]), np.array([0, 1, 1, 0, 0, 1, 4, 2])), (np.array([3]), np.array([3])), (np.array([4]), np.array([4, 4]))]
    for scoring in map_cases.SCORINGS + ((1000, 0, 0, 0, 0), map_ref.DEFAULT_SCORING, (5, 4, 8, 4, 1)):
        for q, t in pairs:
            for name, a, b in zip("HEF", map_ref.matrices(q, t, scoring), map_ref.matrices_by_rows(q, t, scoring)):
                assert np.array_equal(a[1:, 1:], b[1:, 1:]), (scoring, name, q, t)


def _family_params():
    return [pytest.param(f, a, id=f if a is None else "%s-%s" % (f, a)) for f, (_, args, _) in map_cases.FAMILIES.items() for a in args]


@pytest.mark.parametrize("family,arg", _family_params())
def test_every_case_family_is_at_its_limit_in_the_restatement(family, arg):
    """The condition of every family of tests/map_cases.py on the restatement's outputs alone (the GPU tier compares the device
    with these same outputs), and replay() on every mapped row of them: the restatement's columns add up to its scores."""
    map_cases.condition(family, arg)
    mapped = sum(map_cases.replay_all(case, want) for case, want in zip(map_cases.cases(family, arg), map_cases.expected(family, arg)))
    assert mapped > 0


def test_replay_accepts_the_restatement_and_refuses_corrupted_rows():
    rng = np.random.default_rng(31)
    templates = [map_cases.random_letters(rng, L, 0.05) for L in (40, 33, 7)]
    reads = map_cases.mutated_reads(templates, 40, rng)
    for scoring in (map_ref.DEFAULT_SCORING, (5, 4, 8, 4, 1), (1, 0, 0, 0, 0), (2, 4, 0, 2, 1), (2, 4, 4, 0, 1)):
        case = map_cases.Case(reads, templates, scoring, None)
        rows, lens = map_cases.pack(case)
        assert map_cases.replay_all(case, map_ref.map_rows(rows, lens, templates, scoring)) >= 30
    # a read with a substitution, a deletion and an insertion against its template; then the row corrupted by hand
    t = map_cases.random_letters(rng, 64)
    read = "TT" + t[:15] + ("A" if t[15] != "A" else "C") + t[16:30] + t[31:46] + "GG" + t[46:]
    case = map_cases.Case([read, map_cases.revcomp(read)], [t], map_ref.DEFAULT_SCORING, None)
    rows, lens = map_cases.pack(case)
    want = map_ref.map_rows(rows, lens, [t], case.scoring)
    assert map_cases.replay_all(case, want) == 2
    assert all(c in want["ops"][0].tobytes() for c in b"=XID") and want["strand"].tolist() == [1, -1]
    for r in range(2):
        good = {k: want[k][r].copy() for k in want}
        map_cases.replay(rows[r], lens[r], t, good, case.scoring)
        flipped = dict(good, ops=good["ops"].copy())
        at = int(np.flatnonzero(flipped["ops"] == ord("="))[3])
        flipped["ops"][at] = ord("X")
        shorter = dict(good, ops=good["ops"].copy())
        shorter["ops"][at] = ord("D")                                  # a column turned into a gap: the walk ends elsewhere
        for bad in (flipped, shorter, dict(good, q_st=good["q_st"] + 1), dict(good, score=good["score"] + case.scoring[0]),
                    dict(good, score=good["score"] - case.scoring[0]), dict(good, strand=np.int8(-good["strand"])),
                    dict(good, second=good["score"] + 1), dict(good, n_ops=good["n_ops"] - 1), dict(good, r_en=good["r_en"] + 1)):
            with pytest.raises(AssertionError):
                map_cases.replay(rows[r], lens[r], t, bad, case.scoring)


def test_tie_rules_of_the_restatement():
    t = "ACGGTCATTGCA"
    m = map_ref.map_read(t, ["TTTTTTTT", t, t])
    assert (m["tmpl"], m["strand"], m["second"]) == (1, 1, m["score"])
    pal = "ACGTTGCATGCAACGT"
    assert map_ref.map_read(pal, [pal])["strand"] == 1
    assert map_ref.map_read("ACGT", ["ACGTCCCCACGT"])["r_en"] == 4
    # diagonal before deletion before insertion; a homopolymer gap lands where that order puts it
    m = map_ref.map_read("ACGATCGATTTCGATCGAAGCT", ["ACGATCGATTTTCGATCGAAGCT"])
    assert m["ops"].decode().count("D") == 1 and m["ops"].decode().index("D") == 8
    assert map_ref.mapq(100, 0) == 60 and map_ref.mapq(100, 100) == 0 and map_ref.mapq(100, 50) == 30 == mapq(100, 50)


def test_ops_to_cigar_nm_md_cs():
    tpl = "ACGTNACGTTGA"
    m = Mapping("T1", tpl, "ggACGTXACTTcGAc".upper(), +1, 0, 2, "====X==D==I==", score=14, second=7)
    assert (m.cigar_str, m.NM, m.MD, m.blen, m.mlen) == ("7M1D2M1I2M", 3, "4N2^G4", 13, 10)
    assert m.cs == ":4*nn:2-g:2+c:2" and m.cigar == [(7, 0), (1, 2), (2, 0), (1, 1), (2, 0)]
    assert (m.q_st, m.q_en, m.r_st, m.r_en, m.ctg_len, m.mapq) == (2, 14, 0, 12, 12, 30)
    # reverse strand: the aligned letters are the reverse complement; q_st / q_en go back to the call as it was made
    call = "TTCAAACGTYACGT"                       # reverse complement of the codes: ACGT n ACGTTTGAA
    r = Mapping("T1", "ACGTNACGTTTGA", call, -1, 0, 0, "====X========", score=23, second=23)
    assert (r.cigar_str, r.NM, r.MD, r.cs, r.mapq) == ("13M", 1, "4N8", ":4*nn:8", 0)
    assert (r.q_st, r.q_en) == (1, 14)
    # consecutive mismatches, a deletion followed by a mismatch, an insertion inside a match run
    x = Mapping("T", "AACCGGTT", "AAGGGTT", +1, 0, 0, "==XXD=I=")
    assert (x.MD, x.cs, x.cigar_str) == ("2C0C0^G2", ":2*cg*cg-g:1+t:1", "4M1D1M1I1M")
    # an unnatural base called at the template's N prints *nn, a natural base there *na
    assert Mapping("T", "AN", "AX", +1, 0, 0, "=X").cs == ":1*nn" and Mapping("T", "AN", "AA", +1, 0, 0, "=X").cs == ":1*na"


def _designed_score(cs, scoring):
    match, mismatch, go, ge, amb = scoring
    total = 0
    for tok in em._CS_TOKEN.findall(cs):
        kind, val = tok[0], tok[1:]
        if kind == ":":
            total += match * int(val)
        elif kind == "*":
            total -= amb if "n" in val else mismatch
        else:
            total -= go + ge * len(val)
    return total


def test_designed_reads_map_to_their_template_and_strand():
    """The 33 designed reads of evalacc.json against its 3 templates: target and strand right for all, the restatement's
    score at least the designed alignment's (optimality).  How many reproduce the designed cs byte for byte depends on gap
    placement at ties: printed, not asserted; for those, write_paf's text gives back the stored per-read metrics."""
    g = json.load(open(os.path.join(GOLDEN, "evalacc.json")))
    names = list(g["templates"])
    templates = [g["templates"][k] for k in names]
    rows = em.parse_paf(g["paf"])
    same_cs = same_coords = 0
    for (rid, _, seq), row, want in zip(g["reads"], rows, g["per_read"]):
        assert row["read_id"] == rid
        m = map_ref.to_mapping(map_ref.map_read(seq, templates), names, templates, seq)
        assert m is not None and m.ctg == row["target_id"] and ("+" if m.strand == 1 else "-") == row["strand"], rid
        assert m.score >= _designed_score(row["cs"], MAP_ONT), (rid, m.score, row["cs"])
        same_coords += (m.r_st, m.r_en) == (row["target_start"], row["target_end"])
        if m.cs != row["cs"]:
            continue
        same_cs += 1
        buf = pyio.StringIO()
        xio.write_paf(buf, rid, len(seq), m)
        (mine,) = em.parse_paf(buf.getvalue())
        for k in ("read_length", "read_start", "read_end", "strand", "target_id", "target_length", "target_start", "target_end",
                  "n_matches", "block_length", "cs"):
            assert mine[k] == row[k], (rid, k)
        assert "\ttp:A:P\ts1:i:%d\ts2:i:%d\tcs:Z:" % (m.score, m.second) in buf.getvalue()
        _, metrics = em.read_metrics(mine, g["templates"][mine["target_id"]], seq)
        for k, v in want.items():
            if k in ("read_id", "target_id", "strand"):
                continue
            if v is None:
                assert np.isnan(metrics[k]), (rid, k)
            elif isinstance(v, str):
                assert metrics[k] == v, (rid, k)
            else:
                assert abs(metrics[k] - v) < 1e-12, (rid, k)
    print("designed cs reproduced byte for byte: %d of 33; template coordinates: %d of 33" % (same_cs, same_coords))
    assert same_cs > 0


# the five aligned cases of sam.json as alignment columns: (ops, template letters at the mismatches / deletions, score, second)
_SAM_CASES = [("==========", {}, 20, 0), ("===XI====", {6: "A"}, 600, 228), ("===D=====", {8: "C"}, 100, 79),
              ("==X====X===X", {102: "T", 107: "G", 111: "A"}, 50, 50), ("=", {}, 100, 98)]


def test_sam_records_and_summary_columns_through_a_mapping():
    g = json.load(open(os.path.join(GOLDEN, "sam.json")))
    assert len(g["aligned"]) == len(_SAM_CASES)
    for a, (ops, letters, score, second) in zip(g["aligned"], _SAM_CASES):
        want = a["mapping"]
        tpl = list("C" * 120)
        for pos, c in letters.items():
            tpl[pos] = c
        seq = a["sequence"]
        q_aligned = want["q_st"] if want["strand"] == 1 else len(seq) - want["q_en"]
        m = Mapping(want["ctg"], "".join(tpl), seq, want["strand"], want["r_st"], q_aligned, ops, score, second)
        for k, v in want.items():
            if k != "r_en":        # the fixture's stand-in objects carry an r_en of their own choosing (sam_record never reads it)
                assert getattr(m, k) == v, (a["read_id"], k, getattr(m, k), v)
        assert m.r_en == want["r_st"] + sum(ops.count(c) for c in "=XD")
        assert xio.sam_record(a["read_id"], seq, a["qstring"], m, tags=a["tags"]) == a["sam_record"]
        assert xio.sam_record(a["read_id"], seq, a["qstring"], m) == a["sam_record_no_tags"]
        read = types.SimpleNamespace(filename="f", read_id=a["read_id"], run_id="r", channel=1, mux=2, start=0.0, duration=1.0,
                                     template_start=0.0, template_duration=1.0)
        row = xio.summary_row(read, len(seq), 9.0, alignment=m)
        assert list(row) == list(xio.SUMMARY_COLUMNS + xio.ALIGNMENT_COLUMNS) and len(row) == 27
        ins, dels = ops.count("I"), ops.count("D")
        fwd = want["strand"] == 1
        assert [row[c] for c in xio.ALIGNMENT_COLUMNS] == [
            want["ctg"], want["r_st"], m.r_en, want["q_st"] if fwd else len(seq) - want["q_en"],
            want["q_en"] if fwd else len(seq) - want["q_st"], "+" if fwd else "-", len(ops), len(ops) - ins - dels, ops.count("="),
            ins, dels, ops.count("X"), want["mapq"], (want["q_en"] - want["q_st"]) / len(seq),
            ops.count("=") / (len(ops) - ins - dels), ops.count("=") / len(ops)]
    none = xio.summary_row(read, 5, 9.0, alignment=None)
    assert [none[c] for c in xio.ALIGNMENT_COLUMNS] == ["*", -1, -1, -1, -1, "*", 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0]
    assert list(xio.summary_row(read, 5, 9.0)) == list(xio.SUMMARY_COLUMNS)


def _records(g):
    reads = []
    for rec in g["records"]:
        r = types.SimpleNamespace(**rec["read"])
        r.signal = np.zeros(40, np.float32)
        r.start = r.duration = r.template_start = r.template_duration = 0.0
        r.tagdata = (lambda tags: lambda: tags)(rec["tags"][2:])
        reads.append((r, {"sequence": rec["sequence"], "qstring": rec["qstring"],
                          "mean_qscore": float(rec["tags"][1].split(":")[2])}))
    return reads


def test_writer_without_an_aligner_is_unchanged_and_with_one_adds_the_columns(tmp_path):
    g = json.load(open(os.path.join(GOLDEN, "sam.json")))
    out = pyio.StringIO()
    xio.Writer("w", iter(_records(g)), fd=out, group_key=g["model"], groups=set(g["groups"]), summary=str(tmp_path / "a.tsv")).run()
    header = xio.sam_header(sorted(g["groups"]))
    assert "ID:aligner" not in header
    assert out.getvalue() == header + "".join(rec["sam_record"] + "\n" for rec in g["records"])
    fq = pyio.StringIO()
    xio.Writer("wfq", iter(_records(g)), fd=fq, group_key=g["model"], summary=str(tmp_path / "b.tsv")).run()
    assert fq.getvalue() == "".join("@%s %s\n%s\n+\n%s\n" % (rec["read"]["read_id"], "\t".join(rec["tags"]), rec["sequence"],
                                                              rec["qstring"]) for rec in g["records"])
    for name in ("a.tsv", "b.tsv"):
        lines = open(tmp_path / name, newline="").read().split("\r\n")
        assert lines[0].split("\t") == list(xio.SUMMARY_COLUMNS) and all(len(l.split("\t")) == 11 for l in lines[:-1])
    # with an aligner: this package's @PG line, aligned records, 27 summary columns, PAF rows for the mapped reads only
    tpl = "GGACGTNNACGTCC"
    stub = types.SimpleNamespace()
    recs = _records(g)[:2]
    recs[0][1]["mapping"] = Mapping("T9", tpl, recs[0][1]["sequence"], +1, 2, 0, "====XX====", 14, 3)
    recs[1][1]["mapping"] = None
    sam, paf = pyio.StringIO(), pyio.StringIO()
    xio.Writer("w", iter(recs), aligner=stub, fd=sam, group_key=g["model"], groups=set(g["groups"]), summary=str(tmp_path / "c.tsv"),
               paf=paf).run()
    text = sam.getvalue().split("\n")
    from xna_basecaller_amd import __version__
    assert "@PG\tID:aligner\tPN:xnacall-map\tVN:%s\tDS:" % __version__ in sam.getvalue() and "minimap2" not in sam.getvalue()
    body = [l for l in text if l and not l.startswith("@")]
    assert body[0].split("\t")[1:9] == ["0", "T9", "3", "47", "10M", "*", "0", "0"] and "\tNM:i:2\tMD:Z:4N0N4\t" in body[0]
    assert body[1].split("\t")[1:6] == ["4", "*", "0", "0", "*"]
    rows = [l.split("\t") for l in open(tmp_path / "c.tsv", newline="").read().split("\r\n")[:-1]]
    assert [len(r) for r in rows] == [27, 27, 27] and rows[1][11] == "T9" and rows[2][11] == "*"
    assert paf.getvalue() == "%s\t10\t0\t10\t+\tT9\t14\t2\t12\t8\t10\t47\ttp:A:P\ts1:i:14\ts2:i:3\tcs:Z::4*nn*nn:4\n" % recs[0][0].read_id


def test_fasta_reader_and_align_map_order(tmp_path):
    p = tmp_path / "lib.fa"
    p.write_text(">t1 first template\nACGT\nacgt\n\n>t2\tx\nGGNN\n>t3\nA\n")
    assert read_fasta(str(p)) == [("t1", "ACGTacgt"), ("t2", "GGNN"), ("t3", "A")]
    poc = read_fasta(os.path.join(GOLDEN, "poc_refdb_short.fasta"))
    assert len(poc) == 20 and poc[0][0] == "XNA01" and all(set(s) <= set("ACGTN") for _, s in poc)

    class Fake(TemplateAligner):
        def __init__(self):
            self.calls = []

        def map(self, sequences):
            self.calls.append(len(sequences))
            return [None if not s else len(s) for s in sequences]

    fake = Fake()
    items = [("r%d" % i, {"sequence": "A" * (i % 4)}) for i in range(10)]
    out = list(align_map(fake, iter(items), batch=4))
    assert [r for r, _ in out] == [r for r, _ in items] and fake.calls == [4, 4, 2]
    assert [res["mapping"] for _, res in out] == [None if i % 4 == 0 else i % 4 for i in range(10)]
    a = TemplateAligner.from_config(str(p), {"aligner": {"match": 5, "gap_open": 8}})
    assert tuple(a.scoring) == (5, 4, 8, 2, 1) and a.names == ["t1", "t2", "t3"] and a.offsets.tolist() == [0, 8, 12, 13]


# ---- the torchrun gather: every rank maps its own reads, rank 0 writes them -------------------------------------------

WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["XB_ROOT"])
import numpy as np
from xna_basecaller_amd import dist as xd
rank, world = xd.init_from_env(backend="gloo")
from xna_basecaller_amd.aligner import Mapping
from xna_basecaller_amd.cli.basecaller import _gathered_results, READ_FIELDS
class FakeRead:
    def __init__(self, i):
        self.index = i
        for k in READ_FIELDS: setattr(self, k, "%s%d" % (k[:2], i))
        self.signal = np.zeros(100 + i, np.float32)
    def tagdata(self): return ["mx:i:%d" % self.index]
class FakeLoader: total = 11
def mapping(i):
    return None if i % 3 == 0 else Mapping("T%d" % i, "ACGTNACGT", "ACGTXACG", 1 if i % 2 else -1, 0, 0, "====X===", 13, i)
def local(mapped):
    for i in range(rank, 11, 2):
        res = {"sequence": "ACGTXACG", "qstring": "OOOOOOOO"}
        if mapped:
            res["mapping"] = mapping(i)
        yield FakeRead(i), res
got = list(_gathered_results(local(True), FakeLoader, rank, world, window=2))
plain = list(_gathered_results(local(False), FakeLoader, rank, world, window=2))
if rank == 0:
    assert [r.read_id for r, _ in got] == ["re%d" % i for i in range(11)]
    for i, (_, res) in enumerate(got):
        want = mapping(i)
        assert "mapping" in res and (res["mapping"] is None) == (want is None)
        if want is not None:
            assert all(getattr(res["mapping"], k) == getattr(want, k) for k in Mapping.__slots__)
    assert all("mapping" not in res for _, res in plain)
else:
    assert got == [] and plain == []
xd.barrier()
print("rank", rank, "ok")
'''


def test_mappings_survive_the_world2_gather(tmp_path):
    import socket
    import subprocess
    import sys
    from conftest import ROOT
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        port = str(s.getsockname()[1])
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1", MASTER_PORT=port, XB_ROOT=ROOT)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE, stderr=subprocess.STDOUT))
    try:
        outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert "rank %d ok" % r in o
