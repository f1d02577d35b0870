"""CPU: the host side of `basecaller --save-ctc` -- read_chunks against what the reference's returned (tests/golden/savectc.json),
CTCWriter on hand-made (chunk, result) streams against the restatement in tests/savectc_ref.py, the files it leaves through
the package's own ctc-data loader and `segment -n`, and every refusal of the command line.  No device is touched."""
import io as stdio
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

import savectc_ref
from conftest import GOLDEN, ROOT
from xna_basecaller_amd import io as xio
from xna_basecaller_amd import reads as xreads
from xna_basecaller_amd.aligner import Mapping

POC = os.path.join(GOLDEN, "poc_refdb_short.fasta")


# ---- read_chunks ------------------------------------------------------------------------------------------------------
def test_read_chunks_against_the_reference():
    gold = json.load(open(os.path.join(GOLDEN, "savectc.json")))
    assert {c["count"] for c in gold["cases"]} >= {0, 1, 2, 3}
    for case in gold["cases"]:
        length, chunksize, overlap = case["length"], case["chunksize"], case["overlap"]
        signal = np.arange(length, dtype=np.float32)
        read = types.SimpleNamespace(read_id="read-%d" % length, signal=signal, duration=length / 4000.0, **gold["read"])
        got = list(xreads.read_chunks(read, chunksize=chunksize, overlap=overlap))
        assert len(got) == case["count"], case
        assert [c.read_id for c in got] == case["ids"]
        assert [int(c.signal[0]) for c in got] == case["first"] and [int(c.signal[-1]) for c in got] == case["last"]
        assert all(c.signal.shape == (chunksize,) for c in got)
        # strided views of the read's own signal, not copies
        assert all(np.shares_memory(c.signal, signal) for c in got)
        if got:
            c = got[0]
            assert [[c.run_id, c.filename, c.mux, c.channel, c.start, c.duration, c.template_start, c.template_duration]] == case["meta"]
            assert (length - chunksize) % (chunksize - overlap) == case["first"][0]
            assert repr(c) == "ReadChunk('%s')" % case["ids"][0]


# ---- CTCWriter on hand-made streams -------------------------------------------------------------------------------------
TEMPLATES = {"tA": "ACGTACGTACGTACGTACGT", "tN": "ACGTANGTACGTACGTNCGT", "tL": "acgtnACGTN"}


class _Lib:
    """What CTCWriter asks of an aligner: seq(name, start, end)."""
    seq = staticmethod(lambda name, start=0, end=None: TEMPLATES[name][start:end])


def _chunk(i, n=64):
    sig = (np.arange(n, dtype=np.float32) + 100 * i) / 7
    return types.SimpleNamespace(read_id="r%d:1:1" % i, run_id="run", filename="f.fast5", channel=5, mux=2, start=1.5, duration=2.0,
                                 template_start=1.5, template_duration=2.0, signal=sig)


def _mapping(ctg, sequence, strand, r_st, q_st_aligned, ops):
    return Mapping(ctg, TEMPLATES[ctg], sequence, strand, r_st, q_st_aligned, ops, score=30, second=3)


def _stream():
    """(chunk, result, expected verdict) -- every counter, 'both', an empty sequence, kept rows on both strands."""
    S = "ACGTACGTACGTACGTACGT"
    items = [
        (_chunk(0), {"sequence": "", "qstring": "", "mapping": None}, 3),
        (_chunk(1), {"sequence": "GGGG", "qstring": "OOOO", "mapping": None}, 2),
        (_chunk(2), {"sequence": S, "qstring": "O" * 20, "mapping": _mapping("tA", S, 1, 0, 0, "=" * 20)}, 0),
        (_chunk(3), {"sequence": S, "qstring": "O" * 20, "mapping": _mapping("tN", S, -1, 2, 1, "=" * 18)}, 0),
        # 19 / 20 against 0.95: equal is not below
        (_chunk(4), {"sequence": S, "qstring": "O" * 20, "mapping": _mapping("tA", S, 1, 0, 0, "=" * 19 + "X")}, 0),
        (_chunk(5), {"sequence": S, "qstring": "O" * 20, "mapping": _mapping("tA", S, 1, 0, 0, "=" * 18 + "XX")}, 8),
        (_chunk(6), {"sequence": S + "TTTT", "qstring": "O" * 24, "mapping": _mapping("tA", S + "TTTT", 1, 0, 0, "=" * 20)}, 16),
        (_chunk(7), {"sequence": S + "TTTT", "qstring": "O" * 24, "mapping": _mapping("tA", S + "TTTT", 1, 0, 0, "=" * 10 + "X" * 10)}, 24),
        (_chunk(8), {"sequence": S[:18], "qstring": "O" * 18, "mapping": _mapping("tA", S[:18], 1, 2, 0, "=" * 18)}, 0),
        (_chunk(9), {"sequence": "ACGTGACGTG", "qstring": "O" * 10, "mapping": _mapping("tL", "ACGTGACGTG", 1, 0, 0, "====X====X")}, 8),
    ]
    return items


def _run_writer(tmp_path, items, seed=7, **kw):
    out = stdio.StringIO()
    summary = str(tmp_path / "calls_summary.tsv")
    w = xio.CTCWriter("w", ((c, r) for c, r, _ in items), _Lib(), fd=out, groups=["@RG\tID:run_m"], group_key="m",
                      summary=summary, directory=str(tmp_path), **kw)
    np.random.seed(seed)
    w.start()
    w.join()
    assert w.error is None
    return w, out.getvalue(), summary


def test_writer_counters_arrays_and_order(tmp_path, capfd):
    items = _stream()
    w, sam, summary = _run_writer(tmp_path, items)
    for c, r, want in items:
        assert xio.ctc_verdict(r["sequence"], r["mapping"], _Lib.seq)[0] == want, c.read_id
    assert w.counts == {"count_failed_seq": 1, "count_failed_map": 2, "count_failed_acc": 3, "count_failed_cov": 2,
                        "count_failed_both": 1, "non_ubs_skipped": 0}
    assert [rid for rid, _ in w.log] == [c.read_id for c, _, _ in items] and all(n == 64 for _, n in w.log)
    # the restatement, from the same mappings
    ref_items = []
    for c, r, _ in items:
        m = r["mapping"]
        if m is None:
            v, lab = (3 if not r["sequence"] else 2), []
        else:
            q_al = m.q_st if m.strand == 1 else len(r["sequence"]) - m.q_en
            _, _, v, lab = savectc_ref.row(len(r["sequence"]), 0, m.strand, q_al, q_al + (m.q_en - m.q_st), m.r_st, m.r_en,
                                           b"=" * m.mlen + b"X" * (m.blen - m.mlen), [TEMPLATES[m.ctg]])
        ref_items.append((c.signal, c.read_id, v, lab))
    counts, chunks, refs, lengths, order = savectc_ref.predict(ref_items, 7, 64)
    assert counts == w.counts
    got_chunks, got_refs, got_len = (np.load(tmp_path / n) for n in ("chunks.npy", "references.npy", "reference_lengths.npy"))
    assert got_chunks.dtype == np.float16 and got_refs.dtype == np.uint8 and got_len.dtype == np.uint16
    assert got_chunks.shape == (len(order), 64) and got_refs.shape == (len(order), int(lengths.max())) and got_len.shape == (len(order),)
    assert np.array_equal(got_chunks, chunks) and np.array_equal(got_refs, refs) and np.array_equal(got_len, lengths)
    # label lengths 20, 18, 20, 18: mean 19, sd 1, so all four lie inside mean +- 2.5 sd and typical_indices keeps them
    assert sorted(order) == ["r2:1:1", "r3:1:1", "r4:1:1", "r8:1:1"]
    # labels: strand -1 is the reverse complement with the unnatural position labelled 6, strand +1 labels it 5
    by_id = dict(zip(order, got_refs))
    want = [{"A": 1, "C": 2, "G": 3, "T": 4}.get(c, 6) for c in "ACGNACGTACGTACNTAC"]      # revcomp of tN[2:20]
    assert by_id["r3:1:1"][:18].tolist() == want
    # SAM: the header, then one record per chunk that passed the thresholds, in stream order, without tags
    body = [l for l in sam.split("\n") if l and not l.startswith("@")]
    assert [l.split("\t")[0] for l in body] == ["r2:1:1", "r3:1:1", "r4:1:1", "r8:1:1"]
    assert sam.startswith("@HD") and body[1].split("\t")[1] == "16" and len(body[0].split("\t")) == 13
    # the summary: rewritten in the order of the arrays
    rows = open(summary, newline="").read().split("\r\n")
    assert rows[0].split("\t") == list(xio.SUMMARY_COLUMNS + xio.ALIGNMENT_COLUMNS) and rows[-1] == ""
    assert [l.split("\t")[1] for l in rows[1:-1]] == order
    # filter_stats.csv is pandas.Series.to_csv's text
    assert open(tmp_path / "filter_stats.csv", newline="").read() == savectc_ref.filter_stats_text(counts) == \
        ",0\ncount_failed_seq,1\ncount_failed_map,2\ncount_failed_acc,3\ncount_failed_cov,2\ncount_failed_both,1\nnon_ubs_skipped,0\n"
    err = capfd.readouterr().err
    assert "Filtered reads (failed): 1 seq, 2 map\n" in err and "Filtered reads (failed): 3 acc, 2 cov, 1 both\n" in err
    assert "> written ctc training data\n" in err and "  - chunks.npy with shape (%d,64)\n" % len(order) in err
    assert "Non-UB" not in err


def test_writer_permutation_follows_the_seed(tmp_path):
    """Distinct label lengths (so that typical_indices keeps them), two seeds: arrays and summary move together."""
    S = "ACGTACGTACGTACGTACGT"
    items = [(_chunk(i), {"sequence": S[:20 - i], "qstring": "O" * (20 - i), "mapping": _mapping("tA", S[:20 - i], 1, 0, 0, "=" * (20 - i))}, 0)
             for i in range(8)]
    orders = []
    for seed in (1, 2):
        d = tmp_path / ("s%d" % seed)
        d.mkdir()
        _, _, summary = _run_writer(d, items, seed=seed)
        lengths = np.load(d / "reference_lengths.npy")
        ids = [l.split("\t")[1] for l in open(summary, newline="").read().split("\r\n")[1:-1]]
        np.random.seed(seed)
        want = np.random.permutation(savectc_ref.typical_indices(np.arange(20, 12, -1).astype(np.uint16)))
        assert ids == ["r%d:1:1" % i for i in want] and lengths.tolist() == [20 - i for i in want]
        chunks = np.load(d / "chunks.npy")
        assert all(np.array_equal(chunks[k], items[i][0].signal.astype(np.float16)) for k, i in enumerate(want))
        orders.append(ids)
    assert orders[0] != orders[1] and sorted(orders[0]) == sorted(orders[1])


def test_typical_indices_quirk_equal_lengths_keep_nothing(tmp_path, capfd):
    S = "ACGTACGTACGTACGTACGT"
    items = [(_chunk(i), {"sequence": S, "qstring": "O" * 20, "mapping": _mapping("tA", S, 1, 0, 0, "=" * 20)}, 0) for i in range(3)]
    assert xio.typical_indices(np.array([20, 20, 20], np.uint16)).size == 0
    assert xio.typical_indices(np.array([10, 20, 30, 1000], np.uint16)).tolist() == [0, 1, 2, 3]
    _, sam, summary = _run_writer(tmp_path, items)
    assert np.load(tmp_path / "chunks.npy").shape == (0, 64) and np.load(tmp_path / "references.npy").shape == (0, 20)
    assert len([l for l in sam.split("\n") if l and not l.startswith("@")]) == 3
    assert open(summary, newline="").read().count("\r\n") == 1
    assert "  - reference_lengths.npy shape (0)\n" in capfd.readouterr().err


def test_ub_only_and_device_verdicts(tmp_path, capfd):
    items = _stream()
    w, sam, _ = _run_writer(tmp_path, items, ub_only=True)
    # tA has no unnatural position: its six mapped chunks are skipped before the thresholds are looked at
    assert w.counts == {"count_failed_seq": 1, "count_failed_map": 2, "count_failed_acc": 1, "count_failed_cov": 0,
                        "count_failed_both": 0, "non_ubs_skipped": 6}
    assert [l.split("\t")[0] for l in sam.split("\n") if l and not l.startswith("@")] == ["r3:1:1"]
    assert "Non-UB chunks skipped: 6\n" in capfd.readouterr().err
    # a result that carries the device's verdict and label row is taken at its word
    S = "ACGTACGTACGTACGTACGT"
    m = _mapping("tA", S, 1, 0, 0, "=" * 20)
    dev = [(_chunk(0), {"sequence": S, "qstring": "O" * 20, "mapping": m, "verdict": 0, "target": np.array([1, 2, 5], np.uint8)}, 0),
           (_chunk(1), {"sequence": S, "qstring": "O" * 20, "mapping": None, "verdict": 24, "target": None}, 24),
           (_chunk(2), {"sequence": S, "qstring": "O" * 20, "mapping": m, "verdict": 0, "target": np.array([4, 3, 2, 1], np.uint8)}, 0),
           (_chunk(3), {"sequence": "", "qstring": "", "mapping": None, "verdict": 3, "target": None}, 3),
           (_chunk(4), {"sequence": S, "qstring": "O" * 20, "mapping": m, "verdict": 0, "target": np.array([6, 6, 1, 1, 1], np.uint8)}, 0)]
    d = tmp_path / "dev"
    d.mkdir()
    w, _, _ = _run_writer(d, dev)
    assert w.counts["count_failed_both"] == 1 and w.counts["count_failed_seq"] == 1 and w.counts["count_failed_map"] == 1
    refs, lens = np.load(d / "references.npy"), np.load(d / "reference_lengths.npy")
    assert sorted(lens.tolist()) == [3, 4, 5] and refs.shape == (3, 5)
    assert refs[lens.tolist().index(3)].tolist() == [1, 2, 5, 0, 0]


def test_nothing_kept_writes_nothing(tmp_path, capfd):
    items = _stream()[:2]
    _run_writer(tmp_path, items)
    assert not (tmp_path / "chunks.npy").exists() and not (tmp_path / "filter_stats.csv").exists()
    assert "> no suitable ctc data to write\n" in capfd.readouterr().err


def test_written_directory_loads_and_segments(tmp_path):
    from xna_basecaller_amd.data import load_numpy_datasets
    S = "ACGTACGTACGTACGTACGT"
    items = [(_chunk(i, 200), {"sequence": S[:20 - i], "qstring": "O" * (20 - i), "mapping": _mapping("tN", S[:20 - i], 1, 0, 0, "=" * (20 - i))}, 0)
             for i in range(6)]
    _run_writer(tmp_path, items)
    chunks, targets, lengths = load_numpy_datasets(directory=str(tmp_path))
    assert chunks.shape == (6, 200) and targets.shape == (6, 20) and lengths.shape == (6,)
    assert all((targets[i, :lengths[i]] > 0).all() and (targets[i, lengths[i]:] == 0).all() for i in range(6)) and (targets == 5).any()
    r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "segment", str(tmp_path), "-n"], cwd=ROOT, capture_output=True,
                       text=True, timeout=300)
    assert r.returncode == 0, r.stderr
    bp = np.load(tmp_path / "breakpoints-naive.npy")
    assert bp.shape == targets.shape and all(bp[i, lengths[i] - 1] == 200 for i in range(6))


# ---- the command line's refusals ---------------------------------------------------------------------------------------
def _args(*argv):
    from xna_basecaller_amd.cli.basecaller import argparser
    return argparser().parse_args(["model", "reads", *argv])


def test_refusals():
    from xna_basecaller_amd.cli.basecaller import save_ctc_refusal
    assert save_ctc_refusal(_args("--save-ctc")) == "a reference is needed to output ctc training data"
    for flag in ("--revcomp", "--qscores", "--ub-probs"):
        why = save_ctc_refusal(_args("--save-ctc", "--reference", POC, flag))
        assert why is not None and flag in why and "--save-ctc" in why
    why = save_ctc_refusal(_args("--save-ctc", "--reference", POC, "--paf", "x.paf"))
    assert why is not None and "--paf" in why
    why = save_ctc_refusal(_args("--save-ctc", "--reference", POC), world=2)
    assert why is not None and "WORLD_SIZE" in why and "one GPU" in why
    ok = _args("--save-ctc", "--reference", POC, "--ub-only", "--min-accuracy", "0.9")
    assert save_ctc_refusal(ok) is None and save_ctc_refusal(ok, 1, list("NACGTXY"), b"ACGTNACGT") is None
    assert save_ctc_refusal(ok, 1, list("NACGT"), b"ACGTACGTacgt") is None
    why = save_ctc_refusal(ok, 1, list("NACGT"), b"ACGTNACGT")
    assert why is not None and "5 symbols" in why and "NACGT" in why
    assert save_ctc_refusal(ok, 1, list("NACGTX"), b"ACGTXACGT") is not None


def _config_text(labels):
    return ('[model]\npackage = "bonito.crf"\n[labels]\nlabels = [%s]\n[input]\nfeatures = 1\n[global_norm]\nstate_len = 3\n'
            '[encoder]\nstride = 5\nactivation = "swish"\nfeatures = 64\nwinlen = 19\nscale = 5.0\nrnn_type = "lstm"\nblank_score = 2.0\n'
            '[basecaller]\nbatchsize = 8\nchunksize = 1000\noverlap = 100\n' % ", ".join('"%s"' % c for c in labels))


def _cli(tmp_path, *argv, env=None):
    return subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "basecaller", *argv], cwd=ROOT, capture_output=True, text=True,
                          timeout=300, env=dict(os.environ, **(env or {})))


def test_cli_refuses_before_any_device_work(tmp_path):
    """Every refusal ends the command with status 1 and its message, on a machine without a GPU too."""
    model = tmp_path / "m@v1"
    model.mkdir()
    (model / "config.toml").write_text(_config_text("NACGTXY"))
    reads = tmp_path / "reads"
    reads.mkdir()
    r = _cli(tmp_path, str(model), str(reads), "--save-ctc")
    assert r.returncode == 1 and r.stderr.strip().endswith("> a reference is needed to output ctc training data")
    for extra in (["--revcomp"], ["--qscores"], ["--ub-probs"], ["--paf", str(tmp_path / "o.paf")]):
        r = _cli(tmp_path, str(model), str(reads), "--save-ctc", "--reference", POC, *extra)
        assert r.returncode == 1 and extra[0] in r.stderr and "> error: --save-ctc" in r.stderr, (extra, r.stderr)
    r = _cli(tmp_path, str(model), str(reads), "--save-ctc", "--reference", POC, env={"WORLD_SIZE": "2", "RANK": "0"})
    assert r.returncode == 1 and "WORLD_SIZE is 2" in r.stderr
    four = tmp_path / "four@v1"
    four.mkdir()
    (four / "config.toml").write_text(_config_text("NACGT"))
    r = _cli(tmp_path, str(four), str(reads), "--save-ctc", "--reference", POC)
    assert r.returncode == 1 and "letters outside A, C, G, T" in r.stderr and "only 5 symbols" in r.stderr
    # --modified-bases stays rejected: the flag is still parsed, and its error no longer names --save-ctc
    src = open(os.path.join(ROOT, "xna_basecaller_amd", "cli", "basecaller.py")).read()
    assert '"> error: --modified-bases is not part of the MI355X path\\n"' in src


def test_mutated_reads_reach_every_verdict():
    """The reads of tests/savectc_cases.py, as the GPU test draws them, through the CPU restatements of the mapper and of the
    labels: every verdict bit, verdict 0 on both strands, and 'both' occur -- what the GPU test then asserts of the kernel."""
    import map_ref
    import savectc_cases
    from xna_basecaller_amd.aligner import read_fasta
    templates = [s for _, s in read_fasta(POC)]
    reads = savectc_cases.mutated_reads(templates, 160, np.random.default_rng(17))
    rows, lens = map_ref.pack_rows(reads)
    mapped = map_ref.map_rows(rows, lens, templates)
    plain = savectc_ref.targets(lens, rows.shape[1], mapped, templates)["verdict"]
    ub = savectc_ref.targets(lens, rows.shape[1], mapped, templates, ub_only=True)["verdict"]
    for bit in (1, 2, 8, 16):
        assert (plain & bit).any(), bit
    assert (ub & 4).any() and not (plain & 4).any() and (plain == 24).any() and (plain == 3).any()
    kept = plain == 0
    assert (mapped["strand"][kept] == 1).any() and (mapped["strand"][kept] == -1).any()
