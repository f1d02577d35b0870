"""GPU: `basecaller --save-ctc` on the device -- xb_ctc_targets (host and _dev forms) bit-equal to the CPU restatement of its
contract (tests/savectc_ref.py) over the device mapper's outputs, its edge cases, the fused xb_ctc_chunks against the three
host-form calls, and the command line end to end on both decode branches.  minimap2 is in no image: parity unpinned, the
contract is the header's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import map_ref
import savectc_cases
import savectc_ref
from conftest import GOLDEN, ROOT, make_config

pytestmark = pytest.mark.gpu

POC = os.path.join(GOLDEN, "poc_refdb_short.fasta")
OUT = ("mlen", "blen", "verdict", "target", "target_len")
LENIENT = (3, 1, 1, 1, 1)           # match, mismatch, gap_open, gap_extend, ambiguous: long, inexact alignments of arbitrary calls
MAPPED = ("tmpl", "strand", "score", "second", "q_st", "q_en", "r_st", "r_en", "ops", "n_ops")


def _ctx(max_batch=4, chunk_len=1000, weights=False):
    from xna_basecaller_amd import _lib
    _lib.require_gpu()
    ctx = _lib.Context(0, 6, 3, 64, 19, 5, 5.0, 2.0, chunk_len, max_batch)
    if weights:           # seeded weights whose calls follow the signal (the plain seeded ones call the same thing for every chunk)
        from xna_basecaller_amd.synthetic import peaky_weights
        ctx.load_state_dict(peaky_weights(64, 6, 5))
    return ctx


def _library(templates):
    off = np.zeros(len(templates) + 1, np.int32)
    off[1:] = np.cumsum([len(t) for t in templates])
    return "".join(templates).encode("ascii"), off


def _poc():
    from xna_basecaller_amd.aligner import read_fasta
    return [s for _, s in read_fasta(POC)]


def _equal(got, want, what=""):
    for k in OUT:
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (what, k, got[k].shape, want[k].shape)
        bad = np.flatnonzero((got[k] != want[k]).reshape(len(want[k]), -1).any(axis=1))
        assert bad.size == 0, (what, k, bad[:5], got[k][bad[:2]], want[k][bad[:2]])


def _check(ctx, reads, templates, **rule):
    """Reads through the device mapper, then the labels on the device against the restatement over the same mapper outputs."""
    rows, lens = map_ref.pack_rows(reads)
    lib, off = _library(templates)
    mapped = ctx.map_templates(rows, lens, lib, off)
    got = ctx.ctc_targets(lens, rows.shape[1], mapped, lib, off, **rule)
    want = savectc_ref.targets(lens, rows.shape[1], mapped, templates, **rule)
    print("verdicts", rule, np.unique(got["verdict"], return_counts=True))
    _equal(got, want, rule)
    return mapped, got


def test_kernel_against_the_restatement_both_forms():
    import torch
    ctx = _ctx()
    templates = _poc()
    reads = savectc_cases.mutated_reads(templates, 160, np.random.default_rng(17))
    mapped, plain = _check(ctx, reads, templates)
    _, ub = _check(ctx, reads, templates, ub_only=True)
    _check(ctx, reads, templates, min_accuracy=0.9, min_coverage=0.5, ub_plus=7, ub_minus=9)
    v = plain["verdict"]
    for bit in (1, 2, 8, 16):
        assert (v & bit).any(), bit
    assert (ub["verdict"] & 4).any() and (v == 0).any() and (v == 24).any() and (v == 3).any()
    kept = v == 0
    assert (mapped["strand"][kept] == 1).any() and (mapped["strand"][kept] == -1).any()
    assert (plain["target"] == 5).any() and (plain["target"] == 6).any() and plain["target"].max() == 6
    # the mapper's own mlen: the '=' columns
    assert np.array_equal(plain["mlen"], (mapped["ops"] == ord("=")).sum(axis=1)) and np.array_equal(plain["blen"], mapped["n_ops"])
    # the _dev form on device copies of the same rows
    rows, lens = map_ref.pack_rows(reads)
    lib, off = _library(templates)
    dev = torch.device("cuda:0")
    d_len = torch.from_numpy(lens).to(dev)
    d_in = {k: torch.from_numpy(mapped[k]).to(dev) for k in ctx.CTC_INPUTS}
    d_out = {k: torch.full(plain[k].shape, 77, dtype=getattr(torch, str(plain[k].dtype)), device=dev) for k in OUT}
    torch.cuda.synchronize()
    ctx.ctc_targets_dev(d_len.data_ptr(), len(reads), rows.shape[1], {k: t.data_ptr() for k, t in d_in.items()}, lib, off,
                        {k: t.data_ptr() for k, t in d_out.items()}, ub_only=True)
    ctx.synchronize()
    _equal({k: t.cpu().numpy() for k, t in d_out.items()}, ub, "_dev")
    ctx.close()


def test_edge_cases():
    ctx = _ctx()
    # thresholds exactly on a quotient: 19 / 20 and 18 / 20 are not below themselves, and are below the next float up
    t20 = "ACGGTCATTGCAAGCTTGCA"
    reads = [t20[:10] + "A" + t20[11:], t20, "GG" + t20[:18]]        # t20[10] is C
    for acc, cov in ((19 / 20, 18 / 20), (np.nextafter(19 / 20, 1), 18 / 20), (19 / 20, np.nextafter(18 / 20, 1)), (0.95, 0.90)):
        mapped, got = _check(ctx, reads, [t20], min_accuracy=acc, min_coverage=cov)
        assert mapped["n_ops"].tolist() == [20, 20, 18] and got["mlen"].tolist() == [19, 20, 18]
    mapped, got = _check(ctx, reads, [t20], min_accuracy=19 / 20, min_coverage=18 / 20)
    assert got["verdict"].tolist() == [0, 0, 0]
    _, got = _check(ctx, reads, [t20], min_accuracy=np.nextafter(19 / 20, 1), min_coverage=np.nextafter(18 / 20, 1))
    assert got["verdict"].tolist() == [8, 0, 16]
    # ub_only on templates without N, and on a slice that misses the template's N
    _, got = _check(ctx, [t20, "ACGTTGCAGGCATCAG"], [t20, "ACGTTGCAGGCATCAGNNTT"], ub_only=True)
    assert got["verdict"].tolist() == [4, 4]
    _, got = _check(ctx, ["ACGTTGCAGGCATCAGXXTT"], [t20, "ACGTTGCAGGCATCAGNNTT"], ub_only=True, min_accuracy=0.5)
    assert got["verdict"].tolist() == [0] and got["target"][0, :20].tolist() == [1, 2, 3, 4, 4, 3, 2, 1, 3, 3, 2, 1, 4, 2, 1, 3, 5, 5, 4, 4]
    # empty rows and unmapped all-ambiguous rows: bits 0 and 1, bit 1
    _, got = _check(ctx, ["", "NNNNNNNN", "XYXYXY", t20, ""], [t20])
    assert got["verdict"].tolist() == [3, 2, 2, 0, 3] and not got["target"][[0, 1, 2, 4]].any()
    # lowercase templates, other non-ACGT bytes, the reverse strand's labels
    low = "acggtcatnrgcaagcttgca"
    called = low.upper().replace("N", "X").replace("R", "X")
    mapped, got = _check(ctx, [called, savectc_cases.revcomp(called)], [low], min_accuracy=0.8, min_coverage=0.8)
    assert got["verdict"].tolist() == [0, 0] and mapped["strand"].tolist() == [1, -1] and got["target_len"].tolist() == [21, 21]
    assert got["target"][0, :21].tolist() == [{"a": 1, "c": 2, "g": 3, "t": 4}.get(c, 5) for c in low]
    assert got["target"][1, :21].tolist() == [{"a": 4, "c": 3, "g": 2, "t": 1}.get(c, 6) for c in reversed(low)]
    # a 4096-letter template: every stripe of the label row, both strands, slices at unaligned offsets
    rng = np.random.default_rng(2)
    long_t = "".join(rng.choice(np.array(list("ACGTN")), 4096, p=[0.24, 0.24, 0.24, 0.24, 0.04]))
    long_t = "AC" + long_t[2:-2] + "GT"
    called = long_t.replace("N", "X")
    reads = [called, savectc_cases.revcomp(called), called[1:4095], called[1037:3001], savectc_cases.revcomp(called[3:2050]), called[4000:]]
    mapped, got = _check(ctx, reads, [long_t, t20], min_accuracy=0.9, min_coverage=0.9)
    assert got["verdict"].tolist() == [0] * 6 and got["target_len"].tolist()[:2] == [4096, 4096]
    assert all(len(r) - 2 <= n <= len(r) for r, n in zip(reads, got["target_len"].tolist()))     # an X at an end is clipped
    assert got["target"].shape == (6, 4096) and mapped["strand"].tolist() == [1, -1, 1, 1, -1, 1]
    ctx.close()


def test_fused_call_equals_the_three_host_calls():
    """xb_ctc_chunks at a batch the mapper's cell budget splits (300 rows of 200 steps against 1,024,000 letters: 292 + 8)."""
    ctx = _ctx(max_batch=300, chunk_len=1000, weights=True)
    rng = np.random.default_rng(9)
    templates = ["".join(rng.choice(np.array(list("ACGTN")), 4000, p=[0.245, 0.245, 0.245, 0.245, 0.02])) for _ in range(256)]
    lib, off = _library(templates)
    assert 2.0 * 300 * ctx.T * len(lib) > 1.2e11 > 2.0 * 150 * ctx.T * len(lib)
    signal = rng.standard_normal((300, 1000)).astype(np.float32)
    alphabet = list("NACGTXY")
    seq, lens = ctx.basecall_chunks(signal, alphabet)
    assert len({seq[r, :lens[r]].tobytes() for r in range(300)}) > 250
    # the calls of seeded weights are arbitrary: under map-ont's scores they share a dozen exact letters with some template and
    # accuracy is 1 everywhere; lenient scores make the alignments long and inexact, each row with quotients of its own
    parts = [ctx.map_templates(seq[a:b], lens[a:b], lib, off, LENIENT) for a, b in ((0, 150), (150, 300))]
    mapped = {k: np.concatenate([p[k] for p in parts]) for k in MAPPED}
    hit = np.flatnonzero(mapped["tmpl"] >= 0)
    assert hit.size > 250
    # thresholds at the medians of the rows' own quotients: kept and dropped rows both occur, whatever the seeded weights call
    quot = [savectc_ref.quotients(int(lens[r]), int(mapped["q_st"][r]), int(mapped["q_en"][r]),
                                  int((mapped["ops"][r] == ord("=")).sum()), int(mapped["n_ops"][r])) for r in hit]
    rule = dict(min_coverage=float(np.median([c for c, _ in quot])), min_accuracy=float(np.median([a for _, a in quot])), ub_only=False)
    fused = ctx.ctc_chunks(signal, alphabet, lib, off, LENIENT, **rule)
    assert np.array_equal(fused["seq"], seq) and np.array_equal(fused["seq_len"], lens)
    for k in MAPPED:
        assert np.array_equal(fused[k], mapped[k]), k
    labels = ctx.ctc_targets(lens, ctx.T, mapped, lib, off, **rule)
    _equal({k: fused[k] for k in OUT}, labels, "fused")
    _equal(labels, savectc_ref.targets(lens, ctx.T, mapped, templates, **rule), "restatement")
    print("fused verdicts", rule, np.unique(fused["verdict"], return_counts=True))
    assert (fused["verdict"] == 0).any() and (fused["verdict"] != 0).any()
    ctx.close()


# ---- the command line --------------------------------------------------------------------------------------------------
def _write_reads(reads_dir, count, seed):
    from xna_basecaller_amd import reads as xreads
    rng = np.random.default_rng(seed)
    recs = []
    for i in range(count):
        length = int(rng.integers(3000, 14000))
        raw = np.round(rng.normal(90.0, 12.0, length) * 8.0).astype(np.int16)
        recs.append((raw, dict(read_id="read-%02d" % i, range=1443.03, digitisation=8192.0, offset=10, sampling_rate=4000.0,
                               run_id="runX", channel_number=str(100 + i), start_mux=1 + i % 4, read_number=i,
                               start_time=4000 * i, duration=length, exp_start_time="2021-06-01T10:00:00Z")))
    os.makedirs(reads_dir)
    xreads.write_bundle(os.path.join(reads_dir, "batch0.xsig.npz"), recs)


def _predict(model_dir, reads_dir, reference, seed):
    """Every chunk's (signal, id, cov, acc, mapping) through the package's `basecall` and TemplateAligner.map -- the path a user
    had before --save-ctc -- with the quotients and labels from the restatement."""
    from xna_basecaller_amd import reads as xreads
    from xna_basecaller_amd import util
    from xna_basecaller_amd.aligner import TemplateAligner
    from xna_basecaller_amd.crf.basecall import basecall
    model = util.load_model(model_dir, "cuda", weights=0, batchsize=7, use_koi=True)      # the command line's defaults
    assert bool(model.encoder[-1].expand_blanks) == (len(model.alphabet) != 5)                 # 4 bases: the beam search
    run = model.config["basecaller"]
    chunks = [c for read in xreads.get_reads(reads_dir, n_proc=1) for c in xreads.read_chunks(read, run["chunksize"], run["overlap"])]
    called = list(basecall(model, chunks, chunksize=run["chunksize"], overlap=run["overlap"], batchsize=7))
    aligner = TemplateAligner.from_config(reference, model.config, context=lambda: model._ctx)
    mappings = aligner.map([res["sequence"] for _, res in called])
    templates = dict(zip(aligner.names, aligner.templates))
    model._drop_context()
    rows = []
    for (chunk, res), m in zip(called, mappings):
        seq = res["sequence"]
        cov = acc = None
        if seq and m is not None:
            cov, acc = savectc_ref.quotients(len(seq), m.q_st, m.q_en, m.mlen, m.blen)
        rows.append((chunk, seq, m, cov, acc))
    return rows, templates


def _make_model_dir(path, labels, seed):
    """config.toml (with lenient [aligner] scores: every chunk gets quotients of its own) and a checkpoint of seeded weights
    whose calls follow the signal, under the training-time key names as tests/test_gpu_cli.py writes them."""
    import torch
    from test_gpu_cli import TRAIN_INDEX
    from xna_basecaller_amd import toml_lite
    from xna_basecaller_amd.synthetic import peaky_weights
    cfg = make_config(64, labels)
    cfg["model"]["package"] = "bonito.crf"
    cfg["basecaller"] = {"batchsize": 5, "chunksize": 4000, "overlap": 500}
    cfg["aligner"] = dict(zip(("match", "mismatch", "gap_open", "gap_extend", "ambiguous"), LENIENT))
    os.makedirs(path)
    with open(os.path.join(path, "config.toml"), "w") as fh:
        fh.write(toml_lite.dumps(cfg))
    train = {}
    for k, v in peaky_weights(64, len(labels) - 1, seed).items():
        idx = int(k.split(".")[1])
        train["module." + k.replace("encoder.%d." % idx, "encoder.%d." % TRAIN_INDEX[idx])] = torch.from_numpy(v)
    torch.save(train, os.path.join(path, "weights_1.tar"))


def _cli_case(tmp_path, labels, reference, seed):
    model_dir, reads_dir = str(tmp_path / "xna_ctc@v1"), str(tmp_path / "reads")
    _make_model_dir(model_dir, labels, seed=21)
    _write_reads(reads_dir, 10, seed)
    rows, templates = _predict(model_dir, reads_dir, reference, seed)
    covs = [c for _, _, _, c, _ in rows if c is not None]
    accs = [a for _, _, _, _, a in rows if a is not None]
    assert len(covs) >= 8
    min_cov, min_acc = float(np.median(covs)), float(np.median(accs))
    items = []
    for chunk, seq, m, cov, acc in rows:
        if m is None or not seq:
            verdict, lab = (1 if not seq else 0) | (2 if m is None else 0), []
        else:
            q_al = m.q_st if m.strand == 1 else len(seq) - m.q_en
            _, _, verdict, lab = savectc_ref.row(len(seq), 0, m.strand, q_al, q_al + m.q_en - m.q_st, m.r_st, m.r_en,
                                                 b"=" * m.mlen + b"X" * (m.blen - m.mlen), [templates[m.ctg]],
                                                 min_accuracy=min_acc, min_coverage=min_cov)
        items.append((np.asarray(chunk.signal), chunk.read_id, verdict, lab))
    counts, chunks, refs, lengths, order = savectc_ref.predict(items, 25, 4000)
    kept = sum(1 for it in items if it[2] == 0)
    print("chunks", len(items), "kept", kept, "thresholds", repr(min_cov), repr(min_acc), counts)
    assert 0 < kept < len(items)                      # the medians leave both kinds, by construction
    out_dir = tmp_path / "out"
    out_dir.mkdir()
    sam = out_dir / "calls.sam"
    with open(sam, "w") as fh:
        r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "basecaller", model_dir, reads_dir, "--batch", "7",
                            "--save-ctc", "--reference", reference, "--min-coverage", repr(min_cov), "--min-accuracy", repr(min_acc)],
                           cwd=ROOT, stdout=fh, stderr=subprocess.PIPE, timeout=900)
    err = r.stderr.decode()
    assert r.returncode == 0, err
    assert "> writer_kwargs: {'min_coverage': %r, 'min_accuracy': %r, 'ub_only': False}" % (min_cov, min_acc) in err
    assert "> completed reads: %d\n" % len(items) in err and "> written ctc training data" in err
    assert np.array_equal(np.load(out_dir / "chunks.npy"), chunks)
    assert np.array_equal(np.load(out_dir / "references.npy"), refs)
    assert np.array_equal(np.load(out_dir / "reference_lengths.npy"), lengths)
    assert (out_dir / "filter_stats.csv").read_text() == savectc_ref.filter_stats_text(counts)
    body = [l for l in sam.read_text().split("\n") if l and not l.startswith("@")]
    assert [l.split("\t")[0] for l in body] == [it[1] for it in items if it[2] == 0]
    summary = (out_dir / "calls_summary.tsv").read_bytes().decode().split("\r\n")
    assert [l.split("\t")[1] for l in summary[1:-1]] == order and len(summary[0].split("\t")) == 27
    return refs


def test_cli_end_to_end_viterbi(tmp_path):
    refs = _cli_case(tmp_path, list("NACGTXY"), POC, seed=4)
    assert (refs <= 6).all()


def test_cli_end_to_end_beam(tmp_path):
    """A 4-base model takes the beam search: the host forms of the mapper and of the labels.  Its library has no N."""
    from xna_basecaller_amd.aligner import read_fasta
    natural = tmp_path / "natural.fasta"
    natural.write_text("".join(">%s\n%s\n" % (n, s.replace("N", "A")) for n, s in read_fasta(POC)))
    refs = _cli_case(tmp_path, list("NACGT"), str(natural), seed=6)
    assert (refs <= 4).all()          # (typical_indices may keep nothing: a few chunks whose label rows are equally long)
