"""GPU: the Viterbi decode with per-base letter probabilities (xb_decode_ub and the calls built on it) -- bit-exact against
the restatement in tests/ubprob_ref.py, the quality decode's bytes unchanged beside them, the fused and pipelined calls, and
`basecaller --ub-probs` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, random_scores
import ubprob_ref
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu

QS, QO = 0.9722, 0.3498          # the shipped model's [qscore] section


def _ctx(nb, T, N, sl=3, features=32):
    return _lib.Context(0, nb, sl, features, 19, 5, 5.0, 2.0, T * 5, N)


def _check(ctx, sc, nb, with_blank, qscale=QS, qoffset=QO):
    alphabet = "NACGTXY"[:nb + 1]
    seq, lens, q, mv, pr = ctx.decode_ub(sc, alphabet, qscale, qoffset, has_blank=with_blank)
    ref = ubprob_ref.decode_ub(sc, nb, alphabet, blank_score=None if with_blank else 2.0, qscale=qscale, qoffset=qoffset)
    bad = np.argwhere(pr != ref["probs"])
    assert not len(bad), "probability mismatches: %d at (chunk, letter, base) %s, got %s want %s" % (
        len(bad), bad[:8].tolist(), pr[tuple(bad[:8].T)].tolist(), ref["probs"][tuple(bad[:8].T)].tolist())
    # everything else is the quality decode's, byte for byte
    qseq, qlens, qq, qmv = ctx.decode_q(sc, alphabet, qscale, qoffset, has_blank=with_blank)
    for a, b in ((seq, qseq), (lens, qlens), (q, qq), (mv, qmv)):
        assert np.array_equal(a, b)
    assert np.array_equal(seq, ref["seq"]) and np.array_equal(lens, ref["seq_len"])
    return seq, lens, q, mv, pr


@pytest.mark.parametrize("nb", [4, 5, 6])
@pytest.mark.parametrize("with_blank", [True, False])
@pytest.mark.parametrize("lps", [0, 1, 2])
def test_decode_ub_bit_exact_random(nb, with_blank, lps, monkeypatch):
    if lps:
        monkeypatch.setenv("XB_DECODE_LPS", str(lps))
    T, N = 203, 5
    ctx = _ctx(nb, T, N)
    _check(ctx, random_scores(T, N, nb, seed=70 + nb, with_blank=with_blank), nb, with_blank)
    ctx.close()


@pytest.mark.parametrize("T", [1, 2, 63, 64, 65, 2000])
def test_decode_ub_lengths(T):
    N = 3 if T < 2000 else 2
    ctx = _ctx(6, max(T, 8), N)
    _check(ctx, random_scores(T, N, 6, seed=T), 6, True)
    _check(ctx, random_scores(T, N, 6, seed=T + 1, with_blank=False), 6, False, qscale=1.0, qoffset=0.0)
    ctx.close()


def test_decode_ub_ties_and_extremes():
    nb, T, N = 6, 50, 4
    S, E = nb ** 3, nb + 1
    ctx = _ctx(nb, T, N)
    _check(ctx, np.zeros((T, N, S * E), np.float32), nb, True)           # every path ties
    sc = random_scores(T, N, nb, seed=1)
    sc[:, 1] = np.round(sc[:, 1])                                        # heavy ties on a coarse grid
    sc[:, 2] *= 8.0                                                      # deep underflow of the posteriors
    sc[:, 3] = -5.0
    sc[:, 3].reshape(T, S, E)[:, :, 0] = 5.0                             # blank dominates: empty call
    seq, lens, q, mv, pr = _check(ctx, sc, nb, True)
    assert lens[3] == 0 and not pr[3].any()
    flat = np.zeros((T, N, S, E), np.float32)
    flat[..., 0] = -1.0
    _check(ctx, flat.reshape(T, N, S * E), nb, True)
    ctx.close()


def test_decode_ub_dev_equals_host_call():
    import torch
    nb, T, N = 6, 300, 7
    ctx = _ctx(nb, T, N)
    sc = random_scores(T, N, nb, seed=3, with_blank=False)
    want = ctx.decode_ub(sc, "NACGTXY", QS, QO, has_blank=False)
    d_sc = torch.from_numpy(sc).cuda()
    outs = [torch.zeros((N, T), dtype=torch.int8, device="cuda"), torch.zeros((N, T), dtype=torch.int8, device="cuda"),
            torch.zeros((N, T), dtype=torch.uint8, device="cuda"), torch.zeros((N, nb, T), dtype=torch.uint8, device="cuda"),
            torch.zeros((N,), dtype=torch.int32, device="cuda")]
    ctx.decode_ub_dev(d_sc.data_ptr(), T, N, False, "NACGTXY", QS, QO, *[o.data_ptr() for o in outs])
    ctx.synchronize()
    got = [o.cpu().numpy() for o in outs]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[4], want[1])
    assert np.array_equal(got[1], want[2]) and np.array_equal(got[2], want[3]) and np.array_equal(got[3], want[4])
    ctx.close()


def _model_ctx(F, nb, L, n, **kw):
    from xna_basecaller_amd.synthetic import seeded_weights
    ctx = _lib.Context(0, nb, 3, F, 19, 5, 5.0, 2.0, L, n, precision=_lib.XB_PREC_MIXED, **kw)
    ctx.load_state_dict(seeded_weights(F, nb))
    return ctx


@pytest.mark.parametrize("F,L,n", [(32, 1000, 9), (768, 2000, 512)])
def test_fused_call_equals_encode_then_decode_ub(F, L, n):
    nb, alphabet = 6, "NACGTXY"
    ctx = _model_ctx(F, nb, L, n)
    x = np.random.default_rng(F + 1).standard_normal((n, L)).astype(np.float32)
    got = ctx.basecall_chunks_ub(x, alphabet, QS, QO)
    scores = ctx.encode(x, expand_blanks=False)
    want = ctx.decode_ub(scores, alphabet, QS, QO, has_blank=False)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    q = ctx.basecall_chunks_q(x, alphabet, QS, QO)                # the quality call's bytes are unchanged
    for g, w in zip(got[:4], q):
        assert np.array_equal(g, w)
    ctx.close()


def _pipeline_run(overlap):
    """Four slots with pairing reserved: _ub batches, then _ub calls that meet plain and _q calls in the pairing window."""
    nb, alphabet, F, L, n = 6, "NACGTXY", 64, 1500, 40
    os.environ["XB_OVERLAP"] = str(overlap)
    try:
        ctx = _model_ctx(F, nb, L, n)
    finally:
        os.environ.pop("XB_OVERLAP")
    rng = np.random.default_rng(8)
    xs = [rng.standard_normal((n - 3 * (i % 2), L)).astype(np.float32) for i in range(6)]
    sync = [ctx.basecall_chunks_ub(x, alphabet, QS, QO) for x in xs]
    plain_sync = [ctx.basecall_chunks(x, alphabet) for x in xs[:2]]
    q_sync = [ctx.basecall_chunks_q(x, alphabet, QS, QO) for x in xs[:3]]
    assert ctx.reserve_pairing() in (True, False)
    got, pending = [], []
    for i, x in enumerate(xs):
        slot = i % _lib.XB_PIPELINE_SLOTS
        pending.append((slot, ctx.submit_chunks_ub(slot, x, alphabet, QS, QO)))
        if len(pending) == _lib.XB_PIPELINE_SLOTS:
            got.append(ctx.collect_chunks_ub(*pending.pop(0)))
    while pending:
        got.append(ctx.collect_chunks_ub(*pending.pop(0)))
    for g, w in zip(got, sync):
        for a, b in zip(g, w):
            assert np.array_equal(a, b)
    # _ub interleaved with plain and _q calls: each gives its unpaired bytes
    ctx.submit_chunks(0, xs[0], alphabet)
    ctx.submit_chunks_ub(1, xs[1], alphabet, QS, QO)
    ctx.submit_chunks_q(2, xs[2], alphabet, QS, QO)
    ctx.submit_chunks_ub(3, xs[3], alphabet, QS, QO)
    p0 = ctx.collect_chunks(0, len(xs[0]))
    u1 = ctx.collect_chunks_ub(1, len(xs[1]))
    q2 = ctx.collect_chunks_q(2, len(xs[2]))
    u3 = ctx.collect_chunks_ub(3, len(xs[3]))
    assert np.array_equal(p0[0], plain_sync[0][0]) and np.array_equal(p0[1], plain_sync[0][1])
    for g, w in ((u1, sync[1]), (q2, q_sync[2]), (u3, sync[3])):
        for a, b in zip(g, w):
            assert np.array_equal(a, b)
    # two _ub calls of different calibrations do not share a pass
    ctx.submit_chunks_ub(0, xs[4], alphabet, 1.0, 0.0)
    ctx.submit_chunks_ub(1, xs[5], alphabet, QS, QO)
    other = ctx.collect_chunks_ub(0, len(xs[4]))
    u5 = ctx.collect_chunks_ub(1, len(xs[5]))
    for a, b in zip(u5, sync[5]):
        assert np.array_equal(a, b)
    assert np.array_equal(other[0], sync[4][0]) and np.array_equal(other[4], sync[4][4])
    with pytest.raises(_lib.XbError):                   # a _q submission has no letter probabilities to collect
        ctx.submit_chunks_q(0, xs[0], alphabet, QS, QO)
        try:
            ctx.collect_chunks_ub(0, len(xs[0]))
        finally:
            ctx.collect_chunks_q(0, len(xs[0]))
    ctx.close()
    return sync


def test_pipelined_ub_calls_equal_the_synchronous_call():
    a = _pipeline_run(1)
    b = _pipeline_run(0)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)


def test_cli_ub_probs_end_to_end_through_fast5(tmp_path):
    """`basecaller --ub-probs` on a NACGTXY model through multi-read fast5: the sequences of a run without the flag, the
    qualities of a --qscores run, and uX / uY tags whose values are the Python composition of Model.decode_ub rows -- in
    FASTQ and in SAM."""
    from h5write import write_multi_fast5
    from test_gpu_cli import _make_model_dir
    from xna_basecaller_amd import reads as xreads
    from xna_basecaller_amd import util
    from xna_basecaller_amd.crf.basecall import to_str
    from xna_basecaller_amd import toml_lite
    labels = list("NACGTXY")
    model_dir = str(tmp_path / "xna_test@v1")
    cfg, _ = _make_model_dir(model_dir, 64, labels, seed=22)
    cfg["encoder"]["scale"] = 1.5                     # flatter scores: probabilities away from 0 / 255
    cfg["encoder"]["blank_score"] = 0.5
    with open(os.path.join(model_dir, "config.toml"), "w") as fh:
        fh.write(toml_lite.dumps(cfg))
    rng = np.random.default_rng(17)
    recs = []
    for i in range(8):
        length = int(rng.integers(3000, 12000))
        base = rng.normal(90.0, 12.0, length)
        base[: int(rng.integers(300, 900))] = 140.0
        recs.append((np.round(base * 8.0).astype(np.int16),
                     dict(read_id="uuuu-%02d" % i, range=1443.03, digitisation=8192.0, offset=10, sampling_rate=4000.0,
                          run_id="runU", channel_number=str(100 + i), start_mux=1 + i % 4, read_number=i,
                          start_time=4000 * i, duration=length, exp_start_time="2021-06-01T10:00:00Z")))
    f5 = tmp_path / "f5"
    f5.mkdir()
    write_multi_fast5(str(f5 / "batch_0.fast5"), recs, vbz=True)
    batch = 6
    runs = {"plain": ([], "fastq"), "q": (["--qscores"], "fastq"), "ub": (["--ub-probs"], "fastq"),
            "ubq": (["--ub-probs", "--qscores"], "fastq"), "ubsam": (["--ub-probs", "--qscores"], "sam")}
    outs = {}
    for name, (flags, ext) in runs.items():
        out = tmp_path / ("calls_%s.%s" % (name, ext))
        with open(out, "w") as fh:
            r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "basecaller", model_dir, str(f5), "--batch",
                                str(batch)] + flags, cwd=ROOT, stdout=fh, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()
        outs[name] = out.read_text().strip().split("\n")
    plain, q = outs["plain"], outs["q"]
    assert len(plain) == 4 * 8

    # the Python composition: chunks in the CLI's batches -> scores -> xb_decode_ub rows -> the reference's stitch per plane
    model = util.load_model(model_dir, "cuda:0", chunksize=4000, overlap=500, batchsize=batch)
    reads = list(xreads.get_reads(str(f5)))
    chunks = (((rd, 0, len(rd.signal)), util.chunk(np.asarray(rd.signal, np.float32), 4000, 500)) for rd in reads)
    rows = []
    for keys, b in util.batchify(chunks, batchsize=batch):
        seq, _, _, _, pr = model.decode_ub(model(b))
        rows.append((keys, {"sequence": seq, "x": np.ascontiguousarray(pr[:, 4]), "y": np.ascontiguousarray(pr[:, 5])}))
    expect = {}
    for (rd, s, e), res in util.unbatchify(iter(rows)):
        st = util.stitch(res, 4000, 500, e - s, model.stride)
        called = st["sequence"] != 0
        expect[rd.read_id] = (to_str(st["sequence"]),
                              ["uX:B:C," + ",".join(map(str, st["x"][called].tolist())),
                               "uY:B:C," + ",".join(map(str, st["y"][called].tolist()))])

    def check_fastq(lines, quals):
        assert lines[1::4] == plain[1::4]                              # sequences byte-equal
        assert lines[3::4] == quals[3::4]                              # qualities byte-equal
        for hdr, seq in zip(lines[0::4], lines[1::4]):
            fields = hdr[1:].split("\t")
            rid = fields[0].split(" ")[0]
            tags = fields[-2:]
            assert [t[:7] for t in tags] == ["uX:B:C,", "uY:B:C,"]
            assert all(len(t[7:].split(",")) == len(seq) for t in tags)
            assert (seq, tags) == expect[rid]

    check_fastq(outs["ub"], plain)
    check_fastq(outs["ubq"], q)
    sam = [l for l in outs["ubsam"] if not l.startswith("@")]
    assert len(sam) == 8
    by_id = {l.split("\t")[0]: l.split("\t") for l in sam}
    for hdr, seq, qual in zip(outs["ubq"][0::4], outs["ubq"][1::4], outs["ubq"][3::4]):
        rid = hdr[1:].split(" ")[0].split("\t")[0]
        rec = by_id[rid]
        assert rec[9] == seq and rec[10] == qual and rec[-2:] == expect[rid][1]
    assert sum(len(s) for s in plain[1::4]) > 1000
    # the probabilities carry information: not every byte is 0 or 255
    vals = np.concatenate([np.array(t[7:].split(","), int) for tags in (v[1] for v in expect.values()) for t in tags])
    assert 0 < np.mean((vals > 0) & (vals < 255))
