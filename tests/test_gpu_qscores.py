"""GPU: the Viterbi decode with qualities (xb_decode_q and the calls built on it) -- bit-exact against the restatement in
tests/qscore_ref.py, unchanged bases, the fused and pipelined calls, and `basecaller --qscores` end to end."""
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT, random_scores
import qscore_ref
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu

QS, QO = 0.9722, 0.3498          # the shipped model's [qscore] section


def _ctx(nb, T, N, sl=3, features=32):
    return _lib.Context(0, nb, sl, features, 19, 5, 5.0, 2.0, T * 5, N)


def _check(ctx, sc, nb, with_blank, qscale=QS, qoffset=QO):
    alphabet = "NACGTXY"[:nb + 1]
    seq, lens, q, mv = ctx.decode_q(sc, alphabet, qscale, qoffset, has_blank=with_blank)
    ref = qscore_ref.decode_q(sc, nb, alphabet, blank_score=None if with_blank else 2.0, qscale=qscale, qoffset=qoffset)
    assert np.array_equal(mv, ref["moves"]), np.argwhere(mv != ref["moves"])[:8].tolist()
    bad = np.argwhere(q != ref["qstring"])
    assert not len(bad), "quality mismatches: %d at (chunk, base) %s, got %s want %s" % (
        len(bad), bad[:8].tolist(), q[tuple(bad[:8].T)].tolist(), ref["qstring"][tuple(bad[:8].T)].tolist())
    # the bases are the plain decode's, byte for byte, and the moves are its labels != 0
    pseq, plens, labels = ctx.decode(sc, alphabet, has_blank=with_blank, want_labels=True)
    assert np.array_equal(seq, pseq) and np.array_equal(lens, plens)
    assert np.array_equal(mv, (labels != 0).astype(np.uint8))
    assert np.array_equal((q != 0).sum(axis=1), lens)
    return seq, lens, q, mv


@pytest.mark.parametrize("nb", [4, 5, 6])
@pytest.mark.parametrize("with_blank", [True, False])
@pytest.mark.parametrize("lps", [0, 1, 2])
def test_decode_q_bit_exact_random(nb, with_blank, lps, monkeypatch):
    if lps:
        monkeypatch.setenv("XB_DECODE_LPS", str(lps))
    T, N = 203, 5
    ctx = _ctx(nb, T, N)
    _check(ctx, random_scores(T, N, nb, seed=60 + nb, with_blank=with_blank), nb, with_blank)
    ctx.close()


@pytest.mark.parametrize("T", [1, 2, 3, 5, 8, 203, 2000])
def test_decode_q_lengths(T):
    N = 3 if T < 2000 else 2
    ctx = _ctx(6, max(T, 8), N)
    _check(ctx, random_scores(T, N, 6, seed=T), 6, True)
    _check(ctx, random_scores(T, N, 6, seed=T + 1, with_blank=False), 6, False, qscale=1.0, qoffset=0.0)
    ctx.close()


def test_decode_q_ties_and_extremes():
    nb, T, N = 6, 50, 4
    S, E = nb ** 3, nb + 1
    ctx = _ctx(nb, T, N)
    _check(ctx, np.zeros((T, N, S * E), np.float32), nb, True)           # every path ties
    sc = random_scores(T, N, nb, seed=1)
    sc[:, 1] = np.round(sc[:, 1])                                        # heavy ties on a coarse grid
    sc[:, 2] *= 8.0                                                      # deep underflow of the posteriors
    sc[:, 3] = -5.0
    sc[:, 3].reshape(T, S, E)[:, :, 0] = 5.0                             # blank dominates: empty call
    seq, lens, q, mv = _check(ctx, sc, nb, True)
    assert lens[3] == 0 and not q[3].any() and not mv[3].any()
    flat = np.zeros((T, N, S, E), np.float32)
    flat[..., 0] = -1.0
    _check(ctx, flat.reshape(T, N, S * E), nb, True)
    ctx.close()


def test_decode_q_random_shapes():
    rng = np.random.default_rng(2024)
    for i in range(20):
        nb = int(rng.integers(4, 7))
        T, N = int(rng.integers(1, 300)), int(rng.integers(1, 9))
        with_blank = bool(rng.integers(2))
        qs, qo = float(rng.uniform(0.5, 1.5)), float(rng.uniform(-2, 2))
        ctx = _ctx(nb, T + int(rng.integers(0, 20)), N)
        _check(ctx, random_scores(T, N, nb, seed=100 + i, with_blank=with_blank), nb, with_blank, qs, qo)
        ctx.close()


def test_decode_q_dev_equals_host_call():
    import torch
    nb, T, N = 6, 300, 7
    ctx = _ctx(nb, T, N)
    sc = random_scores(T, N, nb, seed=3, with_blank=False)
    want = ctx.decode_q(sc, "NACGTXY", QS, QO, has_blank=False)
    d_sc = torch.from_numpy(sc).cuda()
    outs = [torch.zeros((N, T), dtype=torch.int8, device="cuda"), torch.zeros((N, T), dtype=torch.int8, device="cuda"),
            torch.zeros((N, T), dtype=torch.uint8, device="cuda"), torch.zeros((N,), dtype=torch.int32, device="cuda")]
    ctx.decode_q_dev(d_sc.data_ptr(), T, N, False, "NACGTXY", QS, QO, outs[0].data_ptr(), outs[1].data_ptr(),
                     outs[2].data_ptr(), outs[3].data_ptr())
    ctx.synchronize()
    got = [o.cpu().numpy() for o in outs]
    assert np.array_equal(got[0], want[0]) and np.array_equal(got[3], want[1])
    assert np.array_equal(got[1], want[2]) and np.array_equal(got[2], want[3])
    ctx.close()


def _model_ctx(F, nb, L, n, **kw):
    from xna_basecaller_amd.synthetic import seeded_weights
    ctx = _lib.Context(0, nb, 3, F, 19, 5, 5.0, 2.0, L, n, precision=_lib.XB_PREC_MIXED, **kw)
    ctx.load_state_dict(seeded_weights(F, nb))
    return ctx


@pytest.mark.parametrize("F,L,n", [(32, 1000, 9), (768, 2000, 512)])
def test_fused_call_equals_encode_then_decode_q(F, L, n):
    nb, alphabet = 6, "NACGTXY"
    ctx = _model_ctx(F, nb, L, n)
    x = np.random.default_rng(F).standard_normal((n, L)).astype(np.float32)
    got = ctx.basecall_chunks_q(x, alphabet, QS, QO)
    scores = ctx.encode(x, expand_blanks=False)
    want = ctx.decode_q(scores, alphabet, QS, QO, has_blank=False)
    for g, w in zip(got, want):
        assert np.array_equal(g, w)
    seq, lens = ctx.basecall_chunks(x, alphabet)                 # the plain call's bytes are unchanged
    assert np.array_equal(seq, got[0]) and np.array_equal(lens, got[1])
    ctx.close()


def _pipeline_run(overlap):
    """Four slots with pairing reserved: _q batches, then a plain and a _q call that meet in the pairing window."""
    nb, alphabet, F, L, n = 6, "NACGTXY", 64, 1500, 40
    os.environ["XB_OVERLAP"] = str(overlap)
    try:
        ctx = _model_ctx(F, nb, L, n)
    finally:
        os.environ.pop("XB_OVERLAP")
    rng = np.random.default_rng(7)
    xs = [rng.standard_normal((n - 3 * (i % 2), L)).astype(np.float32) for i in range(6)]
    sync = [ctx.basecall_chunks_q(x, alphabet, QS, QO) for x in xs]
    plain_sync = [ctx.basecall_chunks(x, alphabet) for x in xs[:2]]
    assert ctx.reserve_pairing() in (True, False)
    got, pending = [], []
    for i, x in enumerate(xs):
        slot = i % _lib.XB_PIPELINE_SLOTS
        pending.append((slot, ctx.submit_chunks_q(slot, x, alphabet, QS, QO)))
        if len(pending) == _lib.XB_PIPELINE_SLOTS:
            got.append(ctx.collect_chunks_q(*pending.pop(0)))
    while pending:
        got.append(ctx.collect_chunks_q(*pending.pop(0)))
    for g, w in zip(got, sync):
        for a, b in zip(g, w):
            assert np.array_equal(a, b)
    # a plain call held for a partner and a _q call after it: each gives its unpaired bytes
    ctx.submit_chunks(0, xs[0], alphabet)
    ctx.submit_chunks_q(1, xs[1], alphabet, QS, QO)
    p0 = ctx.collect_chunks(0, len(xs[0]))
    q1 = ctx.collect_chunks_q(1, len(xs[1]))
    assert np.array_equal(p0[0], plain_sync[0][0]) and np.array_equal(p0[1], plain_sync[0][1])
    for a, b in zip(q1, sync[1]):
        assert np.array_equal(a, b)
    # two _q calls of different calibrations do not share a pass either
    ctx.submit_chunks_q(2, xs[2], alphabet, 1.0, 0.0)
    ctx.submit_chunks_q(3, xs[3], alphabet, QS, QO)
    other = ctx.collect_chunks_q(2, len(xs[2]))
    q3 = ctx.collect_chunks_q(3, len(xs[3]))
    for a, b in zip(q3, sync[3]):
        assert np.array_equal(a, b)
    assert np.array_equal(other[0], sync[2][0])
    with pytest.raises(_lib.XbError):                   # a plain submission has no qualities to collect
        ctx.submit_chunks(0, xs[0], alphabet)
        try:
            ctx.collect_chunks_q(0, len(xs[0]))
        finally:
            ctx.collect_chunks(0, len(xs[0]))
    ctx.close()
    return sync


def test_pipelined_q_calls_equal_the_synchronous_call():
    a = _pipeline_run(1)
    b = _pipeline_run(0)
    for x, y in zip(a, b):
        for u, v in zip(x, y):
            assert np.array_equal(u, v)


def test_cli_qscores_end_to_end_through_fast5(tmp_path):
    """`basecaller --qscores` on a 4000-sample-chunk model through multi-read fast5: the sequences of a run without the flag,
    the qualities of the Python composition of xb_decode_q rows, and a summary whose mean_qscore_template is that of the
    written quality string."""
    from h5write import write_multi_fast5
    from test_gpu_cli import _make_model_dir
    from xna_basecaller_amd import io as xio
    from xna_basecaller_amd import reads as xreads
    from xna_basecaller_amd import util
    from xna_basecaller_amd.crf.basecall import to_str
    from xna_basecaller_amd import toml_lite
    labels = list("NACGTXY")
    model_dir = str(tmp_path / "xna_test@v1")
    cfg, _ = _make_model_dir(model_dir, 64, labels, seed=21)
    # flatter scores than the seeded model's (tanh scale 1.5, blank 0.5): path posteriors below 1, qualities below the Q40
    # ceiling of mean_qscore_from_qstring -- the summary's value then tells the device qualities from the placeholder's 40.0
    cfg["encoder"]["scale"] = 1.5
    cfg["encoder"]["blank_score"] = 0.5
    with open(os.path.join(model_dir, "config.toml"), "w") as fh:
        fh.write(toml_lite.dumps(cfg))
    rng = np.random.default_rng(13)
    recs = []
    for i in range(8):
        length = int(rng.integers(3000, 12000))
        base = rng.normal(90.0, 12.0, length)
        base[: int(rng.integers(300, 900))] = 140.0
        recs.append((np.round(base * 8.0).astype(np.int16),
                     dict(read_id="qqqq-%02d" % i, range=1443.03, digitisation=8192.0, offset=10, sampling_rate=4000.0,
                          run_id="runX", channel_number=str(100 + i), start_mux=1 + i % 4, read_number=i,
                          start_time=4000 * i, duration=length, exp_start_time="2021-06-01T10:00:00Z")))
    f5 = tmp_path / "f5"
    f5.mkdir()
    write_multi_fast5(str(f5 / "batch_0.fast5"), recs, vbz=True)
    batch = 6
    outs = {}
    for flag in ("plain", "q"):
        out = tmp_path / ("calls_%s.fastq" % flag)
        with open(out, "w") as fh:
            r = subprocess.run([sys.executable, "-m", "xna_basecaller_amd", "basecaller", model_dir, str(f5), "--batch", str(batch)]
                               + (["--qscores"] if flag == "q" else []), cwd=ROOT, stdout=fh, stderr=subprocess.PIPE, timeout=600)
        assert r.returncode == 0, r.stderr.decode()
        lines = out.read_text().strip().split("\n")
        summary = (tmp_path / ("calls_%s_summary.tsv" % flag)).read_text().strip().split("\n")
        outs[flag] = (lines, summary)
    (plain, _), (lines, summary) = outs["plain"], outs["q"]
    assert len(lines) == 4 * 8
    assert lines[1::4] == plain[1::4]                                   # sequences byte-equal
    assert all(q == "O" * len(s) for s, q in zip(plain[1::4], plain[3::4]))

    # the Python composition: chunks in the CLI's batches -> scores -> xb_decode_q rows -> the reference's stitch
    model = util.load_model(model_dir, "cuda:0", chunksize=4000, overlap=500, batchsize=batch)
    reads = list(xreads.get_reads(str(f5)))
    chunks = (((rd, 0, len(rd.signal)), util.chunk(np.asarray(rd.signal, np.float32), 4000, 500)) for rd in reads)
    rows = []
    for keys, b in util.batchify(chunks, batchsize=batch):
        seq, _, q, _ = model.decode_q(model(b))
        rows.append((keys, {"sequence": seq, "qstring": q}))
    expect = {}
    for (rd, s, e), res in util.unbatchify(iter(rows)):
        st = util.stitch(res, 4000, 500, e - s, model.stride)
        expect[rd.read_id] = (to_str(st["sequence"]), to_str(st["qstring"]))
    hdr = summary[0].split("\t")
    col = hdr.index("mean_qscore_template")
    means = []
    for rec_hdr, seq, qs, row in zip(lines[0::4], lines[1::4], lines[3::4], summary[1:]):
        rid = rec_hdr[1:].split(" ")[0]
        assert (seq, qs) == expect[rid]
        assert len(qs) == len(seq)
        mq = util.mean_qscore_from_qstring(qs)
        assert row.split("\t")[col] == xio._tsv_field(mq)
        means.append(mq)
    assert sum(len(s) for s in lines[1::4]) > 1000
    assert min(means) < 40.0, means                                     # not the placeholder's constant 40.0
