"""GPU: the fused calls and the Model surface at geometries other than the shipped model's (state_len 3, winlen 19,
stride 5): the fused basecalls give the bytes of encode followed by the matching decode on the same context, that decode
is the oracle's, and a Model built from a config with those values runs forward, decode and `basecall` with them."""
import numpy as np
import pytest

import oracle
from conftest import make_config
from xna_basecaller_amd import _lib
from xna_basecaller_amd.synthetic import peaky_weights

pytestmark = pytest.mark.gpu

QS, QO = 0.9722, 0.3498          # the shipped model's [qscore] section
# (nb, state_len, winlen, stride, features, L, N)
GEOMETRIES = [(4, 4, 9, 6, 64, 1002, 9), (5, 2, 5, 3, 32, 600, 5)]


def _steps(L, W, ST):
    return (L + 2 * (W // 2) - W) // ST + 1


@pytest.mark.parametrize("nb,sl,W,ST,F,L,N", GEOMETRIES)
def test_fused_calls_equal_encode_then_decode(nb, sl, W, ST, F, L, N):
    alphabet = "NACGTXY"[:nb + 1]
    ctx = _lib.Context(0, nb, sl, F, W, ST, 5.0, 2.0, L, N, precision=_lib.XB_PREC_MIXED)
    ctx.load_state_dict(peaky_weights(F, nb, seed=F + nb, state_len=sl, winlen=W))
    assert ctx.T == _steps(L, W, ST)
    x = np.random.default_rng(F + W).standard_normal((N, L)).astype(np.float32)
    scores = ctx.encode(x, expand_blanks=False)
    assert scores.shape == (ctx.T, N, nb ** (sl + 1))
    for fused, want in ((ctx.basecall_chunks(x, alphabet), ctx.decode(scores, alphabet, has_blank=False)),
                        (ctx.basecall_chunks_q(x, alphabet, QS, QO), ctx.decode_q(scores, alphabet, QS, QO, has_blank=False)),
                        (ctx.basecall_chunks_ub(x, alphabet, QS, QO), ctx.decode_ub(scores, alphabet, QS, QO, has_blank=False))):
        assert len(fused) == len(want)
        for g, w in zip(fused, want):
            assert np.array_equal(g, w)
    fused, want = ctx.basecall_chunks_beam(x, alphabet), ctx.beam_search(scores, alphabet)
    for k in ("sequence", "qstring", "moves", "score"):
        assert np.array_equal(fused[k], want[k]), k
    # the decode of those scores is the oracle's, and bases are called
    seq, lens, labels = ctx.decode(scores, alphabet, has_blank=False, want_labels=True)
    ref = oracle.decode(scores, nb, sl, blank_score=2.0)["labels"]
    assert np.array_equal(labels, ref)
    rseq, _, rlens = oracle.pack(ref, alphabet)
    assert np.array_equal(seq, rseq) and np.array_equal(lens, rlens) and lens.min() > 0
    ctx.close()


class _Read:
    def __init__(self, i, n):
        self.read_id = "r%d" % i
        self.signal = np.random.default_rng(i).standard_normal(n).astype(np.float32)


@pytest.mark.parametrize("nb,sl,W,ST,F,L,N", GEOMETRIES)
def test_model_surface(nb, sl, W, ST, F, L, N):
    import torch
    from xna_basecaller_amd.crf import Model
    from xna_basecaller_amd.crf.basecall import basecall, compute_scores
    labels = list("NACGTXY"[:nb + 1])
    cfg = make_config(F, labels)
    cfg["global_norm"]["state_len"] = sl
    cfg["encoder"]["winlen"] = W
    cfg["encoder"]["stride"] = ST
    model = Model(cfg)
    sd = peaky_weights(F, nb, seed=F + nb, state_len=sl, winlen=W)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    model = model.to("cuda")
    assert model.stride == ST
    T = _steps(L, W, ST)
    batch = np.random.default_rng(L).standard_normal((N, 1, L)).astype(np.float32)
    scores = model(batch)
    assert scores.shape == (T, N, (nb + 1) * nb ** sl)
    ref = oracle.decode(scores, nb, sl)["labels"]
    rseq, _, rlens = oracle.pack(ref, "".join(labels))
    want = [rseq[i, :rlens[i]].tobytes().decode() for i in range(N)]
    assert model.decode_batch(scores) == want and min(map(len, want)) > 0
    res = compute_scores(model, batch)
    assert np.array_equal(res["sequence"], rseq)
    # two reads, one longer than a chunk and one shorter
    chunksize, overlap = L, 10 * ST
    reads = [_Read(1, 2 * L + 7 * ST + 1), _Read(2, L // 2 + 3)]
    out = list(basecall(model, reads, chunksize=chunksize, overlap=overlap, batchsize=N, qscores=True))
    assert [r.read_id for r, _ in out] == ["r1", "r2"]
    for read, res in out:
        assert len(res["sequence"]) > 0 and set(res["sequence"]) <= set(labels[1:])
        assert len(res["qstring"]) == len(res["sequence"])
        marks = np.flatnonzero(res["sig_move"])
        assert len(marks) > 0 and np.all(marks % ST == 0) and res["sig_move"].size % ST == 0
        if len(read.signal) < chunksize:                     # one chunk: nothing is stitched, one mark per base
            assert len(marks) == len(res["sequence"])
