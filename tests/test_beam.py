"""CRF beam search with qualities and moves (crf/basecall.py:33-46 -> koi.decode.beam_search).

koi 0.0.5 is not in the reference tree and the reference holds no vectors for it: PARITY UNPINNED.  What can be checked:
CPU tier -- the oracle's restatement (oracle/xna_oracle.c, "CRF beam search") against (a) an independent float64 Python
restatement that merges hypotheses by their actual state sequences instead of CRC hashes, (b) exhaustive enumeration of every
alignment of tiny problems (with a beam that holds every hypothesis the search is exact: its score is the best sequence's
log-sum over alignments), (c) structural properties; the host pipeline around the operator with a stand-in model.
GPU tier -- xb_beam_search / xb_basecall_chunks_beam bit-equal to the oracle for n_base 4 / 5 / 6, several state lengths, beam
widths and cuts on Gaussian scores, and the Model-level compute_scores / basecall on a blank-less model.  Every state length, the
tile edges, ties and the branches these scores never take (the one-merge-at-a-time path among them): tests/test_gpu_beam.py on
the cases of tests/beam_cases.py.
"""
import importlib
import itertools
import math

import numpy as np
import pytest

import oracle
from beam_cases import _beam_py
from conftest import make_config, random_scores

FLT_MAX = float(np.finfo(np.float32).max)
ALPHA = {4: "NACGT", 5: "NACGTX", 6: "NACGTXY", 2: "NAC", 3: "NACG"}


def _scores(T, N, nb, sl, seed, gain=3.0):
    rng = np.random.default_rng(seed)
    return (gain * rng.standard_normal((T, N, nb ** sl * nb))).astype(np.float32)


def _strings(plane):
    return [bytes(r[r != 0].astype(np.uint8)).decode() for r in plane]


@pytest.mark.parametrize("nb,sl,W,cut", [(4, 3, 32, 100.0), (6, 2, 8, 100.0), (5, 3, 32, 4.0), (4, 2, 5, 1e6), (6, 3, 32, 100.0)])
def test_oracle_beam_search_against_a_float64_restatement_keyed_by_sequences(nb, sl, W, cut):
    T, N = 48, 3
    sc = _scores(T, N, nb, sl, seed=nb * 10 + sl)
    o = oracle.beam_search(sc, ALPHA[nb], sl, beam_width=W, beam_cut=cut, blank_score=2.0)
    d = oracle.decode(sc, nb, sl, blank_score=2.0, want=("beta",))
    S, E = nb ** sl, nb + 1
    for n in range(N):
        M = np.full((T, S, E), 2.0)
        M[:, :, 1:] = sc[:, n].reshape(T, S, nb)
        score, path, moves = _beam_py(M, d["beta"][:, n].astype(np.float64), nb, sl, W, math.log(cut))
        assert np.array_equal(o["moves"][n], np.array(moves, np.uint8))
        want = "".join(ALPHA[nb][1 + s % nb] for s, m in zip(path, moves) if m)
        assert _strings(o["sequence"][n:n + 1])[0] == want
        assert abs(float(o["score"][n]) - score) < 2e-3


@pytest.mark.parametrize("nb,sl,T", [(2, 1, 4), (3, 1, 2), (2, 2, 3)])
def test_oracle_beam_search_is_exact_when_the_beam_holds_every_hypothesis(nb, sl, T):
    """Enumerate every alignment (initial state, then stay or step per block), sum the alignments of one state sequence
    (= one hypothesis) in the log domain: the search's score is the best hypothesis' total."""
    S, hi, E = nb ** sl, nb ** (sl - 1), nb + 1
    for seed in range(6):
        sc = _scores(T, 1, nb, sl, seed=100 * nb + seed, gain=2.0)
        M = np.full((T, S, E), 2.0)
        M[:, :, 1:] = sc[:, 0].reshape(T, S, nb)
        totals = {}
        for s0 in range(S):
            for edges in itertools.product(range(E), repeat=T):          # 0 = stay, 1 + b = step to base b
                st, key, v = s0, (s0,), 0.0
                for t, e in enumerate(edges):
                    if e == 0:
                        v += M[t, st, 0]
                    else:
                        j = (st % hi) * nb + e - 1
                        v += M[t, j, 1 + st // hi]
                        st, key = j, key + (j,)
                totals[key] = np.logaddexp(totals.get(key, -np.inf), v)
        assert len(totals) <= 32 * E                                      # every block's candidates fit the beam's list
        o = oracle.beam_search(sc, ALPHA[nb], sl, beam_width=32, beam_cut=1e30, blank_score=2.0)
        assert max(len([k for k in totals if len(k) == m]) for m in range(1, T + 2)) <= 32      # ... and its hypotheses the beam
        assert abs(float(o["score"][0]) - max(totals.values())) < 1e-4


def test_oracle_beam_search_structure_and_qualities():
    nb, sl, T, N = 6, 3, 300, 4
    sc = _scores(T, N, nb, sl, seed=5)
    with_blank = np.full((T, N, nb ** sl, nb + 1), 2.0, np.float32)
    with_blank[..., 1:] = sc.reshape(T, N, nb ** sl, nb)
    o = oracle.beam_search(sc, ALPHA[nb], sl, blank_score=2.0)
    ob = oracle.beam_search(with_blank.reshape(T, N, -1), ALPHA[nb], sl)
    for k in o:                                                   # the blank column and the constant are the same input
        assert np.array_equal(o[k], ob[k])
    assert np.all(o["moves"][:, 0] == 1)
    assert np.array_equal(o["moves"] != 0, o["sequence"] != 0) and np.array_equal(o["moves"] != 0, o["qstring"] != 0)
    q = o["qstring"][o["qstring"] != 0]
    assert q.min() >= 34 and q.max() <= 83                        # phred 1..50
    assert set(np.unique(o["sequence"][o["sequence"] != 0])) <= {ord(c) for c in ALPHA[nb][1:]}
    # the result's log-sum score cannot exceed logZ, and is at least the best single alignment's score
    d = oracle.decode(sc, nb, sl, blank_score=2.0, want=("logz", "amax"))
    assert np.all(o["score"] <= d["logz"] + 1e-3)
    # scale / offset act on the phred value before the clamp
    o2 = oracle.beam_search(sc, ALPHA[nb], sl, blank_score=2.0, scale=0.5, offset=3.0)
    assert np.array_equal(o2["sequence"], o["sequence"]) and not np.array_equal(o2["qstring"], o["qstring"])
    # a dominant path: every posterior is ~1 and the qualities saturate at 50
    rng = np.random.default_rng(0)
    S = nb ** sl
    peaky = np.full((40, 1, S, nb), -20.0, np.float32)
    st = 7
    for t in range(40):
        b = int(rng.integers(nb))
        j = (st % (S // nb)) * nb + b
        peaky[t, 0, j, st // (S // nb)] = 20.0
        st = j
    op = oracle.beam_search(peaky.reshape(40, 1, -1), ALPHA[nb], sl, blank_score=2.0)
    assert op["moves"].sum() == 40 and np.all(op["qstring"] == 83)
    with pytest.raises(ValueError):
        oracle.beam_search(sc, ALPHA[nb], sl, beam_width=33, blank_score=2.0)


class _StandInModel:
    """compute_scores' view of a blank-less model whose device calls are the oracle (host-side plumbing test only)."""
    stride = 5

    class _Last:
        expand_blanks, blank_score = False, 2.0

    def __init__(self, nb, sl, T):
        self.nb, self.sl, self.T, self.alphabet = nb, sl, T, ALPHA[nb]
        self.encoder = [self._Last()]

    def _scores_of(self, batch):
        sig = np.asarray(batch, dtype=np.float32).reshape(len(batch), -1)
        return np.stack([_scores(self.T, 1, self.nb, self.sl, seed=int(abs(s[:16]).sum() * 1e3) % 2 ** 31)[:, 0] for s in sig], 1)

    def basecall_chunks_beam(self, batch, beam_width, beam_cut, scale, offset):
        return oracle.beam_search(self._scores_of(batch), self.alphabet, self.sl, beam_width, beam_cut, scale, offset, blank_score=2.0)


def test_host_pipeline_stitches_sequence_quality_and_moves():
    bc = importlib.import_module("xna_basecaller_amd.crf.basecall")
    nb, sl, chunksize, overlap = 4, 2, 400, 100
    model = _StandInModel(nb, sl, chunksize // 5)

    class Read:
        def __init__(self, n, seed):
            self.signal = np.random.default_rng(seed).standard_normal(n).astype(np.float32)

    reads = [Read(1000, 1), Read(250, 2), Read(400, 3)]
    out = list(bc.basecall(model, reads, chunksize=chunksize, overlap=overlap, batchsize=4))
    assert [r for r, _ in out] == reads
    for read, res in out:
        assert len(res["sequence"]) == len(res["qstring"]) > 0
        assert res["sig_move"].dtype == bool and res["sig_move"].sum() == len(res["sequence"])
        assert res["sig_move"].size % model.stride == 0 and np.all(np.where(res["sig_move"])[0] % model.stride == 0)
        assert 1.0 <= res["mean_qscore"] <= 50.0
    # one chunk: the stitched planes are the operator's own rows (crf/basecall.py:15-24, util.stitch with one chunk)
    single = bc.compute_scores(model, reads[2].signal[None, None, :])
    assert out[2][1]["sequence"] == bc.to_str(single["sequence"][0]) and out[2][1]["qstring"] == bc.to_str(single["qstring"][0])
    assert np.array_equal(np.where(out[2][1]["sig_move"])[0], np.where(single["moves"][0])[0] * model.stride)
    with pytest.raises(ValueError):
        bc.compute_scores(model, reads[2].signal[None, None, :], blank_score=1.0)


# ---------------------------------------------------------------------------------------------------------------------
GPU_CASES = [
    # nb, sl, T, N, beam_width, beam_cut, with_blank
    (4, 3, 130, 5, 32, 100.0, False),
    (4, 5, 70, 3, 32, 100.0, False),          # 1024 states: the start threshold selects 32 of them
    (5, 3, 257, 4, 32, 100.0, True),
    (6, 3, 400, 6, 32, 100.0, False),
    (6, 3, 100, 3, 7, 3.0, False),
    (6, 2, 64, 2, 1, 100.0, True),
    (4, 2, 90, 3, 32, 100.0, False),          # 16 states: fewer states than beam elements
    (5, 2, 150, 4, 32, 0.0, False),           # no cut: merged-away duplicates stay in the beam (6880 merges, but with 5 bases no
                                              # stay matches two steps and no two stays claim one: beam_cases.py's nocut-4 rows do)
    (6, 3, 120, 3, 32, 1e30, True),
]


@pytest.mark.gpu
@pytest.mark.parametrize("nb,sl,T,N,W,cut,with_blank", GPU_CASES)
def test_gpu_beam_search_is_the_oracles_bit_for_bit(nb, sl, T, N, W, cut, with_blank):
    from xna_basecaller_amd import _lib
    sc = _scores(T, N, nb, sl, seed=T + nb)
    if with_blank:
        full = np.full((T, N, nb ** sl, nb + 1), 2.0, np.float32)
        full[..., 1:] = sc.reshape(T, N, nb ** sl, nb)
        full[..., 0] += 0.25 * np.random.default_rng(1).standard_normal((T, N, nb ** sl)).astype(np.float32)   # a learned blank
        sc = full.reshape(T, N, -1)
    ctx = _lib.Context(0, nb, sl, 32, 19, 5, 5.0, 2.0, T * 5, N)
    for scale, offset in ((1.0, 0.0), (0.9722, 0.3498)):
        got = ctx.beam_search(sc, ALPHA[nb], beam_width=W, beam_cut=cut, scale=scale, offset=offset)
        ref = oracle.beam_search(sc, ALPHA[nb], sl, beam_width=W, beam_cut=cut, scale=scale, offset=offset, blank_score=2.0)
        for k in ("moves", "sequence", "qstring", "score"):
            assert np.array_equal(got[k], ref[k]), k
    with pytest.raises(_lib.XbError):
        ctx.beam_search(sc, ALPHA[nb], beam_width=33)
    with pytest.raises(_lib.XbError):
        ctx.beam_search(sc, ALPHA[nb][:-1])
    ctx.close()


@pytest.mark.gpu
def test_gpu_beam_search_full_chunk_length_and_device_entry_point():
    import torch
    from xna_basecaller_amd import _lib
    nb, sl, T, N = 6, 3, 2000, 8
    sc = random_scores(T, N, nb, sl, seed=3, with_blank=False)
    ctx = _lib.Context(0, nb, sl, 32, 19, 5, 5.0, 2.0, T * 5, N)
    ref = oracle.beam_search(sc, ALPHA[nb], sl, blank_score=2.0)
    d_sc = torch.from_numpy(sc).cuda()
    d_seq = torch.zeros((N, T), dtype=torch.int8, device="cuda")
    d_q = torch.zeros((N, T), dtype=torch.int8, device="cuda")
    d_mv = torch.zeros((N, T), dtype=torch.uint8, device="cuda")
    d_score = torch.zeros((N,), dtype=torch.float32, device="cuda")
    ctx.beam_search_dev(d_sc.data_ptr(), T, N, 0, ALPHA[nb], d_seq.data_ptr(), d_q.data_ptr(), d_mv.data_ptr(), d_score.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_seq.cpu().numpy(), ref["sequence"]) and np.array_equal(d_q.cpu().numpy(), ref["qstring"])
    assert np.array_equal(d_mv.cpu().numpy(), ref["moves"]) and np.array_equal(d_score.cpu().numpy(), ref["score"])
    # the Viterbi decode of the same scores: random scores carry no ridge, the two decoders agree only loosely
    seq, lens = ctx.decode(sc, ALPHA[nb])
    vit = seq[0, :lens[0]].tobytes().decode()
    beam = _strings(ref["sequence"][:1])[0]
    assert _lib.align_accuracy(vit, beam) > 50.0
    ctx.close()


@pytest.mark.gpu
def test_gpu_model_beam_branch_of_compute_scores_and_basecall():
    bc = importlib.import_module("xna_basecaller_amd.crf.basecall")
    from xna_basecaller_amd.crf.model import Model
    from xna_basecaller_amd.synthetic import peaky_weights
    labels = ("N", "A", "C", "G", "T")
    cfg = make_config(features=96, labels=labels)
    cfg["encoder"]["expand_blanks"] = False
    model = Model(cfg)
    import torch
    sd = peaky_weights(96, 4, seed=11)
    assert set(sd) == set(model.state_dict())
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()})
    model = model.to("cuda")
    assert not model.encoder[-1].expand_blanks
    L, N = 2000, 5
    batch = np.random.default_rng(2).standard_normal((N, 1, L)).astype(np.float32)
    got = bc.compute_scores(model, batch, scale=0.9722, offset=0.3498)
    scores = model(batch)                                                  # (T, N, S * nb): no blank column
    assert scores.shape[2] == 4 ** 3 * 4
    ref = oracle.beam_search(scores, "".join(labels), 3, scale=0.9722, offset=0.3498, blank_score=2.0)
    assert np.array_equal(got["sequence"], ref["sequence"]) and np.array_equal(got["qstring"], ref["qstring"])
    assert got["moves"].dtype == bool and np.array_equal(got["moves"], ref["moves"].astype(bool))
    assert (got["sequence"] != 0).sum() > 0.1 * got["sequence"].size       # the peaky model calls bases

    class Read:
        def __init__(self, n, seed):
            self.signal = np.random.default_rng(seed).standard_normal(n).astype(np.float32)

    reads = [Read(5000, 1), Read(1500, 2)]
    out = list(bc.basecall(model, reads, chunksize=2000, overlap=500, batchsize=4))
    for read, res in out:
        assert len(res["sequence"]) == len(res["qstring"]) == int(res["sig_move"].sum()) > 0
        assert set(res["sequence"]) <= set("ACGT")
