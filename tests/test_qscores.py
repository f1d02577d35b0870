"""CPU: the Viterbi qualities (xb_decode_q) -- the restatement in tests/qscore_ref.py against the oracle's decode, hand-built
cases of the specification, and the host plumbing of `basecaller --qscores` with a stub model."""
import numpy as np
import pytest

import oracle
from conftest import make_config, random_scores
import qscore_ref
from pairs import NEW_PAIRS

F32 = np.float32


@pytest.mark.parametrize("nb", [4, 5, 6])
@pytest.mark.parametrize("with_blank", [True, False])
def test_restated_path_gives_the_oracles_labels(nb, with_blank):
    """f_t rebuilt from the oracle's max-marginals: f_t % E is the oracle's label bit for bit."""
    T, N = 157, 3
    sc = random_scores(T, N, nb, seed=40 + nb, with_blank=with_blank)
    f, ref = qscore_ref.path_edges(sc, nb, blank_score=None if with_blank else 2.0)
    assert np.array_equal((f % (nb + 1)).astype(np.int8), ref["labels"])
    assert f.min() >= 0 and f.max() < nb ** 3 * (nb + 1)


def test_restated_sequences_are_the_oracles():
    nb, alphabet = 6, "NACGTXY"
    sc = random_scores(90, 4, nb, seed=5)
    got = qscore_ref.decode_q(sc, nb, alphabet)
    seq, _, lens = oracle.pack(got["labels"], alphabet)
    assert np.array_equal(got["seq"], seq) and np.array_equal(got["seq_len"], lens)
    assert np.array_equal(got["moves"], (got["labels"] != 0).astype(np.uint8))
    # qstring is packed in parallel with seq: the same count of non-zero bytes, all printable phred+33 characters
    assert np.array_equal((got["qstring"] != 0).sum(axis=1), lens)
    q = got["qstring"][got["qstring"] != 0]
    assert q.min() >= 34 and q.max() <= 83


@pytest.mark.parametrize("with_blank", [True, False])
@pytest.mark.parametrize("nb,sl", NEW_PAIRS)
def test_restatement_at_every_state_length(nb, sl, with_blank):
    """The two checks above at the other state lengths: the rebuilt path is the oracle's, the packed rows are its pack."""
    T, N, alphabet = 61, 3, "NACGTXY"[:nb + 1]
    blank = None if with_blank else 2.0
    sc = random_scores(T, N, nb, sl=sl, seed=40 + nb + sl, with_blank=with_blank)
    f, ref = qscore_ref.path_edges(sc, nb, sl, blank_score=blank)
    assert np.array_equal((f % (nb + 1)).astype(np.int8), ref["labels"])
    assert f.min() >= 0 and f.max() < nb ** sl * (nb + 1)
    got = qscore_ref.decode_q(sc, nb, alphabet, sl=sl, blank_score=blank)
    assert np.array_equal(got["labels"], ref["labels"])
    seq, _, lens = oracle.pack(got["labels"], alphabet)
    assert np.array_equal(got["seq"], seq) and np.array_equal(got["seq_len"], lens)
    assert np.array_equal(got["moves"], (got["labels"] != 0).astype(np.uint8))
    assert np.array_equal((got["qstring"] != 0).sum(axis=1), lens)
    q = got["qstring"][got["qstring"] != 0]
    assert q.min() >= 34 and q.max() <= 83


def _dominant_scores(nb, T, N, sl=3, seed=0):
    """Flat scores plus +20 on one edge per step along a consistent path that emits on most steps."""
    rng = np.random.default_rng(seed)
    S, E = nb ** sl, nb + 1
    sc = np.zeros((T, N, S, E), np.float32)
    for n in range(N):
        s = int(rng.integers(S))
        for t in range(T):
            b = int(rng.integers(nb))
            j = (s % nb ** (sl - 1)) * nb + b                  # a move into j (edge k = 1 + base dropped from s)
            k = 1 + s // nb ** (sl - 1)
            sc[t, n, j, k] = 20.0
            s = j
    return sc.reshape(T, N, S * E)


def test_dominant_path_saturates_at_q50():
    nb = 4
    sc = _dominant_scores(nb, 40, 2)
    got = qscore_ref.decode_q(sc, nb, "NACGT")
    assert got["seq_len"].min() == 40                        # every step emits
    q = got["qstring"][:, :40]
    assert np.all(q == ord("S")), q                           # 33 + 50


def test_flat_scores_give_low_qualities():
    nb = 5
    sc = np.zeros((60, 2, nb ** 3, nb + 1), np.float32)       # every base equally likely at every step ...
    sc[..., 0] = -1.0                                          # ... and a stay less likely than a move
    sc = sc.reshape(60, 2, -1)
    got = qscore_ref.decode_q(sc, nb, "NACGTX")
    q = got["qstring"][got["qstring"] != 0].astype(int) - 33
    assert len(q) > 0 and q.max() <= 5, q


def test_hand_worked_two_base_chunk():
    """nb = 4, p = (1, 0.5, 0), moves (1, 0, 1).  Base 1 spans steps 0-1: bp = 1.5, tot = 1 + (0.5 + 3 * 0.5 / 3) = 2,
    e = 0.25, q = 6.02 -> chr(int(39.52)) = "'".  Base 2 at step 2: p = 0, e = 1, q = 0 -> clamped to 1 -> '"'."""
    got = qscore_ref.base_qualities(np.array([1.0, 0.5, 0.0], F32), np.array([1, 0, 1], bool), 4)
    assert bytes(got) == b"'\""
    # the steps before the first move belong to no base
    got = qscore_ref.base_qualities(np.array([0.0, 0.0, 1.0, 0.5], F32), np.array([0, 0, 1, 0], bool), 4)
    assert bytes(got) == b"'"
    assert len(qscore_ref.base_qualities(np.ones(5, F32), np.zeros(5, bool), 4)) == 0


def test_qscale_qoffset_and_clamps():
    p = np.array([0.9, 0.99, 0.999, 0.0, 1.0], F32)
    mv = np.ones(5, bool)
    base = qscore_ref.base_qualities(p, mv, 4).astype(int) - 33
    # e = 1 - p per single-step base: q = -10 log10(1 - p) (10, 20, 30 up to rounding), p = 0 -> 1, p = 1 -> FLT_MAX -> 50
    assert list(base) == [10, 19, 29, 1, 50] or list(base) == [10, 20, 30, 1, 50], base
    scaled = qscore_ref.base_qualities(p, mv, 4, qscale=0.5, qoffset=3.0).astype(int) - 33
    assert list(scaled[:3]) == [int(0.5 + 3.0 + 0.5 * q) for q in (10.0, 20.0, 30.0)]
    assert scaled[3] == 3 and scaled[4] == 50                # q = 0 * 0.5 + 3 = 3;  FLT_MAX * 0.5 + 3 -> 50
    low = qscore_ref.base_qualities(p, mv, 4, qscale=1.0, qoffset=-100.0).astype(int) - 33
    assert list(low) == [1, 1, 1, 1, 50]                     # an error-free base stays at FLT_MAX before the clamp
    high = qscore_ref.base_qualities(p, mv, 4, qscale=1.0, qoffset=100.0).astype(int) - 33
    assert np.all(high == 50)


# ---- host plumbing with a stub model ------------------------------------------------------------------------------------

class _StubModel:
    """Stand-in for crf.model.Model on the host path of `basecall`: every chunk of T steps calls one base every 3rd step,
    with a quality character derived from the chunk's first sample."""

    class _Enc:
        expand_blanks = True
        blank_score = 2.0

    stride = 5
    alphabet = ["N", "A", "C", "G", "T", "X", "Y"]

    def __init__(self):
        self.encoder = [self._Enc()]
        self.config = make_config()
        self.busy = {}
        self.qscore_calls = []

    def qscore_params(self):
        q = self.config["qscore"]
        return q["scale"], q["bias"]

    def context_is_current(self, chunk_len, batch):
        return True

    def pipeline_depth(self, chunk_len, n):
        return 2

    def _rows(self, batch, qscores):
        batch = np.asarray(batch)
        n, T = batch.shape[0], batch.shape[-1] // self.stride
        seq = np.zeros((n, T), np.int8)
        q = np.zeros((n, T), np.int8)
        mv = np.zeros((n, T), np.uint8)
        mv[:, ::3] = 1
        k = int(mv[0].sum())
        seq[:, :k] = ord("A")
        q[:, :k] = (35 + (np.abs(batch[:, 0, :1]) * 10).astype(np.int8) % 40)
        self.qscore_calls.append(qscores)
        return (seq, np.full(n, k, np.int32), q, mv) if qscores else (seq, np.full(n, k, np.int32))

    def basecall_chunks(self, batch, qscores=False):
        return self._rows(batch, qscores)

    def submit_chunks(self, slot, batch, qscores=False):
        assert slot not in self.busy
        self.busy[slot] = self._rows(batch, qscores)
        return ("ctx", slot, np.asarray(batch).shape[0]) + ((True,) if qscores else ())

    def collect_chunks(self, handle):
        return self.busy.pop(handle[1])


class _Read:
    def __init__(self, i, n):
        self.read_id = "r%d" % i
        self.signal = np.random.default_rng(i).standard_normal(n).astype(np.float32)


def _run(qscores, reads, chunksize=1000, overlap=100):
    from xna_basecaller_amd.crf.basecall import basecall
    model = _StubModel()
    kw = {"qscores": True} if qscores else {}
    out = list(basecall(model, reads, chunksize=chunksize, overlap=overlap, batchsize=4, **kw))
    return model, out


def test_basecall_with_qscores_stitches_qualities_beside_the_bases():
    from xna_basecaller_amd.util import mean_qscore_from_qstring
    reads = [_Read(i, n) for i, n in enumerate([700, 2500, 4100, 1000, 9000])]
    model, out = _run(True, reads)
    assert set(model.qscore_calls) == {True}
    for read, res in out:
        assert len(res["qstring"]) == len(res["sequence"]) > 0
        assert res["mean_qscore"] == mean_qscore_from_qstring(res["qstring"])
        assert res["mean_qscore"] != 40.0
        assert res["sig_move"].dtype == bool and res["sig_move"].any()
        assert len(res["sig_move"]) % model.stride == 0


def test_basecall_without_qscores_is_unchanged():
    reads = [_Read(i, n) for i, n in enumerate([700, 2500, 4100])]
    model, out = _run(False, reads)
    assert set(model.qscore_calls) == {False}
    for read, res in out:
        assert set(res) == {"qstring", "sequence", "sig_move", "mean_qscore"}
        assert res["qstring"] == "O" * len(res["sequence"]) and res["mean_qscore"] == 40.0
        assert not res["sig_move"].any()
    # the sequences do not depend on the flag
    _, out_q = _run(True, reads)
    assert [r["sequence"] for _, r in out] == [r["sequence"] for _, r in out_q]


def test_compute_scores_with_qscores_returns_the_device_planes():
    from xna_basecaller_amd.crf.basecall import compute_scores
    model = _StubModel()
    batch = np.random.default_rng(1).standard_normal((3, 1, 500)).astype(np.float32)
    res = compute_scores(model, batch, qscores=True)
    assert set(res) == {"qstring", "sequence", "moves"} and res["moves"].dtype == bool
    assert np.array_equal(res["moves"], model._rows(batch, True)[3].astype(bool))
    plain = compute_scores(model, batch)
    assert np.array_equal(plain["sequence"], res["sequence"])
    assert np.all(plain["qstring"][plain["sequence"] != 0] == ord("O")) and not plain["moves"].any()


def test_cli_parses_qscores():
    from xna_basecaller_amd.cli.basecaller import argparser
    p = argparser()
    assert p.parse_args(["m", "r", "--qscores"]).qscores is True
    assert p.parse_args(["m", "r"]).qscores is False


def test_model_qscore_params_follow_the_config():
    from xna_basecaller_amd.crf.model import Model
    m = Model(make_config(features=32))
    assert m.qscore_params() == (pytest.approx(0.9722), pytest.approx(0.3498))
    c = make_config(features=32)
    del c["qscore"]
    assert Model(c).qscore_params() == (1.0, 0.0)
