"""CPU: the per-base letter probabilities (xb_decode_ub) -- the restatement in tests/ubprob_ref.py against an exhaustive
enumeration of tiny CRFs, hand-built cases of the specification, and the host plumbing of `basecaller --ub-probs` (planes,
tags, writers, the torchrun gather) with a stub model."""
import io
import itertools
import os
import socket
import subprocess
import sys

import numpy as np
import pytest

import oracle
from conftest import ROOT, random_scores
import ubprob_ref
from pairs import NEW_PAIRS
from test_qscores import _StubModel, _Read

F32 = np.float32


# ---- the restatement against every path of a tiny CRF -----------------------------------------------------------------

def _enumerate(scores, nb, sl):
    """float64 edge posteriors (T, S*E) of one chunk by enumerating every path: any start state (alpha_0 = 0), at every
    step one of the E out-edges of the current state (source idx(j, k) = (k - 1) * hi + j / nb for k >= 1, j itself for the
    stay k = 0), any end state (beta_T = 0)."""
    S, E, hi = nb ** sl, nb + 1, nb ** (sl - 1)
    T = scores.shape[0]
    M = scores.astype(np.float64).reshape(T, S, E)
    out_edges = [[(i, 0)] + [((i % hi) * nb + e - 1, i // hi + 1) for e in range(1, nb + 1)] for i in range(S)]
    weights, used = [], []
    for s0 in range(S):
        for choice in itertools.product(range(E), repeat=T):
            s, score, edges = s0, 0.0, []
            for t, c in enumerate(choice):
                j, k = out_edges[s][c]
                score += M[t, j, k]
                edges.append(j * E + k)
                s = j
            weights.append(score)
            used.append(edges)
    w = np.exp(np.array(weights) - max(weights))
    w /= w.sum()
    post = np.zeros((T, S * E))
    for wt, edges in zip(w, used):
        for t, c in enumerate(edges):
            post[t, c] += wt
    return post


@pytest.mark.parametrize("nb,sl,T", [(2, 1, 5), (2, 2, 4), (3, 1, 5), (3, 2, 3), (4, 1, 4), (4, 2, 2)])
def test_restatement_matches_exhaustive_enumeration(nb, sl, T):
    S, E = nb ** sl, nb + 1
    rng = np.random.default_rng(100 * nb + 10 * sl + T)
    sc = (2.0 * np.tanh(rng.standard_normal((T, 1, S * E)))).astype(np.float32)
    got = ubprob_ref.decode_ub(sc, nb, "NACGTXY"[:nb + 1], sl=sl)
    post64 = _enumerate(sc[:, 0], nb, sl)
    assert np.abs(got["post"][:, 0] - post64).max() < 1e-5
    # letter mass: every move edge into any destination with label k = b + 1
    e64 = post64.reshape(T, S, E)[:, :, 1:].sum(axis=1)
    assert np.abs(got["e"][:, 0] - e64).max() < 1e-5
    # windowed probabilities over the decode's own path
    moves = got["moves"][0] != 0
    L = int(moves.sum())
    for i, (t, lo, hi) in enumerate(ubprob_ref.base_windows(moves)):
        mass = e64[lo:hi].sum(axis=0)
        want = mass / mass.sum()
        assert np.abs(got["prob"][0, :, i] - want).max() < 1e-5, (i, t, lo, hi)
    assert not got["probs"][0, :, L:].any() and not got["prob"][0, :, L:].any()


# ---- properties ------------------------------------------------------------------------------------------------------

def _dominant(nb, T, N, sl=3, seed=0):
    """Flat scores plus +20 on one move edge per step along a consistent path (every step emits); the letters called."""
    rng = np.random.default_rng(seed)
    S, E, hi = nb ** sl, nb + 1, nb ** (sl - 1)
    sc = np.zeros((T, N, S, E), np.float32)
    letters = np.zeros((N, T), np.int64)
    for n in range(N):
        s = int(rng.integers(S))
        for t in range(T):
            j = (s % hi) * nb + int(rng.integers(nb))
            k = 1 + s // hi
            sc[t, n, j, k] = 20.0
            letters[n, t] = k - 1
            s = j
    return sc.reshape(T, N, S * E), letters


def test_dominant_path_gives_255_for_the_called_letter():
    nb, T, N = 5, 30, 2
    sc, letters = _dominant(nb, T, N)
    got = ubprob_ref.decode_ub(sc, nb, "NACGTX")
    assert got["seq_len"].min() == T
    for n in range(N):
        pl = got["probs"][n, :, :T]
        assert np.all(pl[letters[n], np.arange(T)] == 255)
        other = np.ones_like(pl, bool)
        other[letters[n], np.arange(T)] = False
        assert not pl[other].any()


@pytest.mark.parametrize("nb", [4, 5, 6])
def test_flat_scores_give_an_even_split(nb):
    sc = np.zeros((40, 2, nb ** 3, nb + 1), np.float32)
    sc[..., 0] = -1.0                                          # moves more likely than stays: bases get called
    got = ubprob_ref.decode_ub(sc.reshape(40, 2, -1), nb, "NACGTXY"[:nb + 1])
    L = got["seq_len"]
    assert L.min() > 0
    for n in range(2):
        v = got["probs"][n, :, :L[n]].astype(int)
        assert np.abs(v - 256 / nb).max() <= 1, v


@pytest.mark.parametrize("with_blank", [True, False])
def test_probabilities_sum_to_one(with_blank):
    nb = 6
    sc = random_scores(120, 3, nb, seed=9, with_blank=with_blank)
    got = ubprob_ref.decode_ub(sc, nb, "NACGTXY", blank_score=None if with_blank else 2.0)
    for n in range(3):
        L = got["seq_len"][n]
        assert L > 0
        s = got["prob"][n, :, :L].astype(np.float64).sum(axis=0)
        assert np.abs(s - 1.0).max() < 1e-6
        # bytes floor the probabilities: their sum is at most 256 and loses less than one per letter
        tot = got["probs"][n, :, :L].astype(int).sum(axis=0)
        assert np.all(tot <= 256) and np.all(tot > 256 - nb)
        assert not got["probs"][n, :, L:].any()
    # the bases, qualities and moves are those of the quality decode
    import qscore_ref
    q = qscore_ref.decode_q(sc, nb, "NACGTXY", blank_score=None if with_blank else 2.0)
    for k in ("seq", "qstring", "moves", "seq_len"):
        assert np.array_equal(got[k], q[k])


@pytest.mark.parametrize("with_blank", [True, False])
@pytest.mark.parametrize("nb,sl", NEW_PAIRS)
def test_restatement_at_every_state_length(nb, sl, with_blank):
    """The state lengths other than 3 (nb^(sl - 1) = 4 .. 256 sources per letter: fewer than the 16 summing lanes, and
    many rounds of them): the posteriors and the letter mass against float64 (autograd posteriors and their float64
    sums), probabilities that sum to one, and the quality decode's bases, qualities and moves.  Tolerance 1e-4, the one
    tests/test_oracle.py holds the oracle's posteriors to on these scores: in the fp32 log domain the exponent
    alpha + M + beta - logZ carries the rounding of numbers of size |logZ| ~ 6 T = 240, i.e. 240 x 2^-24 = 1.4e-5 relative
    on a posterior of up to 1, and a letter's mass is a sum of posteriors that total at most 1."""
    import qscore_ref
    from test_oracle import _fp64_posteriors
    T, N, alphabet = 40, 2, "NACGTXY"[:nb + 1]
    S, E = nb ** sl, nb + 1
    blank = None if with_blank else 2.0
    sc = random_scores(T, N, nb, sl=sl, seed=9 + nb + sl, with_blank=with_blank)
    got = ubprob_ref.decode_ub(sc, nb, alphabet, sl=sl, blank_score=blank)
    # the float64 posteriors take the layout with the blank column; the blank-less run above adds the same constant 2.0
    # (random_scores' blank and blank_score), so one float64 result serves both layouts
    post64, _ = _fp64_posteriors(random_scores(T, N, nb, sl=sl, seed=9 + nb + sl), nb, sl)
    assert np.abs(got["post"] - post64).max() < 1e-4
    e64 = post64.reshape(T, N, S, E)[..., 1:].sum(axis=2)
    assert np.abs(got["e"] - e64).max() < 1e-4
    for n in range(N):
        L = got["seq_len"][n]
        assert L > 0
        assert np.abs(got["prob"][n, :, :L].astype(np.float64).sum(axis=0) - 1.0).max() < 1e-6
        tot = got["probs"][n, :, :L].astype(int).sum(axis=0)
        assert np.all(tot <= 256) and np.all(tot > 256 - nb)
        assert not got["probs"][n, :, L:].any()
    q = qscore_ref.decode_q(sc, nb, alphabet, sl=sl, blank_score=blank)
    for k in ("seq", "qstring", "moves", "seq_len"):
        assert np.array_equal(got[k], q[k])


def test_hand_worked_two_base_chunk():
    """nb = 4, moves (1, 0, 1, 0).  Base 0 at t = 0: window 0..1 (t_0 = -1, t_2 = 2).  Base 1 at t = 2: window 1..3
    (t_3 = T = 4).  The windows overlap at step 1."""
    e = np.array([[0.50, 0.25, 0.00, 0.25],
                  [0.50, 0.00, 0.00, 0.00],
                  [0.00, 0.00, 1.00, 0.00],
                  [0.00, 0.00, 0.50, 0.00]], F32)
    prob, by = ubprob_ref.base_probs(e, np.array([1, 0, 1, 0], bool))
    # base 0: mass (1.0, 0.25, 0, 0.25) / 1.5;  base 1: mass (0.5, 0, 1.5, 0) / 2.0
    assert np.allclose(prob, [[2 / 3, 1 / 6, 0, 1 / 6], [0.25, 0, 0.75, 0]])
    assert by.tolist() == [[170, 42, 0, 42], [64, 0, 192, 0]]
    # a single base taking the whole chunk, and a certain letter: 256 * 1 is binned to 255
    prob, by = ubprob_ref.base_probs(e[:1], np.array([1], bool))
    assert by.tolist() == [[128, 64, 0, 64]]
    prob, by = ubprob_ref.base_probs(e[2:3], np.array([1], bool))
    assert by.tolist() == [[0, 0, 255, 0]]
    assert ubprob_ref.base_windows(np.array([0, 1, 0, 0, 1, 1], bool)) == [(1, 0, 4), (4, 2, 5), (5, 5, 6)]


def test_no_mass_gives_no_information():
    e = np.zeros((5, 6), F32)
    e[4] = 1.0                                                 # mass only outside every window but the last base's
    prob, by = ubprob_ref.base_probs(e, np.array([1, 0, 1, 0, 0], bool))
    assert not by[0].any() and not prob[0].any()              # window 0..1: tot = 0 -> every byte 0
    assert by[1].tolist() == [42] * 6                          # window 1..4: an even split


# ---- host plumbing with a stub model -----------------------------------------------------------------------------------

class _UbStub(_StubModel):
    """The qualities stub of tests/test_qscores.py with letter-probability planes: plane b at base i of a chunk holds
    (first sample digit * 7 + 11 b + i) % 256, so that every plane, chunk and base differs."""

    def __init__(self, alphabet=None):
        super().__init__()
        if alphabet is not None:
            self.alphabet = list(alphabet)
        self.ub_calls = []
        self.seqdist = self

    def reverse_complement(self, scores):
        return scores

    def __call__(self, batch):
        return np.asarray(batch)

    def context(self, chunk_len, n):
        model = self

        class _Ctx:
            @staticmethod
            def decode_ub(scores, alphabet, qscale, qoffset):
                return model._ub_rows(scores)
        return _Ctx()

    def _ub_rows(self, batch):
        seq, lens, q, mv = self._rows(batch, True)
        self.qscore_calls.pop()
        self.ub_calls.append(True)
        n, T = seq.shape
        nb = len(self.alphabet) - 1
        d = (np.abs(np.asarray(batch)[:, 0, 0]) * 10).astype(np.int64)
        probs = np.zeros((n, nb, T), np.uint8)
        k = int(lens[0])
        for b in range(nb):
            probs[:, b, :k] = (d[:, None] * 7 + 11 * b + np.arange(k)[None, :]) % 256
        return seq, lens, q, mv, probs

    def basecall_chunks(self, batch, qscores=False, ub_probs=False):
        return self._ub_rows(batch) if ub_probs else self._rows(batch, qscores)

    def submit_chunks(self, slot, batch, qscores=False, ub_probs=False):
        if not ub_probs:
            return super().submit_chunks(slot, batch, qscores)
        assert slot not in self.busy
        self.busy[slot] = self._ub_rows(batch)
        return ("ctx", slot, np.asarray(batch).shape[0], "ub")


def _run(reads, reverse=False, chunksize=1000, overlap=100, **kw):
    from xna_basecaller_amd.crf.basecall import basecall
    model = _UbStub()
    return model, list(basecall(model, reads, chunksize=chunksize, overlap=overlap, batchsize=4, reverse=reverse, **kw))


def _expected_tags(model, read, chunksize, overlap, reverse):
    """The planes composed independently: chunk the read, the stub's rows per chunk, the reference's stitch per plane,
    the bytes where the stitched sequence holds a base."""
    from xna_basecaller_amd import util
    ch = util.chunk(np.asarray(read.signal, np.float32), chunksize, overlap)
    seq, _, _, _, probs = model._ub_rows(ch)
    n = len(read.signal)
    st_seq = util.stitch(seq, chunksize, overlap, n, model.stride, reverse=reverse)
    called = st_seq != 0
    tags = []
    for b, letter in enumerate(model.alphabet[1:]):
        if letter in "ACGT":
            continue
        pl = util.stitch(np.ascontiguousarray(probs[:, b]), chunksize, overlap, n, model.stride, reverse=reverse)
        tags.append("u%s:B:C," % letter + ",".join(str(int(v)) for v in pl[called]))
    return tags


@pytest.mark.parametrize("reverse", [False, True])
def test_planes_are_stitched_beside_the_bases(reverse):
    reads = [_Read(i, n) for i, n in enumerate([700, 2500, 4100, 1000, 9000])]
    model, out = _run(reads, reverse=reverse, ub_probs=True)
    assert model.ub_calls and set(model.qscore_calls) <= {True}
    for read, res in out:
        seq = res["sequence"]
        assert len(seq) > 0
        assert [t.split(":")[0] for t in res["mods"]] == ["uX", "uY"]
        for tag in res["mods"]:
            assert tag.startswith("u") and tag[2:7] == ":B:C,"
            assert len(tag[7:].split(",")) == len(seq)
        assert res["mods"] == _expected_tags(model, read, 1000, 100, reverse)
        # without --qscores the quality string stays the placeholder
        assert res["qstring"] == "O" * len(seq) and res["mean_qscore"] == 40.0


def test_no_mods_and_unchanged_results_without_the_flag():
    reads = [_Read(i, n) for i, n in enumerate([700, 2500, 4100])]
    _, plain = _run(reads)
    for _, res in plain:
        assert "mods" not in res
    model, ub = _run(reads, ub_probs=True)
    _, ubq = _run(reads, ub_probs=True, qscores=True)
    _, q = _run(reads, qscores=True)
    for (_, a), (_, b), (_, c), (_, d) in zip(plain, ub, ubq, q):
        assert a["sequence"] == b["sequence"] == c["sequence"] == d["sequence"]
        assert a["qstring"] == b["qstring"] and c["qstring"] == d["qstring"]
        assert b["mods"] == c["mods"] and "mods" not in d


def test_compute_scores_with_ub_probs_returns_the_planes():
    from xna_basecaller_amd.crf.basecall import compute_scores
    model = _UbStub()
    batch = np.random.default_rng(3).standard_normal((3, 1, 500)).astype(np.float32)
    res = compute_scores(model, batch, ub_probs=True)
    assert set(res) == {"qstring", "sequence", "moves", "probs"}
    assert res["probs"].shape == (3, 6, 100) and res["probs"].dtype == np.uint8
    assert not res["moves"].any()                              # placeholders without qscores
    resq = compute_scores(model, batch, ub_probs=True, qscores=True)
    assert res["moves"].dtype == bool and resq["moves"].any()
    assert np.array_equal(res["probs"], resq["probs"])


def _records(mode, results):
    from xna_basecaller_amd.io import Writer

    class R:
        def __init__(self, rid):
            self.read_id, self.run_id, self.filename, self.channel, self.mux = rid, "run", "f.fast5", 1, 1
            self.start, self.duration, self.template_start, self.template_duration = 0, 1, 0, 1
            self.signal = np.zeros(10, np.float32)

        def tagdata(self):
            return ["mx:i:1"]

    fd = io.StringIO()
    w = Writer(mode, ((R(rid), res) for rid, res in results), fd=fd, group_key="m",
               summary=os.devnull)
    w.run()
    return fd.getvalue()


def test_tags_in_fastq_and_sam_lines():
    reads = [_Read(i, n) for i, n in enumerate([2500, 4100])]
    model, out = _run(reads, ub_probs=True)
    results = [(r.read_id, res) for r, res in out]
    fq = _records("wfq", results).split("\n")
    sam = [l for l in _records("w", results).split("\n") if l and not l.startswith("@")]
    for k, (rid, res) in enumerate(results):
        hdr = fq[4 * k].split("\t")
        assert hdr[-2:] == res["mods"] and hdr[-3] == "mx:i:1"
        rec = sam[k].split("\t")
        assert rec[0] == rid and rec[-2:] == res["mods"]


def test_cli_parses_ub_probs_and_refuses_models_without_it():
    from types import SimpleNamespace
    from xna_basecaller_amd.cli.basecaller import argparser, ub_probs_refusal
    p = argparser()
    assert p.parse_args(["m", "r", "--ub-probs"]).ub_probs is True
    assert p.parse_args(["m", "r"]).ub_probs is False
    a = p.parse_args(["m", "r", "--ub-probs", "--qscores"])
    assert a.ub_probs and a.qscores
    assert ub_probs_refusal(_UbStub()) is None
    assert "outside A, C, G, T" in ub_probs_refusal(_UbStub("NACGT"))
    beam = _UbStub()
    beam.encoder = [SimpleNamespace(expand_blanks=False, blank_score=2.0)]
    assert "beam" in ub_probs_refusal(beam)
    from xna_basecaller_amd.crf.basecall import compute_scores
    with pytest.raises(ValueError):
        compute_scores(beam, np.zeros((1, 1, 500), np.float32), ub_probs=True)


# ---- the torchrun gather ---------------------------------------------------------------------------------------------

WORKER = r'''
import os, sys
sys.path.insert(0, os.environ["XB_ROOT"])
import numpy as np
from xna_basecaller_amd import dist as xd
rank, world = xd.init_from_env(backend="gloo")
from xna_basecaller_amd.cli.basecaller import _gathered_results, READ_FIELDS
class FakeRead:
    def __init__(self, i):
        self.index = i
        for k in READ_FIELDS: setattr(self, k, "%s%d" % (k[:2], i))
        self.signal = np.zeros(100 + i, np.float32)
    def tagdata(self): return ["mx:i:%d" % self.index]
class FakeLoader: total = 17
def mods(i):
    return ["uX:B:C," + ",".join(str((i * 3 + j) % 256) for j in range(1 + i % 4)),
            "uY:B:C," + ",".join(str((i * 5 + j) % 256) for j in range(1 + i % 4))]
def local():
    for i in range(rank, 17, 2):
        res = {"sequence": "ACGX"[: 1 + i % 4], "qstring": "O" * (1 + i % 4)}
        if i % 5:
            res["mods"] = mods(i)
        yield FakeRead(i), res
got = list(_gathered_results(local(), FakeLoader, rank, world, window=3))
if rank == 0:
    assert [r.read_id for r, _ in got] == ["re%d" % i for i in range(17)]
    for i, (r, res) in enumerate(got):
        assert res["sequence"] == "ACGX"[: 1 + i % 4]
        if i % 5:
            assert res["mods"] == mods(i)
        else:
            assert "mods" not in res
else:
    assert got == []
xd.barrier()
print("rank", rank, "ok")
'''


def _free_port():
    with socket.socket() as s:
        s.bind(("127.0.0.1", 0))
        return s.getsockname()[1]


def test_tags_survive_the_world2_gather(tmp_path):
    script = tmp_path / "worker.py"
    script.write_text(WORKER)
    port = str(_free_port())
    procs = []
    for r in range(2):
        env = dict(os.environ, RANK=str(r), LOCAL_RANK=str(r), WORLD_SIZE="2", MASTER_ADDR="127.0.0.1",
                   MASTER_PORT=port, XB_ROOT=ROOT)
        procs.append(subprocess.Popen([sys.executable, str(script)], env=env, stdout=subprocess.PIPE,
                                      stderr=subprocess.STDOUT))
    try:
        outs = [p.communicate(timeout=240)[0].decode() for p in procs]
    finally:
        for p in procs:
            if p.poll() is None:
                p.kill()
    for r, (p, o) in enumerate(zip(procs, outs)):
        assert p.returncode == 0, o
        assert "rank %d ok" % r in o
