"""GPU: the Viterbi decode family at every state length the C ABI accepts other than 3 -- (n_base, state_len) = (4, 2),
(5, 2), (6, 2), (4, 4), (5, 4), (4, 5) -- bit for bit against the oracle and the restatements built on it
(tests/qscore_ref.py, tests/ubprob_ref.py): xb_decode, xb_decode_q, xb_decode_ub, xb_crf_logz and xb_crf_scans, with and
without the blank column, with XB_DECODE_LPS unset, 1 and 2.

Which case runs which workgroup size of launch_nb_lps (S = n_base^state_len states, need = lanes per state x S; the
library's own choice is 2 lanes while 2 S <= 256, the scans always run 1 lane):
    64    (4, 2) S 16 and (5, 2) S 25 with 1 or 2 lanes; (6, 2) S 36 with 1 lane
    128   (6, 2) with 2 lanes (unset or XB_DECODE_LPS=2)
    256   (4, 4) S 256 with 1 lane (unset or XB_DECODE_LPS=1)
    640   (4, 4) with XB_DECODE_LPS=2 (512 lanes in 640 threads); (5, 4) S 625 with 1 lane
    1024  (4, 5) S 1024 with 1 lane; at T 2000 the four-wide row loads no longer fit the LDS and are dropped
    (128 / 256 / 448 at state_len 3 are run by tests/test_gpu_decode.py.)
XB_DECODE_LPS=2 is ignored where 2 S > 1024, at (5, 4) and (4, 5): those runs pin that the ignored override changes no
bit and raises no error."""
import functools

import numpy as np
import pytest

import oracle
import ubprob_ref
from conftest import random_scores
from pairs import NEW_PAIRS
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu

QS, QO = 0.9722, 0.3498          # the shipped model's [qscore] section
LARGE = [(5, 4), (4, 5)]
SHAPES = [(nb, sl, T) for nb, sl in NEW_PAIRS for T in (1, 2, 63, 64, 65, 203)] + [(nb, sl, 2000) for nb, sl in LARGE]
SCAN_SUBSETS = (("alpha", "beta", "logz", "post"), ("post",), ("beta",), ("alpha", "logz"), ("logz", "post"))


def _ctx(nb, sl, T, N):
    return _lib.Context(0, nb, sl, 32, 19, 5, 5.0, 2.0, T * 5, N)


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def _reference(sc, nb, sl, with_blank):
    """Everything the decode family returns, from the oracle and the two restatements, computed once per score tensor."""
    alphabet = "NACGTXY"[:nb + 1]
    blank = None if with_blank else 2.0
    r = ubprob_ref.decode_ub(sc, nb, alphabet, sl=sl, blank_score=blank, qscale=QS, qoffset=QO)
    labels = oracle.decode(sc, nb, sl, blank_score=blank)["labels"]
    seq, _, lens = oracle.pack(labels, alphabet)
    out = {"labels": labels, "seq": seq, "lens": lens, "qstring": r["qstring"], "moves": r["moves"], "probs": r["probs"],
           "post": r["post"], "alpha": r["oracle"]["alpha"], "beta": r["oracle"]["beta"], "logz": r["oracle"]["logz"]}
    assert np.array_equal(r["seq"], seq) and np.array_equal(r["seq_len"], lens)     # the restatements call the oracle's path
    for v in out.values():
        v.setflags(write=False)
    return out


@functools.lru_cache(maxsize=3)
def _random_case(nb, sl, T, with_blank):
    sc = random_scores(T, 3 if T < 2000 else 2, nb, sl=sl, seed=100 * sl + 10 * nb + T, with_blank=with_blank)
    sc.setflags(write=False)
    return sc, _reference(sc, nb, sl, with_blank)


def _check_family(ctx, sc, ref, nb, with_blank, subsets=SCAN_SUBSETS):
    alphabet = "NACGTXY"[:nb + 1]
    T, N, _ = sc.shape

    def check_plain():
        seq, lens, labels = ctx.decode(sc, alphabet, has_blank=with_blank, want_labels=True)
        assert np.array_equal(labels, ref["labels"]), "label mismatches: %d of %d at (chunk, t) %s" % (
            (labels != ref["labels"]).sum(), labels.size, np.argwhere(labels != ref["labels"])[:8].tolist())
        assert np.array_equal(lens, ref["lens"]) and np.array_equal(seq, ref["seq"])

    check_plain()
    seq, lens, q, mv = ctx.decode_q(sc, alphabet, QS, QO, has_blank=with_blank)
    assert np.array_equal(seq, ref["seq"]) and np.array_equal(lens, ref["lens"])
    assert np.array_equal(mv, ref["moves"]), np.argwhere(mv != ref["moves"])[:8].tolist()
    assert np.array_equal(q, ref["qstring"]), np.argwhere(q != ref["qstring"])[:8].tolist()
    seq, lens, q, mv, pr = ctx.decode_ub(sc, alphabet, QS, QO, has_blank=with_blank)
    assert np.array_equal(seq, ref["seq"]) and np.array_equal(lens, ref["lens"])
    assert np.array_equal(mv, ref["moves"]) and np.array_equal(q, ref["qstring"])
    assert np.array_equal(pr, ref["probs"]), np.argwhere(pr != ref["probs"])[:8].tolist()
    lz = ctx.crf_logz(sc, has_blank=with_blank)
    assert lz.dtype == np.float32 and np.array_equal(_bits(lz), _bits(ref["logz"]))
    for want in subsets:
        got = ctx.crf_scans(sc, want=want, has_blank=with_blank)
        for k in want:
            assert got[k].shape == ref[k].shape, (want, k)
            assert np.array_equal(_bits(got[k]), _bits(ref[k])), (want, k, np.abs(got[k] - ref[k]).max())
    check_plain()                                          # the scans share the decode's workspaces


@pytest.mark.parametrize("lps", [0, 1, 2])
@pytest.mark.parametrize("with_blank", [True, False])
@pytest.mark.parametrize("nb,sl,T", SHAPES)
def test_decode_family_bit_exact(nb, sl, T, with_blank, lps, monkeypatch):
    """T 1, 2, 63, 64, 65, 203: the boundaries of the 64-step label finalisation and of the prefetch rings; T 2000 at the
    two largest state counts: the largest LDS carve (5 S floats, the label and path rows, 2 S more for decode_ub)."""
    if lps:
        monkeypatch.setenv("XB_DECODE_LPS", str(lps))
    sc, ref = _random_case(nb, sl, T, with_blank)
    ctx = _ctx(nb, sl, max(T, 8), sc.shape[1])
    _check_family(ctx, sc, ref, nb, with_blank)
    ctx.close()


@pytest.mark.parametrize("lps", [0, 1, 2])
@pytest.mark.parametrize("nb,sl", [(6, 2), (4, 4), (4, 5)])
def test_ties_and_extremes(nb, sl, lps, monkeypatch):
    """All-zero scores (every path ties: the lowest flat index wins, state 0 through its blank edge, at every workgroup
    size), a coarse grid, x 8 scores (deep underflow) and a dominant blank."""
    if lps:
        monkeypatch.setenv("XB_DECODE_LPS", str(lps))
    T, N = 50, 4
    S, E = nb ** sl, nb + 1
    ctx = _ctx(nb, sl, T, N)
    zero = np.zeros((T, N, S * E), np.float32)
    ref = _reference(zero, nb, sl, True)
    assert not ref["labels"].any() and not ref["lens"].any()
    _check_family(ctx, zero, ref, nb, True, subsets=SCAN_SUBSETS[:1])
    sc = random_scores(T, N, nb, sl=sl, seed=1)
    sc[:, 1] = np.round(sc[:, 1])
    sc[:, 2] *= 8.0
    sc[:, 3] = -5.0
    sc[:, 3].reshape(T, S, E)[:, :, 0] = 5.0
    ref = _reference(sc, nb, sl, True)
    assert ref["lens"][3] == 0 and ref["lens"][:3].all()
    _check_family(ctx, sc, ref, nb, True, subsets=SCAN_SUBSETS[:1])
    ctx.close()


@pytest.mark.parametrize("with_blank", [True, False])
@pytest.mark.parametrize("nb,sl", [(5, 2), (5, 4)])
def test_device_pointer_forms(nb, sl, with_blank):
    """xb_decode_dev and xb_crf_scans_dev where the padded posterior row ldq = (S E + 3) & ~3 is longer than S E."""
    import torch
    T = 65
    S, E = nb ** sl, nb + 1
    ldq = (S * E + 3) & ~3
    assert ldq != S * E
    sc, ref = _random_case(nb, sl, T, with_blank)
    N = sc.shape[1]
    ctx = _ctx(nb, sl, T, N)
    d_sc = torch.from_numpy(sc.copy()).cuda()
    d_lab = torch.zeros((N, T), dtype=torch.int8, device="cuda")
    d_seq = torch.zeros((N, T), dtype=torch.int8, device="cuda")
    d_len = torch.zeros((N,), dtype=torch.int32, device="cuda")
    d_a = torch.zeros((T + 1, N, S), dtype=torch.float32, device="cuda")
    d_b = torch.zeros((T + 1, N, S), dtype=torch.float32, device="cuda")
    d_lz = torch.zeros((N,), dtype=torch.float32, device="cuda")
    d_p = torch.full((T, N, ldq), -7.0, dtype=torch.float32, device="cuda")
    torch.cuda.synchronize()
    ctx.crf_scans_dev(d_sc.data_ptr(), T, N, with_blank, d_a.data_ptr(), d_b.data_ptr(), d_lz.data_ptr(), d_p.data_ptr())
    ctx.decode_dev(d_sc.data_ptr(), T, N, with_blank, "NACGTXY"[:nb + 1], d_lab.data_ptr(), d_seq.data_ptr(), d_len.data_ptr())
    ctx.synchronize()
    assert np.array_equal(_bits(d_a.cpu().numpy()), _bits(ref["alpha"]))
    assert np.array_equal(_bits(d_b.cpu().numpy()), _bits(ref["beta"]))
    assert np.array_equal(_bits(d_lz.cpu().numpy()), _bits(ref["logz"]))
    assert np.array_equal(_bits(d_p.cpu().numpy()[:, :, :S * E]), _bits(ref["post"]))
    assert np.array_equal(d_lab.cpu().numpy(), ref["labels"])
    assert np.array_equal(d_seq.cpu().numpy(), ref["seq"]) and np.array_equal(d_len.cpu().numpy(), ref["lens"])
    ctx.close()
