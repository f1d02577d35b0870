"""GPU: xb_beam_search / xb_beam_search_dev / xb_basecall_chunks_beam against the oracle, bit for bit (moves, sequence, qstring,
and the score's 32 bits), on the cases of tests/beam_cases.py: every (n_base, state_len) a context takes at the edges of the
64-block trace-back tile and both parities of the double buffer, with and without the blank column (both LDS-DMA widths, every
row remainder, the largest LDS carve); the no-cut rows that take the one-merge-at-a-time branch; widths 1..31 and cuts from 1 up;
all-equal, integer, steep, blank-only and single-path scores.  tests/test_beam_cases_host.py proves on the CPU that each case
reaches the branches it is named for.  Then what no single call shows: one context through calls of different width, cut and
length (stale history), the device-pointer form's output planes, independence of a chunk from its batch, and the fused call
against the oracle (so far it was compared with another GPU call only).

No case here has a beam_cut inside (0, 1) or a non-finite score: the first is refused (tests/refusal_cases.py), the second is
the caller's to avoid (include/xna_basecaller.h)."""
import functools

import numpy as np
import pytest

import beam_cases as bc
import oracle
from xna_basecaller_amd import _lib
from xna_basecaller_amd.synthetic import peaky_weights

pytestmark = pytest.mark.gpu

KEYS = ("moves", "sequence", "qstring", "score")
SENTINEL = 0x5A


@functools.lru_cache(maxsize=None)
def _ref(name):
    c = bc.BY_NAME[name]
    return oracle.beam_search(bc.scores(c), bc.ALPHA[c.nb], c.sl, c.W, c.cut, c.scale, c.offset, blank_score=bc.BLANK)


def _context(nb, sl, T, N):
    return _lib.Context(0, nb, sl, 32, 19, 5, 5.0, bc.BLANK, T * 5, N)


def _same(got, ref, what=""):
    for k in KEYS:
        g, r = got[k], ref[k]
        if k == "score":
            g, r = g.view(np.uint32), r.view(np.uint32)
        assert g.dtype == r.dtype and np.array_equal(g, r), (what, k)


def _call(ctx, c):
    return ctx.beam_search(bc.scores(c), bc.ALPHA[c.nb], beam_width=c.W, beam_cut=c.cut, scale=c.scale, offset=c.offset)


@pytest.mark.parametrize("name", [c.name for c in bc.CASES])
def test_case_is_the_oracles_bit_for_bit(name):
    c = bc.BY_NAME[name]
    ctx = _context(c.nb, c.sl, c.T, c.N)
    try:
        assert ctx.T == c.T
        _same(_call(ctx, c), _ref(name), name)
    finally:
        ctx.close()


def test_one_context_through_widths_cuts_and_lengths():
    """No pristine context in between: a call finds the history, path and probability planes of the calls before it, written at
    another width and another row pitch."""
    order = ("width-gauss-W31", "nocut-4-sl2-T65", "width-gauss-W1", "cut-gauss-1", "nocut-4-sl2-T20", "sweep-4-sl2-T63-const",
             "sweep-4-sl2-T2-blank", "width-gauss-W2", "sweep-4-sl2-T1-const", "nocut-4-sl2-T65")
    cases = [bc.BY_NAME[n] for n in order]
    assert {(c.nb, c.sl, c.N) for c in cases} == {(4, 2, 3)}
    assert (cases[1].W, cases[1].cut, cases[2].W) == (32, 0.0, 1) and cases[4].T < cases[2].T
    ctx = _context(4, 2, max(c.T for c in cases), 3)
    try:
        for c in cases:
            _same(_call(ctx, c), _ref(c.name), c.name)
    finally:
        ctx.close()


@pytest.mark.parametrize("nb,sl", [(5, 4), (6, 2)])
@pytest.mark.parametrize("form", ["const", "blank"])
def test_device_pointer_form_writes_its_rows_and_no_more(nb, sl, form):
    import torch
    c = bc.BY_NAME["sweep-%d-sl%d-T65-%s" % (nb, sl, form)]
    ref = _ref(c.name)
    ctx = _context(nb, sl, c.T, c.N + 1)
    try:
        d_sc = torch.from_numpy(bc.scores(c)).cuda()
        planes = [torch.full((c.N + 1, c.T), SENTINEL, dtype=dt, device="cuda") for dt in (torch.int8, torch.int8, torch.uint8)]
        d_score = torch.full((c.N + 1,), -123.0, dtype=torch.float32, device="cuda")
        ctx.beam_search_dev(d_sc.data_ptr(), c.T, c.N, c.with_blank, bc.ALPHA[nb], planes[0].data_ptr(), planes[1].data_ptr(),
                            planes[2].data_ptr(), d_score.data_ptr(), beam_width=c.W, beam_cut=c.cut, scale=c.scale, offset=c.offset)
        ctx.synchronize()
        seq, q, mv = (p.cpu().numpy() for p in planes)
        score = d_score.cpu().numpy()
        _same({"sequence": seq[:c.N], "qstring": q[:c.N], "moves": mv[:c.N], "score": score[:c.N]}, ref, c.name)
        assert np.all(seq[c.N] == SENTINEL) and np.all(q[c.N] == SENTINEL) and np.all(mv[c.N] == SENTINEL) and score[c.N] == -123.0
    finally:
        ctx.close()


def test_a_chunk_does_not_depend_on_its_batch():
    nb, sl, T, N = 4, 3, 129, 40
    steps, blank = bc.ridge(np.random.default_rng(77), nb, sl, T, N)
    sc = np.ascontiguousarray(steps).reshape(T, N, -1)
    ctx = _context(nb, sl, T, N)
    try:
        whole = ctx.beam_search(sc, bc.ALPHA[nb], scale=bc.QS, offset=bc.QO)
        part = ctx.beam_search(np.ascontiguousarray(sc[:, 7:29]), bc.ALPHA[nb], scale=bc.QS, offset=bc.QO)
    finally:
        ctx.close()
    _same(part, {k: whole[k][7:29] for k in KEYS}, "chunks 7..28 alone")
    ref = oracle.beam_search(np.ascontiguousarray(sc[:, :6]), bc.ALPHA[nb], sl, scale=bc.QS, offset=bc.QO, blank_score=bc.BLANK)
    _same({k: whole[k][:6] for k in KEYS}, ref, "first 6 chunks")
    bases = whole["moves"].sum(1)
    assert bases.min() >= 0.3 * T and bases.max() <= 0.7 * T and len({m.tobytes() for m in whole["moves"]}) == N


# (nb, state_len, winlen, stride, features, L, N): the geometries of tests/test_gpu_geometry_calls.py
GEOMETRIES = [(4, 4, 9, 6, 64, 1002, 9), (5, 2, 5, 3, 32, 600, 5)]


@pytest.mark.parametrize("nb,sl,W,ST,F,L,N", GEOMETRIES)
def test_fused_call_is_the_oracles_on_the_encoders_scores(nb, sl, W, ST, F, L, N):
    """At (5, 2) the fused call's rows are padded (125 -> 128 floats): the 16-byte row path beside a 4-byte back guide."""
    alphabet = bc.ALPHA[nb]
    ctx = _lib.Context(0, nb, sl, F, W, ST, 5.0, bc.BLANK, L, N, precision=_lib.XB_PREC_MIXED)
    try:
        ctx.load_state_dict(peaky_weights(F, nb, seed=F + nb, state_len=sl, winlen=W))
        x = np.random.default_rng(F + W).standard_normal((N, L)).astype(np.float32)
        scores = ctx.encode(x, expand_blanks=False)
        assert scores.shape == (ctx.T, N, nb ** (sl + 1)) and np.all(np.isfinite(scores))
        fused = ctx.basecall_chunks_beam(x, alphabet, scale=bc.QS, offset=bc.QO)
    finally:
        ctx.close()
    ref = oracle.beam_search(scores, alphabet, sl, scale=bc.QS, offset=bc.QO, blank_score=bc.BLANK)
    _same(fused, ref)
    assert ref["moves"].sum(1).min() > 1
