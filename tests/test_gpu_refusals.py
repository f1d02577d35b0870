"""GPU: what the entry points on chunks and score tensors refuse (tests/refusal_cases.py) -- the exact status and the exact text of
xb_last_error, through the C ABI itself (Context's wrappers refuse bad shapes before the library sees them), on one small context
without weights and one with.  A refused call leaves the context as it found it: the last test decodes on both against the oracle."""
import ctypes as C

import numpy as np
import pytest
import torch

import oracle
import refusal_cases as rc
from conftest import random_scores
from xna_basecaller_amd import _lib
from xna_basecaller_amd.synthetic import seeded_weights

pytestmark = pytest.mark.gpu

BUF_BYTES = 4 << 20           # more than any argument of a call on this context holds, should a call be accepted after all


def _context(loaded):
    ctx = _lib.Context(0, rc.NB, rc.SL, rc.F, rc.WIN, rc.STRIDE, rc.SCALE, rc.BLANK, rc.CHUNK, rc.MAX_BATCH)
    if loaded:
        ctx.load_state_dict(seeded_weights(rc.F, rc.NB))
    return ctx


class Buffers:
    """The good call's pointers: zeros on either side, and a label batch (rows of LT labels 1 .. n_base, full lengths)."""

    def __init__(self):
        self.host = np.zeros(BUF_BYTES, np.uint8)
        self.dev = torch.zeros(BUF_BYTES, dtype=torch.uint8, device="cuda")
        self.labels = {}
        for fault in (None, rc.SHORT_LENGTH, rc.HIGH_LABEL):
            targets = (1 + np.arange(rc.MAX_BATCH * rc.LT) % rc.NB).reshape(rc.MAX_BATCH, rc.LT)
            lengths = np.full(rc.MAX_BATCH, rc.LT, np.int32)
            if fault == rc.SHORT_LENGTH:
                lengths[0] = rc.SL - 1
            if fault == rc.HIGH_LABEL:
                targets[0, 0] = rc.NB + 1
            self.labels[fault] = (targets.astype(np.int32), targets.astype(np.uint8), lengths)
        self.dev_labels = tuple(torch.from_numpy(a).cuda() for a in self.labels[None][1:])

    def pointer(self, fn, name, value):
        if value is None:
            return None
        if name in ("targets", "lengths"):
            if fn.endswith("_dev"):
                return self.dev_labels[name == "lengths"].data_ptr()
            t32, t8, lengths = self.labels[value if value in (rc.SHORT_LENGTH, rc.HIGH_LABEL) else None]
            return (lengths if name == "lengths" else (t32 if fn in rc.INT32_LABELS else t8)).ctypes.data
        return self.dev.data_ptr() if fn.endswith("_dev") else self.host.ctypes.data

    def args(self, fn, overrides):
        out = []
        for name, value in rc.good(fn).items():
            value = overrides.get(name, value)
            if name in rc.SCALARS:
                out.append(C.c_float(value) if name in rc.FLOATS else value)
            else:
                out.append(self.pointer(fn, name, value))
        return out


@pytest.fixture(scope="module")
def world():
    w = {"bare": _context(False), "loaded": _context(True), "bufs": Buffers()}
    yield w
    w["bare"].close()
    w["loaded"].close()


def _call(ctx, bufs, r):
    code = getattr(ctx.lib, r.fn)(ctx.h, *bufs.args(r.fn, r.args))
    return code, (ctx.lib.xb_last_error(ctx.h) or b"").decode()


@pytest.mark.parametrize("r", rc.ROWS[:rc.SINGLE], ids=rc.row_id)
def test_single_fault(world, r):
    for which in ("bare", "loaded") if r.ctx == "both" else (r.ctx,):
        code, message = _call(world[which], world["bufs"], r)
        assert (code, message) == (r.code, r.message), which


@pytest.mark.parametrize("r", rc.ROWS[rc.SINGLE:], ids=rc.row_id)
def test_double_fault(world, r):
    for which in ("bare", "loaded") if r.ctx == "both" else (r.ctx,):
        code, message = _call(world[which], world["bufs"], r)
        assert code == r.code and message in r.message, (which, code, message)


@pytest.mark.parametrize("fn", sorted(rc.SIGNATURES))
def test_null_context(world, fn):
    assert getattr(world["loaded"].lib, fn)(None, *world["bufs"].args(fn, {})) == _lib.XB_ERR_INVALID


def test_contexts_still_decode(world):
    """After every refusal above (or none, when run alone): xb_decode of 2 chunks at T = 8 against the oracle, on both contexts."""
    alphabet = rc.ALPHABET.decode()
    sc = random_scores(8, 2, rc.NB, seed=5)
    ref = oracle.decode(sc, rc.NB, rc.SL)["labels"]
    rseq, _, rlens = oracle.pack(ref, alphabet)
    for which in ("bare", "loaded"):
        ctx = world[which]
        assert ctx.lib.xb_synchronize(ctx.h) == _lib.XB_OK
        seq, lens, labels = ctx.decode(sc, alphabet, want_labels=True)
        assert np.array_equal(labels, ref) and np.array_equal(lens, rlens) and np.array_equal(seq, rseq), which


def test_refusal_beside_a_held_call():
    """A held-back xb_basecall_chunks_dev, then a refused xb_decode_dev (T too large), then xb_synchronize: the held call gives what
    it gives on a context without pairing -- whether the refusal comes before or after the held call is launched."""
    n = 2
    x = torch.randn((n, rc.CHUNK), dtype=torch.float32, device="cuda", generator=torch.Generator(device="cuda").manual_seed(11))
    got = []
    for paired in (False, True):
        ctx = _context(True)
        if paired:
            ctx.reserve_pairing()
            assert ctx.pairing_active()
        seq = torch.zeros((n, ctx.T), dtype=torch.int8, device="cuda")
        lens = torch.zeros((n,), dtype=torch.int32, device="cuda")
        ctx.basecall_chunks_dev(x.data_ptr(), n, rc.ALPHABET.decode(), seq.data_ptr(), lens.data_ptr())
        if paired:
            scores = torch.zeros((rc.T + 1, n, ctx.C_blank), dtype=torch.float32, device="cuda")
            code = ctx.lib.xb_decode_dev(ctx.h, scores.data_ptr(), rc.T + 1, n, 1, rc.ALPHABET, None, seq.data_ptr(), lens.data_ptr())
            assert (code, ctx.lib.xb_last_error(ctx.h).decode()) == (rc.INVALID, rc.steps(rc.T + 1))
        assert ctx.lib.xb_synchronize(ctx.h) == _lib.XB_OK
        got.append((seq.cpu().numpy(), lens.cpu().numpy()))
        ctx.close()
    assert np.array_equal(got[0][1], got[1][1]) and np.array_equal(got[0][0], got[1][0])
