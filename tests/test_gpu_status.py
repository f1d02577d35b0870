"""GPU: the two device status words of a context (csrc/xb_status.h) and the shared call prologue.

A loss call whose device-resident lengths are bad leaves its refusal in the data word until the next synchronising call.  The
persistent recurrence polls the sync word only, so the encoder passes that follow compute what they compute alone, a
pipelined batch is collected as usual, and the refusal is reported once, as XB_ERR_INVALID with the loss's text.  And a _dev
entry names its result stream after it has launched a held-back call, not before.

The geometry is tests/test_gpu_valloss.py's refusal case at the smallest feature size whose recurrence is a persistent launch
of more than one workgroup per group -- asserted through the planner, so that the kernel's wait loop is there.  Nothing here
provokes a timeout: the sync-lost report is covered on the CPU (tests/test_status_host.py)."""
import functools

import numpy as np
import pytest
import torch

import host_logic
from conftest import encoder_shapes, seeded_state_dict
from ctc_wide_cases import BLANK, label_rows, loss_reference
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu

NB, SL, T, N, LT, STRIDE, WINLEN = 5, 3, 40, 4, 14, 5, 19
ALPHABET = "NACGTX"
LOSS_TEXT = "xb_ctc_loss: a target length outside [state_len, Lt] or a label above n_base inside it"
FEATURES = (32, 64, 96, 128, 256, 384, 512, 768)           # what xb_ctx_create accepts


def _members(planner, F, cu_count):
    """Workgroups per chunk group of the recurrence at F features, read off the planner: a persistent launch needs all of a
    group's workgroups on one XCD's CUs, so the smallest cu_count / 8 at which the plan turns persistent is their number."""
    for per_xcd in range(1, cu_count // 8 + 1):
        plan, _ = planner.plan(F, N, T, 8 * per_xcd)
        if plan.error == 0 and plan.mode == 2:
            return per_xcd
    return None


@functools.lru_cache(maxsize=None)
def _features():
    """The smallest feature size whose recurrence, on this device, is a persistent launch with more than one workgroup per
    group (whose members therefore wait for each other)."""
    cu_count = torch.cuda.get_device_properties(0).multi_processor_count
    planner = host_logic.Planner()
    for field, value in host_logic.knobs_from_env().items():   # the knobs a context created here gets
        setattr(planner.q.knobs, field, value)
    for F in FEATURES:
        plan, launches = planner.plan(F, N, T, cu_count)
        members = _members(planner, F, cu_count)
        if plan.error == 0 and plan.mode == 2 and members is not None and members > 1:
            assert launches is not None and len(launches) >= 1
            return F
    raise AssertionError("no feature size gives a persistent launch with more than one workgroup per group")


@functools.lru_cache(maxsize=None)
def _inputs():
    F = _features()
    keys, shapes = encoder_shapes(F, NB)
    sd = seeded_state_dict(keys, shapes, seed=5)
    x = np.random.default_rng(9).standard_normal((N, T * STRIDE)).astype(np.float32)
    targets, lens = label_rows(np.random.default_rng(1), N, LT, NB, SL, dtype=np.uint8)
    return sd, x, targets, lens.astype(np.int32)


def _context():
    ctx = _lib.Context(0, NB, SL, _features(), WINLEN, STRIDE, 5.0, BLANK, T * STRIDE, N)
    assert ctx.T == T
    ctx.load_state_dict(_inputs()[0])
    return ctx


class _Device:
    """The device side of one context: the inputs, and outputs that every pass overwrites."""

    def __init__(self, ctx):
        _, x, targets, lens = _inputs()
        dev = torch.device("cuda", 0)
        bad = lens.copy()
        bad[2] = LT + 1
        self.ctx = ctx
        self.x = torch.from_numpy(x).to(dev)
        self.targets, self.lens, self.bad_lens = (torch.from_numpy(a).to(dev) for a in (targets, lens, bad))
        self.scores = torch.zeros((T, N, ctx.C_noblank), dtype=torch.float32, device=dev)
        self.loss_in = torch.zeros_like(self.scores)            # the scores the loss calls read: the reference's, never rewritten
        self.seq = torch.zeros((N, T), dtype=torch.int8, device=dev)
        self.len = torch.zeros((N,), dtype=torch.int32, device=dev)
        self.loss = torch.zeros((N,), dtype=torch.float32, device=dev)
        torch.cuda.synchronize()

    def encode(self):
        self.ctx.encode_dev(self.x.data_ptr(), N, False, self.scores.data_ptr())

    def basecall(self):
        self.ctx.basecall_chunks_dev(self.x.data_ptr(), N, ALPHABET, self.seq.data_ptr(), self.len.data_ptr())

    def loss_call(self, lens):
        self.ctx.ctc_loss_dev(self.loss_in.data_ptr(), T, N, False, self.targets.data_ptr(), LT, lens.data_ptr(), self.loss.data_ptr())

    def clear(self):
        for t in (self.scores, self.seq, self.len):
            t.zero_()
        torch.cuda.synchronize()


def _reference(ctx, d):
    """Clean input on a clean context: the scores of encode_dev, the host call's sequences and lengths, the loss of those scores."""
    _, x, targets, lens = _inputs()
    d.encode()
    ctx.synchronize()
    scores = d.scores.cpu().numpy()
    d.loss_in.copy_(d.scores)
    torch.cuda.synchronize()
    seq, slen = ctx.basecall_chunks(x, ALPHABET)
    d.loss_call(d.lens)
    ctx.synchronize()
    loss = d.loss.cpu().numpy()
    want, _ = loss_reference(ctx, scores, targets, lens, NB, SL, False)
    assert np.array_equal(loss, want)
    assert slen.min() >= 0 and np.abs(scores).max() > 0
    return scores, seq, slen, loss


def _refused_once(ctx):
    with pytest.raises(_lib.XbError) as e:
        ctx.synchronize()
    assert e.value.code == _lib.XB_ERR_INVALID and LOSS_TEXT in str(e.value)
    ctx.synchronize()                                           # reported once: the second one is clean


def test_a_refused_label_does_not_disturb_the_next_pass():
    ctx = _context()
    d = _Device(ctx)
    scores, seq, slen, loss = _reference(ctx, d)
    d.clear()
    d.loss_call(d.bad_lens)                                     # not synchronised: the refusal stays in the data word
    d.encode()
    d.basecall()
    _refused_once(ctx)
    assert d.scores.cpu().numpy().tobytes() == scores.tobytes()
    assert d.seq.cpu().numpy().tobytes() == seq.tobytes() and d.len.cpu().numpy().tobytes() == slen.tobytes()
    d.loss_call(d.lens)
    ctx.synchronize()
    assert d.loss.cpu().numpy().tobytes() == loss.tobytes()
    ctx.close()


def test_the_pipeline_is_not_failed_by_a_validation_bit():
    ctx = _context()
    d = _Device(ctx)
    _, seq, slen, _ = _reference(ctx, d)
    d.loss_call(d.bad_lens)
    assert ctx.submit_chunks(0, _inputs()[1].copy(), ALPHABET) == N
    got_seq, got_len = ctx.collect_chunks(0, N)
    assert got_seq.tobytes() == seq.tobytes() and got_len.tobytes() == slen.tobytes()
    _refused_once(ctx)
    ctx.close()


@pytest.mark.parametrize("decode_async", [0, 1])
def test_result_stream_after_a_held_call(decode_async, monkeypatch):
    """With XB_DECODE_ASYNC=1 a launched basecall leaves its results to the third stream, which the held call's launch inside
    xb_encode_dev's prologue names as it goes: the encoder's own stream must be named after that."""
    monkeypatch.setenv("XB_DECODE_ASYNC", str(decode_async))
    ctx = _context()
    d = _Device(ctx)
    d.encode()
    ctx.synchronize()
    scores = d.scores.cpu().numpy()
    plain = ctx.result_stream()
    assert plain != 0
    assert ctx.reserve_pairing()
    d.clear()
    d.basecall()                                                # held back for a partner
    d.encode()                                                  # launches it on its own first
    assert ctx.result_stream() == plain
    ctx.synchronize()
    assert d.scores.cpu().numpy().tobytes() == scores.tobytes()
    ctx.close()
