"""GPU: xb_ctc_loss_grad / xb_ctc_loss_grad_dev and the autograd criterion on top of them (crf/loss.py).

The contract is bit-equality (np.array_equal) of loss and gradient with the numpy restatement tests/ctcgrad_ref.py -- whose worth
tests/test_ctcgrad_host.py establishes on the CPU -- in the host form and the _dev form, in both score layouts, and with the
host composition the device call replaces (model.seqdist.ctc_loss(numpy scores, want_grad=True)).  The shapes: tests/test_ctc.py's
GPU_CASES, a batch of one on a larger context, label rows built to collide (positions that share a score column must add up in
ascending position, the same bytes on every run), the first width of every instantiation and both sides of every step of the
thread rule, 2048 positions, clipping, a stash bound that forces several launches, two calls
in a row, the refusals, and the torch.autograd surface.  A chunk without a path (T < length - state_len: the header's
precondition, unspecified values) is left out of the comparison; GPU_CASES' 5-90-4-300 holds such chunks."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import ctcgrad_ref as G
from conftest import make_config, random_scores
from ctc_wide_cases import BLANK, half_positions, label_rows
from test_ctc import GPU_CASES
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)


def _context(nb, sl, T, N):
    ctx = _lib.Context(0, nb, sl, 32, 19, 5, 5.0, BLANK, T * 5, N)
    assert ctx.T >= T
    return ctx


def _same(what, got, ref, ok):
    """Bit-equality over the chunks `ok` of a per-chunk vector (N,) or a gradient (T, N, C)."""
    assert got.shape == ref.shape and got.dtype == ref.dtype == np.float32, (what, got.shape, ref.shape, got.dtype)
    g, r = (got[ok], ref[ok]) if got.ndim == 1 else (got[:, ok], ref[:, ok])
    if not np.array_equal(g, r):
        bad = np.argwhere(g != r)
        pytest.fail("%s: %d of %d values differ, first at %s: %r, reference %r; max |difference| %g"
                    % (what, len(bad), g.size, tuple(bad[0]), g[tuple(bad[0])], r[tuple(bad[0])], np.nanmax(np.abs(g - r))))


def _dev_call(ctx, sc, targets, lens, hb, clip=None, reduction="mean", loss_fill=-7.0):
    """xb_ctc_loss_grad_dev on torch's memory: (loss, grad) as numpy; the loss starts as loss_fill, the gradient as NaN."""
    sc = np.ascontiguousarray(sc)
    T, N, _ = sc.shape
    d_sc = torch.from_numpy(sc).to(DEV)
    d_t = torch.from_numpy(np.ascontiguousarray(targets, np.uint8)).to(DEV)
    d_l = torch.from_numpy(np.ascontiguousarray(lens, np.int32)).to(DEV)
    d_loss = torch.full((N,), loss_fill, dtype=torch.float32, device=DEV)
    d_grad = torch.full(sc.shape, float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    err = None
    try:
        ctx.ctc_loss_grad_dev(d_sc.data_ptr(), T, N, hb, d_t.data_ptr(), d_t.shape[1], d_l.data_ptr(), d_loss.data_ptr(),
                              d_grad.data_ptr(), loss_clip=clip, reduction=reduction)
        ctx.synchronize()
    except _lib.XbError as e:
        err = e
    return d_loss.cpu().numpy(), d_grad.cpu().numpy(), err


def _check(ctx, sc, targets, lens, nb, sl, hb, clip=None, reduction="mean", what=""):
    """Both forms against the restatement; returns the reference (loss, grad)."""
    T = sc.shape[0]
    ok = G.has_path(T, lens, sl)
    assert ok.any()
    what = "%s%s, %s" % (what, "with blank" if hb else "blank-less", reduction)
    ref = G.reference(sc, targets, lens, nb, sl, hb, loss_clip=clip, reduction=reduction)
    loss, grad = ctx.ctc_loss_grad(sc, targets, lens, has_blank=hb, loss_clip=clip, reduction=reduction)
    print("%s: max |loss - ref| = %g, max |grad - ref| = %g" % (what, np.abs(loss - ref[0])[ok].max(), np.abs(grad - ref[1])[:, ok].max()))
    _same(what + ", host form, loss", loss, ref[0], ok)
    _same(what + ", host form, grad", grad, ref[1], ok)
    dloss, dgrad, err = _dev_call(ctx, sc, targets, lens, hb, clip, reduction)
    assert err is None, err
    _same(what + ", device form, loss", dloss, ref[0], ok)
    _same(what + ", device form, grad", dgrad, ref[1], ok)
    return ref


def _scores(T, N, nb, sl, hb, seed):
    return random_scores(T, N, nb, sl=sl, seed=seed, with_blank=hb)


@pytest.mark.parametrize("nb,T,N,Lt,sl", GPU_CASES,
                         ids=["%d-%d-%d-%d" % c[:4] + ("" if c[4] == 3 else "-sl%d" % c[4]) for c in GPU_CASES])
def test_gradient_is_the_restatement_bit_for_bit(nb, T, N, Lt, sl):
    targets, lens = label_rows(np.random.default_rng(Lt + nb), N, Lt, nb, sl, lens=None if sl == 3 else [Lt, sl + 1, sl],
                               dtype=np.uint8)
    ctx = _context(nb, sl, T, N)
    for hb in (True, False):
        sc = _scores(T, N, nb, sl, hb, T)
        _check(ctx, sc, targets, lens, nb, sl, hb, reduction="mean")
        _check(ctx, sc, targets, lens, nb, sl, hb, reduction="none")
    ctx.close()


def test_more_than_one_position_per_thread_and_a_batch_of_one():
    """300 label columns with a path for every row (GPU_CASES' own 300-column case has T = 90); then one chunk alone on the same,
    larger context, at a shorter T."""
    nb, sl, T, N, Lt = 5, 3, 310, 3, 300
    targets, lens = label_rows(np.random.default_rng(1), N, Lt, nb, sl, lens=[Lt, 259 + sl - 1, 150], dtype=np.uint8)
    assert G.has_path(T, lens, sl).all()
    ctx = _context(nb, sl, T, N)
    for hb in (True, False):
        sc = _scores(T, N, nb, sl, hb, 3)
        _check(ctx, sc, targets, lens, nb, sl, hb)
        _check(ctx, sc[:200, 2:], targets[2:], lens[2:], nb, sl, hb, what="batch of one, ")
    ctx.close()


@pytest.mark.parametrize("nb", [4, 6])
def test_colliding_label_rows(nb):
    """All one letter, period 2, a k-mer planted three times far apart, a ragged mix: positions that share a stay or a move column
    add up in ascending position.  Also the bytes of the host composition the device call replaces."""
    from xna_basecaller_amd.crf import Model
    sl, T, Lt = 3, 80, 70
    targets, lens = G.colliding_batch(nb, sl, Lt, seed=nb)
    share = G.sharing(targets, lens, nb, sl)
    assert share[0] == (Lt - sl + 1, Lt - sl), share
    assert all(s >= 3 and m >= 3 for s, m in share), share
    assert len(set(lens.tolist())) > 1 and G.has_path(T, lens, sl).all()
    model = Model(make_config(32, "NACGT" if nb == 4 else "NACGTXY")).to("cuda")
    ctx = model.context(T * model.stride, 4)
    ok = np.ones(4, bool)
    for hb in (True, False):
        sc = _scores(T, 4, nb, sl, hb, 21)
        for reduction in ("mean", "none"):
            ref = _check(ctx, sc, targets, lens, nb, sl, hb, reduction=reduction)
            again = ctx.ctc_loss_grad(sc, targets, lens, has_blank=hb, reduction=reduction)      # the same bytes on every run
            _same("second call, loss", again[0], ref[0], ok)
            _same("second call, grad", again[1], ref[1], ok)
            if hb:
                value, grad = model.seqdist.ctc_loss(sc, targets, lens, reduction=reduction, want_grad=True)
                assert isinstance(grad, np.ndarray)
                _same("the host route's grad, " + reduction, grad, ref[1], ok)
                if reduction == "none":
                    _same("the host route's loss", value, ref[0], ok)
                else:
                    assert abs(float(value) - float(ref[0].mean(dtype=np.float32))) < 1e-6


@pytest.mark.parametrize("npos", [64, 65, 128, 129, 257, 513, 1025])
def test_every_instantiation_and_thread_count_boundary(npos):
    """ctc_grad_kernel<1> at 64 threads, <2> at 64 -> 128, <1> -> <2> at 128 -> 256 threads, and the first row of <2>, <4> and <8>
    at 256: the full row beside a chunk of about half its positions, both with a path (T = positions + 2)."""
    nb, sl, N = 4, 3, 2
    T, Lt = npos + 2, npos + sl - 1
    targets, lens = label_rows(np.random.default_rng(npos), N, Lt, nb, sl, lens=[Lt, half_positions(npos) + sl - 1], dtype=np.uint8)
    assert G.has_path(T, lens, sl).all()
    ctx = _context(nb, sl, T, N)
    for hb in (True, False):
        _check(ctx, _scores(T, N, nb, sl, hb, npos), targets, lens, nb, sl, hb)
    ctx.close()


def test_2048_positions():
    nb, sl, N, npos = 5, 3, 2, 2048
    T, Lt = npos + 4, npos + sl - 1
    targets, lens = label_rows(np.random.default_rng(2048), N, Lt, nb, sl, lens=[Lt, 1025 + sl - 1], dtype=np.uint8)
    ctx = _context(nb, sl, T, N)
    for hb in (True, False):
        _check(ctx, _scores(T, N, nb, sl, hb, 7), targets, lens, nb, sl, hb)
    with pytest.raises(_lib.XbError) as e:                        # 2049 positions
        wide = np.ones((N, Lt + 1), np.uint8)
        ctx.ctc_loss_grad(_scores(T, N, nb, sl, True, 7), wide, np.full(N, Lt + 1, np.int32))
    assert e.value.code == _lib.XB_ERR_INVALID and "2049" in str(e.value)
    ctx.close()


def test_loss_clip_zeroes_the_clipped_chunks():
    nb, sl, T, N, Lt = 4, 3, 48, 5, 14
    targets, lens = label_rows(np.random.default_rng(4), N, Lt, nb, sl, dtype=np.uint8)
    ctx = _context(nb, sl, T, N)
    for hb in (True, False):
        sc = _scores(T, N, nb, sl, hb, 9)
        free = ctx.ctc_loss_grad(sc, targets, lens, has_blank=hb, reduction="none")
        assert np.array_equal(free[0], ctx.ctc_loss(sc, targets, lens, has_blank=hb))          # the value is xb_ctc_loss's
        clip = float(np.sort(free[0])[2]) + 1e-4
        out = free[0] > np.float32(clip)
        assert out.sum() == 2
        for reduction in ("none", "mean"):
            loss, grad = _check(ctx, sc, targets, lens, nb, sl, hb, clip=clip, reduction=reduction)
            assert np.all(grad[:, out] == 0) and np.all(loss[out] == np.float32(clip))
            assert np.all(np.abs(grad[:, ~out]).max(axis=(0, 2)) > 0)
        assert np.array_equal(_check(ctx, sc, targets, lens, nb, sl, hb, clip=clip, reduction="none")[1][:, ~out], free[1][:, ~out])
    ctx.close()


def test_stash_bound_splits_the_call_without_changing_a_byte(monkeypatch):
    """A chunk's alpha stash is (T + 1) x positions floats = 311 x 298 x 4 = 370 KB: under XB_CTC_SCRATCH_MB=1 two chunks fit a
    launch, so five chunks take three launches (2, 2, 1).  Then a stale, larger stash must not matter either."""
    nb, sl, T, N, Lt = 5, 3, 310, 5, 300
    targets, lens = label_rows(np.random.default_rng(6), N, Lt, nb, sl, lens=[Lt, 200, 150, 280, 3], dtype=np.uint8)
    assert 2 * 311 * 298 * 4 <= (1 << 20) < 3 * 311 * 298 * 4
    ok = np.ones(N, bool)
    for hb in (True, False):
        sc = _scores(T, N, nb, sl, hb, 13)
        monkeypatch.setenv("XB_CTC_SCRATCH_MB", "1")              # the library reads it on every call
        ctx = _context(nb, sl, T, N)
        ref = _check(ctx, sc, targets, lens, nb, sl, hb, what="split, ")
        monkeypatch.delenv("XB_CTC_SCRATCH_MB")
        whole = ctx.ctc_loss_grad(sc, targets, lens, has_blank=hb)
        _same("one launch, loss", whole[0], ref[0], ok)
        _same("one launch, grad", whole[1], ref[1], ok)
        ctx.close()


def test_refusals_leave_the_other_chunks_right_and_the_context_usable():
    """A bad length, a bad label: the host form refuses with the chunk's index; the _dev form reports by the next synchronize,
    leaves the offending chunk's loss untouched and its gradient zero, and the other chunks' results right."""
    nb, sl, T, N, Lt = 4, 3, 40, 3, 12
    targets, lens = label_rows(np.random.default_rng(8), N, Lt, nb, sl, lens=[Lt, 9, 7], dtype=np.uint8)
    ctx = _context(nb, sl, T, N)
    for hb in (True, False):
        sc = _scores(T, N, nb, sl, hb, 17)
        ref = _check(ctx, sc, targets, lens, nb, sl, hb)
        bad_label, bad_long, bad_short = targets.copy(), lens.copy(), lens.copy()
        bad_label[1, 4] = nb + 1
        bad_long[1], bad_short[1] = Lt + 1, sl - 1
        beyond = targets.copy()
        beyond[1, 10] = nb + 1                                   # beyond the chunk's length: not read
        _same("a label beyond the length", ctx.ctc_loss_grad(sc, beyond, lens, has_blank=hb)[1], ref[1], np.ones(N, bool))
        for t, l in ((bad_label, lens), (targets, bad_long), (targets, bad_short)):
            with pytest.raises(_lib.XbError) as e:
                ctx.ctc_loss_grad(sc, t, l, has_blank=hb)
            assert e.value.code == _lib.XB_ERR_INVALID
            with pytest.raises(_lib.XbError) as e0:
                ctx.ctc_loss(sc, t, l, has_blank=hb)
            assert str(e.value).replace("xb_ctc_loss_grad", "xb_ctc_loss") == str(e0.value)      # as xb_ctc_loss refuses it
            dloss, dgrad, err = _dev_call(ctx, sc, t, l, hb)
            assert err is not None and err.code == _lib.XB_ERR_INVALID
            assert dloss[1] == -7.0 and np.all(dgrad[:, 1] == 0)
            keep = np.array([True, False, True])
            _same("beside a refused chunk, loss", dloss, ref[0], keep)
            _same("beside a refused chunk, grad", dgrad, ref[1], keep)
            _check(ctx, sc, targets, lens, nb, sl, hb, what="after a refusal, ")           # the context works afterwards
    with pytest.raises(_lib.XbError):
        ctx.ctc_loss_grad(_scores(T + 1, N, nb, sl, True, 1), targets, lens)                   # T above the context's
    ctx.close()


@pytest.mark.parametrize("labels", ["NACGT", "NACGTXY"])
def test_autograd_criterion(labels):
    """model.seqdist.ctc_loss on a device tensor: the reference's signature, a tensor with a grad_fn, scores.grad = the C ABI's
    gradient bit for bit; reduction='none' with a grad_output; through F.pad's constant blank column; numpy stays numpy."""
    from xna_basecaller_amd.crf import Model
    nb, sl, T, N, Lt = len(labels) - 1, 3, 30, 3, 10
    model = Model(make_config(32, labels)).to("cuda")
    targets, lens = label_rows(np.random.default_rng(7), N, Lt, nb, sl)
    sc = random_scores(T, N, nb, seed=11)
    ctx = model.context(T * model.stride, N)
    ref_loss, ref_grad = ctx.ctc_loss_grad(sc, targets, lens, reduction="mean")
    ok = np.ones(N, bool)
    _same("C ABI grad", ref_grad, G.reference(sc, targets, lens, nb, sl, True)[1], ok)

    x = torch.tensor(sc, device="cuda", requires_grad=True)
    loss = model.seqdist.ctc_loss(x, torch.from_numpy(targets), torch.from_numpy(lens))
    assert isinstance(loss, torch.Tensor) and loss.grad_fn is not None and loss.shape == ()
    assert abs(float(loss.detach()) - float(ref_loss.mean(dtype=np.float32))) < 1e-6
    loss.backward()
    _same("scores.grad, mean", x.grad.cpu().numpy(), ref_grad, ok)

    per_loss, per_grad = ctx.ctc_loss_grad(sc, targets, lens, reduction="none")
    x = torch.tensor(sc, device="cuda", requires_grad=True)
    per = model.seqdist.ctc_loss(x, targets, lens, reduction="none")
    assert per.shape == (N,) and per.grad_fn is not None and np.array_equal(per.detach().cpu().numpy(), per_loss)
    go = np.array([0.5, -2.0, 3.0], np.float32)
    per.backward(torch.from_numpy(go).to("cuda"))
    _same("scores.grad, none", x.grad.cpu().numpy(), per_grad * go[None, :, None], ok)

    # the reference's expand_blanks training layout: the encoder's blank-less scores padded with the constant blank column
    S = nb ** sl
    nbl = np.ascontiguousarray(sc.reshape(T, N, S, nb + 1)[..., 1:]).reshape(T, N, S * nb)
    y = torch.tensor(nbl, device="cuda", requires_grad=True)
    padded = F.pad(y.view(T, N, S, nb), (1, 0, 0, 0, 0, 0, 0, 0), value=BLANK).view(T, N, -1)
    assert np.array_equal(padded.detach().cpu().numpy(), sc)
    model.seqdist.ctc_loss(padded, targets, lens).backward()
    nbl_grad = ctx.ctc_loss_grad(nbl, targets, lens, has_blank=False, reduction="mean")[1]
    _same("through F.pad", y.grad.cpu().numpy(), nbl_grad, ok)
    _same("through F.pad, the with-blank gradient's move columns", y.grad.cpu().numpy(),
          np.ascontiguousarray(ref_grad.reshape(T, N, S, nb + 1)[..., 1:]).reshape(T, N, S * nb), ok)
    # ... and the blank-less tensor itself
    z = torch.tensor(nbl, device="cuda", requires_grad=True)
    model.seqdist.ctc_loss(z, targets, lens).backward()
    _same("blank-less scores.grad", z.grad.cpu().numpy(), nbl_grad, ok)

    # what is refused, and what stays as it was
    with pytest.raises(NotImplementedError, match="numpy"):
        model.seqdist.ctc_loss(x, targets, lens, normalise_scores=False)
    with pytest.raises(TypeError, match="float32"):
        model.seqdist.ctc_loss(x.detach().half(), targets, lens)
    with pytest.raises(ValueError, match="contiguous"):
        model.seqdist.ctc_loss(x.detach().transpose(0, 1).contiguous().transpose(0, 1), targets, lens)
    with pytest.raises(ValueError):
        model.seqdist.ctc_loss(x.detach()[:, :, :-1].contiguous(), targets, lens)
    value = model.seqdist.ctc_loss(sc, targets, lens)
    assert isinstance(value, np.floating) and not isinstance(value, torch.Tensor)
    value, grad = model.seqdist.ctc_loss(sc, targets, lens, want_grad=True)
    assert isinstance(grad, np.ndarray)
    _same("the host route's grad", grad, ref_grad, ok)
