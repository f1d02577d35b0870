"""GPU: the trainer of every layer (csrc/xb_top.hip: xb_full_train_begin, then xb_top_train_grad / _step / _get_weights / _end) on the
small model of tests/test_gpu_toptrainer.py: n_base 5, state_len 2 (C = 125), features 32, chunks of 200 samples (T = 40), n = 6, label
rows of 20.

  parts      after xb_top_train_grad the scores and all 28 gradients equal, byte for byte, what the public entry points give when
             chained by hand: xb_conv_train_forward_dev three times, tests/toptrain_dev.py's forward, xb_ctc_loss_grad_dev, its
             backward, xb_conv_train_backward_dev three times (tests/convtrain_dev.py); loss and norm too; a second call gives the
             same bytes
  accuracy   the gradients read through xb_internal_top_state against the whole chain in float64 (torch autograd on the CPU, fed the
             device's own d loss / d scores as tests/test_gpu_toptrain.py's loss case is), by the rule of that file: per tensor,
             relative to the tensor's maximum, within MARGIN = 8 times the error of the same chain in torch float32
  step       a step changes every tensor, and AdamW's step count; xb_top_get_weights returns the whole flat array
  refusals   XB_ERR_STATE while a head trainer or a top trainer is open, and the other way round

Largest ratio to torch float32 measured on an MI355X: see DESIGN.md 4.2.9."""
import numpy as np
import pytest
import torch

import convtrain_dev as CD
import toptrain_dev as D
import train_geometry_cases as G
from conftest import encoder_shapes, seeded_state_dict
from ctc_wide_cases import label_rows
from lstm_train_ref import rel
from xna_basecaller_amd import _lib
from xna_basecaller_amd.crf.trainer import full_keys, top_keys

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NB, SL, F, C, CHUNK, T, LT, N, SCALE = 5, 2, 32, 125, 200, 40, 20, 6, 5.0
MARGIN = 8.0
RATIOS = []


def weights(seed=3):
    keys, shapes = encoder_shapes(F, NB, SL)
    assert keys == full_keys()
    return seeded_state_dict(keys, shapes, seed=seed)


def context(n=N, precision=_lib.XB_PREC_MIXED):
    ctx = _lib.Context(0, NB, SL, F, 19, 5, SCALE, 2.0, CHUNK, n, precision=precision)
    assert (ctx.T, ctx.C_noblank) == (T, C)
    sd = weights()
    ctx.load_state_dict(sd)
    return ctx, sd


def batch(n, seed):
    rng = np.random.default_rng(seed)
    signal = rng.standard_normal((n, CHUNK)).astype(np.float32)
    targets, lens = label_rows(rng, n, LT, NB, SL, dtype=np.uint8)
    assert (T >= lens.astype(np.int64) - SL).all()                      # every row has a path
    return signal, targets, lens.astype(np.int32)


def flat(sd):
    return np.concatenate([sd[k].ravel() for k in full_keys()])


def split(flat_array, sd):
    out, at = [], 0
    for k in full_keys():
        out.append(flat_array[at:at + sd[k].size].reshape(sd[k].shape))
        at += sd[k].size
    assert at == flat_array.size
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def state(ctx, sd, n):
    s = ctx.top_state_dev()
    params = flat(sd).size
    assert s["rows"] == T * n and params == ctx.full_params() == 360 + F * (16 * 19 + 1) + ctx.top_params(5)
    out = {k: ctx.peek(s[k], (params,)) for k in ("p", "g", "m", "v")}
    out.update(x0=ctx.peek(s["x0"], (T, n, F)), scores=ctx.peek(s["scores"], (T, n, C)), dscores=ctx.peek(s["dscores"], (T, n, C)), step=s["step"])
    return out


def torch_chain(signal, tensors, dscores, dtype):
    """train_geometry_cases.torch_chain, the whole encoder in torch on the CPU, at this file's stride and scale."""
    return G.torch_chain(signal, tensors, dscores, dtype, stride=5, scale=SCALE)


@pytest.fixture(scope="module")
def grad_run():
    """One xb_top_train_grad of the full trainer, its state, and the same call again."""
    ctx, sd = context()
    signal, targets, lens = batch(N, seed=61)
    ctx.full_train_begin(flat(sd))
    loss, norm = ctx.top_train_grad(signal, targets, lens)
    got = state(ctx, sd, N)
    again = ctx.top_train_grad(signal, targets, lens)
    second = state(ctx, sd, N)
    yield dict(ctx=ctx, sd=sd, signal=signal, targets=targets, lens=lens, loss=loss, norm=norm, got=got, again=again, second=second)
    ctx.top_train_end()
    ctx.close()
    if RATIOS:
        print("largest ratio to torch float32: %.2f (%s)" % max(RATIOS))


def test_gradient_is_the_chained_entry_points_byte_for_byte(grad_run):
    r = grad_run
    ctx, sd, got = r["ctx"], r["sd"], r["got"]
    assert got["step"] == 0 and got["p"].tobytes() == flat(sd).tobytes() and not got["m"].any() and not got["v"].any()
    masters = [_dev(a) for a in split(got["p"], sd)]
    conv = CD.stack_forward(ctx, _dev(r["signal"]), masters[:6])
    x0 = conv[2]["y"]
    assert tuple(x0.shape) == (T, N, F) and x0.cpu().numpy().tobytes() == got["x0"].tobytes()
    stages = D.forward(ctx, x0, masters[6:], SCALE)
    assert stages["scores"].cpu().numpy().tobytes() == got["scores"].tobytes()
    d_t, d_l = _dev(r["targets"]), _dev(r["lens"])
    d_loss = torch.full((N,), float("nan"), dtype=torch.float32, device=DEV)
    d_grad = torch.full((T, N, C), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.ctc_loss_grad_dev(stages["scores"].data_ptr(), T, N, False, d_t.data_ptr(), LT, d_l.data_ptr(), d_loss.data_ptr(), d_grad.data_ptr())
    ctx.synchronize()
    assert d_grad.cpu().numpy().tobytes() == got["dscores"].tobytes()
    top = D.backward(ctx, stages, d_grad)
    grads = CD.stack_backward(ctx, conv, stages["layers"][0]["dx"]) + top
    assert len(grads) == 28
    for key, mine, theirs in zip(full_keys(), split(got["g"], sd), grads):
        theirs = theirs.cpu().numpy()
        assert np.isfinite(mine).all() and np.abs(mine).max() > 0, key
        assert mine.tobytes() == theirs.tobytes(), (key, float(np.abs(mine - theirs).max()))

    total = 0.0
    for x in d_loss.cpu().numpy():
        total += float(x)
    assert np.float32(r["loss"]).tobytes() == np.float32(total / N).tobytes()
    d_g, d_norm = torch.cat([g.reshape(-1) for g in grads]), torch.zeros(1, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.grad_norm_dev(d_g.data_ptr(), d_g.numel(), None, 0, d_norm.data_ptr())
    ctx.synchronize()
    assert np.float32(r["norm"]).tobytes() == d_norm.cpu().numpy().tobytes()
    print("loss %.4f norm %.4g" % (r["loss"], r["norm"]))

    assert r["again"] == (r["loss"], r["norm"])                         # a second call gives the same bytes
    for k in ("p", "g", "m", "v", "x0", "scores", "dscores"):
        assert r["second"][k].tobytes() == got[k].tobytes(), k


def test_gradients_against_float64_by_the_rule(grad_run):
    r = grad_run
    sd, got = r["sd"], r["got"]
    tensors = [sd[k] for k in full_keys()]
    ref = torch_chain(r["signal"], tensors, got["dscores"], torch.float64)
    t32 = torch_chain(r["signal"], tensors, got["dscores"], torch.float32)
    failed = []
    rows = [("scores", got["scores"], ref["scores"], t32["scores"])] + list(zip(full_keys(), split(got["g"], sd), ref["grads"], t32["grads"]))
    for what, g, want, t in rows:
        assert g.shape == want.shape, what
        err, yard = rel(g, want), rel(t, want)
        ratio = err / yard if yard else (0.0 if err == 0.0 else float("inf"))
        RATIOS.append((ratio, what))
        print("%-32s device %.3g  torch float32 %.3g  ratio %.2f" % (what, err, yard, ratio))
        if not np.isfinite(g).all() or not err <= MARGIN * yard:
            failed.append((what, err, yard))
    assert not failed, failed


def test_a_step_changes_every_tensor():
    ctx, sd = context(precision=_lib.XB_PREC_F16F8)                     # the inference bottom never runs: its precision is free
    signal, targets, lens = batch(N, seed=62)
    ctx.full_train_begin(flat(sd))
    before = ctx.top_get_weights()
    assert before.tobytes() == flat(sd).tobytes()
    loss0, norm0 = ctx.top_train_grad(signal, targets, lens)
    loss, norm = ctx.top_train_step(signal, targets, lens, 2e-3)
    assert (loss, norm) == (loss0, norm0) and np.isfinite(loss) and np.isfinite(norm) and norm > 0
    after = ctx.top_get_weights()
    assert ctx.top_state_dev()["step"] == 1 and np.isfinite(after).all()
    for key, a, b in zip(full_keys(), split(before, sd), split(after, sd)):
        assert (a != b).any(), key
    loss2, _ = ctx.top_train_step(signal, targets, lens, 2e-3)
    print("loss %.4f -> %.4f" % (loss, loss2))
    assert np.isfinite(loss2) and ctx.top_state_dev()["step"] == 2
    ctx.top_train_end()
    ctx.close()


def test_one_trainer_at_a_time():
    ctx, sd = context(n=4)
    with pytest.raises(ValueError, match="floats expected"):
        ctx.full_train_begin(flat(sd)[:-1])
    ctx.head_train_begin(sd["encoder.9.linear.weight"], sd["encoder.9.linear.bias"])
    with pytest.raises(_lib.XbError, match="xb_full_train_begin.*xb_head_train_end") as e:
        ctx.full_train_begin(flat(sd))
    assert e.value.code == _lib.XB_ERR_STATE
    ctx.head_train_end()
    ctx.top_train_begin(2, np.concatenate([sd[k].ravel() for k in top_keys(2)]))
    with pytest.raises(_lib.XbError, match="xb_full_train_begin.*already open") as e:
        ctx.full_train_begin(flat(sd))
    assert e.value.code == _lib.XB_ERR_STATE
    ctx.top_train_end()
    ctx.full_train_begin(flat(sd))
    for call, needle in ((lambda: ctx.full_train_begin(flat(sd)), "already open"), (lambda: ctx.top_train_begin(2, np.concatenate([sd[k].ravel() for k in top_keys(2)])), "already open"),
                         (lambda: ctx.head_train_begin(sd["encoder.9.linear.weight"], sd["encoder.9.linear.bias"]), "xb_top_train_end")):
        with pytest.raises(_lib.XbError, match=needle) as e:
            call()
        assert e.value.code == _lib.XB_ERR_STATE
    ctx.top_train_end()
    ctx.top_train_begin(1, np.concatenate([sd[k].ravel() for k in top_keys(1)]))      # a top trainer after a full one lays out its own buffers
    signal, targets, lens = batch(4, seed=63)
    loss, norm = ctx.top_train_step(signal, targets, lens, 2e-3)
    assert np.isfinite(loss) and np.isfinite(norm)
    assert ctx.top_get_weights().size == ctx.top_params(1)
    ctx.top_train_end()
    ctx.close()
