"""GPU: the three trainers on contexts of other geometries than the shipped one's (tests/train_geometry_cases.py): every head width
a context takes beside 64, 125, 256 and 1296, under windows 1 .. 31 and strides 1 .. 8 of conv3, a stride above the window, features
96 with a ragged row tile, and a chunk shorter than the window (T = 1).  Every comparison is one the trainers' own tests make at
window 19, stride 5 (tests/test_gpu_fulltrain.py, test_gpu_toptrainer.py, test_gpu_headtrain.py):

  full    after xb_full_train_begin and xb_top_train_grad x0, the scores, d loss / d scores, all 28 gradients, the loss and the norm
          equal, byte for byte, the public entry points chained by hand (tests/convtrain_dev.py at the case's stride, tests/toptrain_dev.py,
          xb_ctc_loss_grad_dev); the scores and gradients are within MARGIN = 8 times the error of torch float32 of the float64 chain
          (train_geometry_cases.torch_chain, fed the device's own d loss / d scores; tests/test_train_geometry_host.py holds that
          chain to the restatements) -- not at T = 1, where the yardstick is degenerate and every dW_hh is zero bytes; then one
          xb_top_train_step is tests/adamw_ref.py on the gradient just read, bit for bit
  top     L = 2: x0 is xb_encode_bottom_dev(layers = 3) byte for byte, the gradient tests/toptrain_dev.py's composed step
  head    two xb_head_train_step calls equal, in loss, norm, weights and the three images, the step composed from the public parts on
          a second context

Largest ratio to torch float32 measured on an MI355X: see DESIGN.md 4.2.9."""
import numpy as np
import pytest
import torch

import adamw_ref as A
import convtrain_dev as CD
import toptrain_dev as D
import train_geometry_cases as G
from lstm_train_ref import rel
from test_gpu_headtrain import B_KEY, W_KEY, _composed_step, _expected_image, _same_image
from xna_basecaller_amd import _lib
from xna_basecaller_amd.crf.trainer import full_keys, top_keys

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MARGIN = 8.0
LR = 2e-3
RATIOS = []


@pytest.fixture(scope="module", autouse=True)
def largest_ratio():
    yield
    if RATIOS:
        print("largest ratio to torch float32: %.2f (%s)" % max(RATIOS))


def context(c, sd=None):
    ctx = _lib.Context(0, c.nb, c.sl, c.F, c.W, c.S, G.SCALE, 2.0, c.chunk, c.n, precision=_lib.XB_PREC_MIXED)
    assert (ctx.T, ctx.C_noblank) == (G.steps(c)[2], G.columns(c))
    sd = G.weights(c) if sd is None else sd
    ctx.load_state_dict(sd)
    return ctx, sd


def flat(sd, keys):
    return np.concatenate([sd[k].ravel() for k in keys])


def split(flat_array, sd, keys):
    out, at = [], 0
    for k in keys:
        out.append(flat_array[at:at + sd[k].size].reshape(sd[k].shape))
        at += sd[k].size
    assert at == flat_array.size
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def state(ctx, c, params):
    T, C = G.steps(c)[2], G.columns(c)
    s = ctx.top_state_dev()
    assert s["rows"] == T * c.n
    out = {k: ctx.peek(s[k], (params,)) for k in ("p", "g", "m", "v")}
    out.update(x0=ctx.peek(s["x0"], (T, c.n, c.F)), scores=ctx.peek(s["scores"], (T, c.n, C)), dscores=ctx.peek(s["dscores"], (T, c.n, C)),
               step=s["step"])
    return out


def loss_gradient(ctx, c, d_scores, targets, lens):
    """xb_ctc_loss_grad_dev (mean, blank-less) of scores on the device: the losses (n,) and d loss / d scores, both on the device."""
    T, C = G.steps(c)[2], G.columns(c)
    d_t, d_l = _dev(targets), _dev(lens)
    d_loss = torch.full((c.n,), float("nan"), dtype=torch.float32, device=DEV)
    d_grad = torch.full((T, c.n, C), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.ctc_loss_grad_dev(d_scores.data_ptr(), T, c.n, False, d_t.data_ptr(), targets.shape[1], d_l.data_ptr(), d_loss.data_ptr(), d_grad.data_ptr())
    ctx.synchronize()
    return d_loss, d_grad


def loss_and_norm_are(ctx, c, loss, norm, d_loss, grads):
    """The trainer's mean loss is the running float sum of the losses over n, its norm xb_grad_norm_dev of the gradients in their order."""
    total = 0.0
    for x in d_loss.cpu().numpy():
        total += float(x)
    assert np.isfinite(loss) and np.float32(loss).tobytes() == np.float32(total / c.n).tobytes()
    d_g, d_norm = torch.cat([g.reshape(-1) for g in grads]), torch.zeros(1, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.grad_norm_dev(d_g.data_ptr(), d_g.numel(), None, 0, d_norm.data_ptr())
    ctx.synchronize()
    assert np.isfinite(norm) and norm > 0 and np.float32(norm).tobytes() == d_norm.cpu().numpy().tobytes()


def same_gradients(c, keys, mine, theirs):
    for key, m, t in zip(keys, mine, theirs):
        t = t.cpu().numpy() if isinstance(t, torch.Tensor) else t
        assert m.shape == t.shape and np.isfinite(m).all(), key
        if G.steps(c)[2] == 1 and key.endswith("weight_hh_l0"):         # h_-1 = 0: no step has a recurrent product
            assert m.tobytes() == bytes(m.nbytes), key
        else:
            assert np.abs(m).max() > 0, key
        assert m.tobytes() == t.tobytes(), (key, float(np.abs(m - t).max()))


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_full_trainer_is_the_chained_entry_points_and_within_the_rule(c):
    T = G.steps(c)[2]
    keys = full_keys()
    assert keys == G.KEYS
    ctx, sd = context(c)
    signal, targets, lens = G.batch(c, seed=61)
    params = flat(sd, keys).size
    assert params == ctx.full_params()
    ctx.full_train_begin(flat(sd, keys))
    loss, norm = ctx.top_train_grad(signal, targets, lens)
    got = state(ctx, c, params)
    assert got["step"] == 0 and got["p"].tobytes() == flat(sd, keys).tobytes() and not got["m"].any() and not got["v"].any()

    # the public entry points chained by hand, on the trainer's own masters
    masters = [_dev(a) for a in split(got["p"], sd, keys)]
    conv = CD.stack_forward(ctx, _dev(signal), masters[:6], stride=c.S)
    x0 = conv[2]["y"]
    assert tuple(x0.shape) == (T, c.n, c.F) and np.isfinite(got["x0"]).all() and x0.cpu().numpy().tobytes() == got["x0"].tobytes()
    stages = D.forward(ctx, x0, masters[6:], G.SCALE)
    assert np.isfinite(got["scores"]).all() and stages["scores"].cpu().numpy().tobytes() == got["scores"].tobytes()
    d_loss, d_grad = loss_gradient(ctx, c, stages["scores"], targets, lens)
    assert np.isfinite(got["dscores"]).all() and np.abs(got["dscores"]).max() > 0
    assert d_grad.cpu().numpy().tobytes() == got["dscores"].tobytes()
    top = D.backward(ctx, stages, d_grad)
    grads = CD.stack_backward(ctx, conv, stages["layers"][0]["dx"]) + top
    assert len(grads) == 28
    same_gradients(c, keys, split(got["g"], sd, keys), grads)
    loss_and_norm_are(ctx, c, loss, norm, d_loss, grads)
    print("%s: loss %.4f norm %.4g" % (G.case_id(c), loss, norm))

    # the float64 chain, fed the device's own d loss / d scores
    if T > 1:
        tensors = [sd[k] for k in keys]
        ref = G.torch_chain(signal, tensors, got["dscores"], torch.float64, c.S)
        t32 = G.torch_chain(signal, tensors, got["dscores"], torch.float32, c.S)
        failed = []
        rows = [("scores", got["scores"], ref["scores"], t32["scores"])] + list(zip(keys, split(got["g"], sd, keys), ref["grads"], t32["grads"]))
        for what, g, want, t in rows:
            assert g.shape == want.shape, what
            err, yard = rel(g, want), rel(t, want)
            ratio = err / yard if yard else (0.0 if err == 0.0 else float("inf"))
            RATIOS.append((ratio, "%s %s" % (G.case_id(c), what)))
            print("%-32s device %.3g  torch float32 %.3g  ratio %.2f" % (what, err, yard, ratio))
            if not np.isfinite(g).all() or not err <= MARGIN * yard:
                failed.append((what, err, yard))
        assert not failed, failed

    # one step: AdamW on the gradient just read
    loss1, norm1 = ctx.top_train_step(signal, targets, lens, LR)
    assert (loss1, norm1) == (loss, norm)
    p, gc, m, v = A.step(got["p"], got["g"], got["m"], got["v"], A.clip_factor(norm), *A.scalars(float(np.float32(LR)), 1))
    after = state(ctx, c, params)
    assert after["step"] == 1
    for name, mine, want in (("p", after["p"], p), ("g", after["g"], gc), ("m", after["m"], m), ("v", after["v"], v)):
        assert mine.tobytes() == want.tobytes(), name
    assert ctx.top_get_weights().tobytes() == p.tobytes() and p.tobytes() != got["p"].tobytes()
    ctx.top_train_end()
    ctx.close()


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_top_trainer_is_the_bottom_pass_and_the_composed_step(c):
    L, T = 2, G.steps(c)[2]
    keys = top_keys(L)
    ctx, sd = context(c)
    signal, targets, lens = G.batch(c, seed=62)
    params = flat(sd, keys).size
    assert params == ctx.top_params(L)
    ctx.top_train_begin(L, flat(sd, keys))
    loss, norm = ctx.top_train_grad(signal, targets, lens)
    got = state(ctx, c, params)
    assert got["step"] == 0 and got["p"].tobytes() == flat(sd, keys).tobytes() and not got["m"].any() and not got["v"].any()

    d_sig = _dev(signal)
    d_x0 = torch.full((T, c.n, c.F), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.encode_bottom_dev(d_sig.data_ptr(), c.n, 5 - L, d_x0.data_ptr())
    ctx.synchronize()
    assert np.isfinite(got["x0"]).all() and np.abs(got["x0"]).max() > 0 and got["x0"].tobytes() == d_x0.cpu().numpy().tobytes()

    # the loss gradient of the trainer's own scores, then the composed step on the trainer's x0 and masters
    d_loss, d_grad = loss_gradient(ctx, c, _dev(got["scores"]), targets, lens)
    assert np.isfinite(got["dscores"]).all() and np.abs(got["dscores"]).max() > 0
    assert d_grad.cpu().numpy().tobytes() == got["dscores"].tobytes()
    step = D.composed_step(ctx, _dev(got["x0"]), [_dev(a) for a in split(got["p"], sd, keys)], G.SCALE, d_grad)
    assert np.isfinite(got["scores"]).all() and step["scores"].tobytes() == got["scores"].tobytes()
    same_gradients(c, keys, split(got["g"], sd, keys), step["grads"])
    loss_and_norm_are(ctx, c, loss, norm, d_loss, [_dev(g) for g in step["grads"]])
    print("%s: loss %.4f norm %.4g" % (G.case_id(c), loss, norm))
    ctx.top_train_end()
    ctx.close()


@pytest.mark.parametrize("c", G.CASES, ids=G.case_id)
def test_head_trainer_is_its_parts(c):
    a, sd = context(c)
    b, _ = context(c, sd=sd)
    a.head_train_begin(sd[W_KEY], sd[B_KEY])
    held = {"w": [_dev(sd[W_KEY]), _dev(np.zeros_like(sd[W_KEY])), _dev(np.zeros_like(sd[W_KEY]))],
            "b": [_dev(sd[B_KEY]), _dev(np.zeros_like(sd[B_KEY])), _dev(np.zeros_like(sd[B_KEY]))]}
    torch.cuda.synchronize()
    for t in (1, 2):
        batch = G.batch(c, seed=70 + t)
        loss, norm = a.head_train_step(*batch, LR)
        ref_loss, ref_norm = _composed_step(b, held, batch, LR, t)
        print("%s step %d: loss %.6f norm %.6g" % (G.case_id(c), t, loss, norm))
        assert np.isfinite(loss) and np.isfinite(norm) and norm > 0
        assert np.float32(loss).tobytes() == ref_loss.tobytes() and np.float32(norm).tobytes() == ref_norm.tobytes(), (t, loss, ref_loss)
        w, bias = a.head_get_weights()
        assert w.tobytes() == held["w"][0].cpu().numpy().tobytes() and bias.tobytes() == held["b"][0].cpu().numpy().tobytes(), t
        assert not np.array_equal(w, sd[W_KEY]) and not np.array_equal(bias, sd[B_KEY])
        _same_image(a.head_image(), b.head_image(), "step %d" % t)
        _same_image(a.head_image(), _expected_image(w, bias), "step %d, master weights" % t)
    a.head_train_end()
    for ctx in (a, b):
        ctx.close()
