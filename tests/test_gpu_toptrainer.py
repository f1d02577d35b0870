"""GPU: the trainer of the head and the top L LSTM layers (csrc/xb_top.hip, crf/trainer.py TopTrainer) on a small model: n_base 5,
state_len 2 (C = 125 blank-less columns, a ragged last tile), chunks of 200 samples (T = 40), as toptrain_ref.LOSS_CASE; features
32 or 64 (a context takes 32, 64, 96, ..: the 48 of toptrain_ref's cases exists for the products alone).

  xb_transpose_f32_dev   the bytes of numpy's .T
  xb_encode_bottom_dev   layers = 4 / 5: hi + lo (fp32) of what a full encode leaves in xb_debug_layer_output(0 / 1), byte for byte;
                         every depth 0 .. 3: fed through the float64 restatement of the remaining layers and the head
                         (tests/toptrain_ref.py), the result is the device's own mixed-precision scores within the bound
                         tests/encoder_cases.py holds for the mixed encoder at features 32 -- a layer too many or too few is off by O(1)
  xb_top_train_grad      the scores and all 4 L + 2 gradients equal, byte for byte, the step tests/toptrain_dev.py composes from the
                         public entry points on the trainer's own x0, masters and loss gradient; loss and norm too; a second call
                         gives the same bytes.  (The composed step's accuracy is tests/test_gpu_toptrain.py's subject.)
  xb_top_train_step      p, m, v over three steps equal tests/adamw_ref.py on the unclipped gradient with the step's clip and
                         scalars, bit for bit, with a clip below 1 among them
  TopTrainer             frozen tensors stay the pretrained bytes, trained ones move; after publish() the training context encodes
                         what a fresh context loaded with trainer.state_dict() encodes; ten steps bring the loss down
  refusals"""
import numpy as np
import pytest
import torch

import adamw_ref as A
import toptrain_dev as D
import toptrain_ref as TR
from conftest import encoder_shapes, make_config, seeded_state_dict
from ctc_wide_cases import label_rows
from encoder_cases import BOUNDS
from xna_basecaller_amd import _lib
from xna_basecaller_amd.crf.trainer import top_keys

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
NB, SL, C, CHUNK, T, LT, SCALE = 5, 2, 125, 200, 40, 20, 5.0
assert (C, T) == (TR.LOSS_CASE.C, TR.LOSS_CASE.T)
# The whole mixed encoder at features 32 against float64 (weights drawn to be sensitive): here only the layers above the cut
# differ from float64, on seeded weights.
MIXED_MAX = BOUNDS["f32_nb4_L23_N65"]["mixed"][0]


def weights(F, seed=3):
    keys, shapes = encoder_shapes(F, NB, SL)
    return seeded_state_dict(keys, shapes, seed=seed)


def context(F, n, precision=_lib.XB_PREC_MIXED, sd=None):
    ctx = _lib.Context(0, NB, SL, F, 19, 5, SCALE, 2.0, CHUNK, n, precision=precision)
    assert (ctx.T, ctx.C_noblank) == (T, C)
    sd = weights(F) if sd is None else sd
    ctx.load_state_dict(sd)
    return ctx, sd


def batch(n, seed):
    rng = np.random.default_rng(seed)
    signal = rng.standard_normal((n, CHUNK)).astype(np.float32)
    targets, lens = label_rows(rng, n, LT, NB, SL, dtype=np.uint8)
    assert (T >= lens.astype(np.int64) - SL).all()                      # every row has a path
    return signal, targets, lens.astype(np.int32)


def flat(sd, L):
    return np.concatenate([sd[k].ravel() for k in top_keys(L)])


def split(flat_array, sd, L):
    out, at = [], 0
    for k in top_keys(L):
        out.append(flat_array[at:at + sd[k].size].reshape(sd[k].shape))
        at += sd[k].size
    assert at == flat_array.size
    return out


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


# ---- the transpose ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def ctx32():
    ctx, sd = context(32, 65)
    yield ctx, sd
    ctx.close()


@pytest.mark.parametrize("shape", [(64, 16), (192, 48), (125, 48), (3072, 768), (1, 7)], ids=lambda s: "%dx%d" % s)
def test_transpose_is_numpys(ctx32, shape):
    ctx, _ = ctx32
    a = np.random.default_rng(shape[0]).standard_normal(shape).astype(np.float32)
    a.flat[:3] = [0.0, -0.0, np.float32(1e-42)]
    d_in = _dev(a)
    d_out = torch.full((shape[1], shape[0]), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.transpose_f32_dev(d_in.data_ptr(), shape[0], shape[1], d_out.data_ptr())
    ctx.synchronize()
    assert d_out.cpu().numpy().tobytes() == np.ascontiguousarray(a.T).tobytes()


# ---- the bottom pass --------------------------------------------------------------------------------------------------------------
def bottom(ctx, signal, layers, F):
    n = signal.shape[0]
    d_sig = _dev(signal)
    d_x0 = torch.full((T, n, F), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.encode_bottom_dev(d_sig.data_ptr(), n, layers, d_x0.data_ptr())
    ctx.synchronize()
    return d_x0.cpu().numpy()


@pytest.mark.parametrize("n", [6, 65])
def test_bottom_pass_is_the_full_pass_byte_for_byte(ctx32, n):
    ctx, _ = ctx32
    signal = batch(n, seed=n)[0]
    ctx.encode(signal, expand_blanks=False)
    want = []
    for which in (0, 1):
        hi, lo = ctx.debug_layer_output(which, n)
        want.append(hi.view(np.float16).astype(np.float32) + lo.view(np.float16).astype(np.float32))
    for layers, w in ((4, want[0]), (5, want[1])):
        got = bottom(ctx, signal, layers, 32)
        assert np.isfinite(got).all() and np.abs(got).max() > 0
        assert got.tobytes() == w.tobytes(), (layers, n, float(np.abs(got - w).max()))
    assert want[0].tobytes() != want[1].tobytes()


@pytest.mark.parametrize("depth", [0, 1, 2, 3])
def test_bottom_pass_at_every_depth_continues_to_the_encoders_scores(ctx32, depth):
    ctx, sd = ctx32
    n, L = 6, 5 - depth
    signal = batch(n, seed=40 + depth)[0]
    scores = ctx.encode(signal, expand_blanks=False)
    x0 = bottom(ctx, signal, depth, 32)
    tensors = [sd[k] for k in top_keys(L)]
    ref = TR.run(x0, tensors, SCALE, np.zeros((T, n, C)))["scores"]
    err = float(np.abs(scores - ref).max())
    print("depth %d: |device mixed scores - float64 continuation| max %.3g, bound %.3g" % (depth, err, MIXED_MAX))
    assert err <= MIXED_MAX, (depth, err)
    # the bound tells a layer too many or too few apart: the continuation from one layer further down is O(1) away
    if depth:
        wrong = TR.run(bottom(ctx, signal, depth - 1, 32), tensors, SCALE, np.zeros((T, n, C)))["scores"]
        assert float(np.abs(scores - wrong).max()) > 100 * MIXED_MAX


# ---- refusals ---------------------------------------------------------------------------------------------------------------------
def test_refusals():
    ctx, sd = context(32, 4, precision=_lib.XB_PREC_F16F8)
    signal, targets, lens = batch(4, seed=1)
    d_sig, d_x0 = _dev(signal), torch.zeros((T, 4, 32), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    with pytest.raises(_lib.XbError, match="mixed or f16x3") as e:
        ctx.encode_bottom_dev(d_sig.data_ptr(), 4, 4, d_x0.data_ptr())
    assert e.value.code == _lib.XB_ERR_INVALID
    with pytest.raises(_lib.XbError, match="mixed or f16x3") as e:
        ctx.top_train_begin(1, flat(sd, 1))
    assert e.value.code == _lib.XB_ERR_INVALID
    ctx.close()

    ctx, sd = context(32, 4)
    for layers in (-1, 6):
        with pytest.raises(_lib.XbError, match="0 .. 5") as e:
            ctx.encode_bottom_dev(d_sig.data_ptr(), 4, layers, d_x0.data_ptr())
        assert e.value.code == _lib.XB_ERR_INVALID
    for call in (lambda: ctx.top_train_step(signal, targets, lens, 2e-3), lambda: ctx.top_train_grad(signal, targets, lens),
                 ctx.top_get_weights, ctx.top_train_end):
        with pytest.raises(_lib.XbError, match="no trainer is open") as e:
            call()
        assert e.value.code == _lib.XB_ERR_STATE
    for L in (0, 6):
        with pytest.raises(_lib.XbError, match="1 .. 5") as e:
            ctx.top_train_begin(L, flat(sd, 5))
        assert e.value.code == _lib.XB_ERR_INVALID
    ctx.head_train_begin(sd["encoder.9.linear.weight"], sd["encoder.9.linear.bias"])
    with pytest.raises(_lib.XbError, match="xb_head_train_end") as e:
        ctx.top_train_begin(2, flat(sd, 2))
    assert e.value.code == _lib.XB_ERR_STATE
    ctx.head_train_end()
    ctx.top_train_begin(2, flat(sd, 2))
    with pytest.raises(_lib.XbError, match="already open") as e:
        ctx.top_train_begin(2, flat(sd, 2))
    assert e.value.code == _lib.XB_ERR_STATE
    with pytest.raises(_lib.XbError, match="xb_top_train_end") as e:
        ctx.head_train_begin(sd["encoder.9.linear.weight"], sd["encoder.9.linear.bias"])
    assert e.value.code == _lib.XB_ERR_STATE
    bad = (signal, targets, np.array([LT + 1, 5, 5, 5], np.int32))
    with pytest.raises(_lib.XbError, match="target_lengths"):
        ctx.top_train_step(*bad, 2e-3)
    ctx.load_state_dict(sd)                                             # allowed: the inference forms only
    loss, norm = ctx.top_train_step(signal, targets, lens, 2e-3)
    assert np.isfinite(loss) and np.isfinite(norm)
    ctx.top_train_end()
    ctx.close()


# ---- the gradient is its parts ----------------------------------------------------------------------------------------------------
def state(ctx, sd, L, n):
    s = ctx.top_state_dev()
    params = flat(sd, L).size
    rows = T * n
    assert s["rows"] == rows
    out = {k: ctx.peek(s[k], (params,)) for k in ("p", "g", "m", "v")}
    F = sd["encoder.2.conv.bias"].size
    out.update(x0=ctx.peek(s["x0"], (T, n, F)), scores=ctx.peek(s["scores"], (T, n, C)), dscores=ctx.peek(s["dscores"], (T, n, C)),
               step=s["step"])
    return out


@pytest.mark.parametrize("L,F", [(1, 64), (2, 64), (5, 32)], ids=["L1", "L2", "L5"])
@pytest.mark.parametrize("n", [6, 17])
def test_gradient_is_the_composed_step_byte_for_byte(L, F, n):
    ctx, sd = context(F, n)
    signal, targets, lens = batch(n, seed=10 * L + n)
    ctx.top_train_begin(L, flat(sd, L))
    loss, norm = ctx.top_train_grad(signal, targets, lens)
    got = state(ctx, sd, L, n)
    assert got["step"] == 0 and got["p"].tobytes() == flat(sd, L).tobytes()
    assert np.isfinite(got["x0"]).all() and got["x0"].tobytes() == bottom(ctx, signal, 5 - L, F).tobytes()

    # the loss gradient of the trainer's own scores, then the composed step on the trainer's x0 and masters
    d_scores, d_t, d_l = _dev(got["scores"]), _dev(targets), _dev(lens)
    d_loss = torch.full((n,), float("nan"), dtype=torch.float32, device=DEV)
    d_grad = torch.full((T, n, C), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.ctc_loss_grad_dev(d_scores.data_ptr(), T, n, False, d_t.data_ptr(), LT, d_l.data_ptr(), d_loss.data_ptr(), d_grad.data_ptr())
    ctx.synchronize()
    assert d_grad.cpu().numpy().tobytes() == got["dscores"].tobytes()
    step = D.composed_step(ctx, _dev(got["x0"]), [_dev(a) for a in split(got["p"], sd, L)], SCALE, d_grad)
    assert step["scores"].tobytes() == got["scores"].tobytes()
    for key, mine, theirs in zip(top_keys(L), split(got["g"], sd, L), step["grads"]):
        assert np.isfinite(mine).all() and np.abs(mine).max() > 0, key
        assert mine.tobytes() == theirs.tobytes(), (key, float(np.abs(mine - theirs).max()))

    total = 0.0
    for x in d_loss.cpu().numpy():
        total += float(x)
    assert np.float32(loss).tobytes() == np.float32(total / n).tobytes()
    d_g, d_norm = _dev(np.concatenate([g.ravel() for g in step["grads"]])), torch.zeros(1, dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.grad_norm_dev(d_g.data_ptr(), d_g.numel(), None, 0, d_norm.data_ptr())
    ctx.synchronize()
    assert np.float32(norm).tobytes() == d_norm.cpu().numpy().tobytes()
    print("L %d n %d: loss %.4f norm %.4g" % (L, n, loss, norm))

    again = ctx.top_train_grad(signal, targets, lens)
    second = state(ctx, sd, L, n)
    assert again == (loss, norm)
    for k in ("p", "g", "m", "v", "x0", "scores", "dscores"):
        assert second[k].tobytes() == got[k].tobytes(), k
    assert not got["m"].any() and not got["v"].any()
    ctx.top_train_end()
    ctx.close()


# ---- the update -------------------------------------------------------------------------------------------------------------------
def test_three_steps_are_adamw_on_the_unclipped_gradient():
    L, F, n, lr = 2, 64, 3, 2e-3
    sd = weights(F)
    # short label rows under a head ten times as steep: a gradient whose norm exceeds max_norm = 2, so the step clips
    sd["encoder.9.linear.weight"] = (sd["encoder.9.linear.weight"] * np.float32(10)).astype(np.float32)
    ctx, _ = context(F, n, sd=sd)
    rng = np.random.default_rng(5)
    signal = rng.standard_normal((n, CHUNK)).astype(np.float32)
    targets, lens = label_rows(rng, n, LT, NB, SL, lens=np.array([3, 4, 5]), dtype=np.uint8)
    lens = lens.astype(np.int32)
    ctx.top_train_begin(L, flat(sd, L))
    p, m, v = flat(sd, L), np.zeros(flat(sd, L).size, np.float32), np.zeros(flat(sd, L).size, np.float32)
    clips = []
    for t in range(1, 4):
        loss0, norm0 = ctx.top_train_grad(signal, targets, lens)
        g = state(ctx, sd, L, n)["g"]
        loss, norm = ctx.top_train_step(signal, targets, lens, lr)
        assert (loss, norm) == (loss0, norm0)
        clip = A.clip_factor(norm)
        clips.append(float(clip))
        p, gc, m, v = A.step(p, g, m, v, clip, *A.scalars(float(np.float32(lr)), t))
        got = state(ctx, sd, L, n)
        assert got["step"] == t
        for name, mine, ref in (("p", got["p"], p), ("g", got["g"], gc), ("m", got["m"], m), ("v", got["v"], v)):
            assert mine.tobytes() == ref.tobytes(), (name, t)
        assert ctx.top_get_weights().tobytes() == p.tobytes()
        print("step %d: loss %.4f norm %.4g clip %.4g" % (t, loss, norm, clip))
    assert min(clips) < 1.0, clips
    ctx.top_train_end()
    ctx.close()


# ---- TopTrainer -------------------------------------------------------------------------------------------------------------------
def model_of(F, n, sd):
    from xna_basecaller_amd.crf import Model
    config = make_config(F, list("NACGTX"))
    config["global_norm"]["state_len"] = SL
    config["basecaller"] = {"batchsize": n, "chunksize": CHUNK, "overlap": 0}
    m = Model(config).to("cuda")
    m.load_state_dict({k: torch.from_numpy(v.copy()) for k, v in sd.items()})
    return m


@pytest.mark.parametrize("L", [1, 3])
def test_frozen_stays_frozen_and_the_trained_layers_reach_the_inference_path(L):
    F, n = 32, 6
    sd = weights(F, seed=7)
    model = model_of(F, n, sd)
    signal, targets, lens = batch(n, seed=3)
    before = model(signal[:, None, :])
    trainer = model.top_trainer(L, CHUNK, n)
    for _ in range(3):
        loss, norm = trainer.step(signal[:, None, :], targets, lens, 2e-3)
        assert np.isfinite(loss) and np.isfinite(norm)
    assert model(signal[:, None, :]).tobytes() == before.tobytes()      # the inference forms are not the trainer's
    trainer.publish()
    trained = trainer.state_dict()
    assert list(trained) == list(sd)
    moved = set(top_keys(L))
    assert len(moved) == 4 * L + 2
    for k in sd:
        same = trained[k].numpy().tobytes() == sd[k].tobytes()
        assert same != (k in moved), k
        assert model.state_dict()[k].numpy().tobytes() == trained[k].numpy().tobytes(), k
    after = model(signal[:, None, :])
    fresh, _ = context(F, n, sd={k: v.numpy() for k, v in trained.items()})
    assert fresh.encode(signal).tobytes() == after.tobytes() and after.tobytes() != before.tobytes()
    fresh.close()
    seq, seq_lens, vloss = model.validate_chunks(signal[:, None, :], targets, lens)
    assert np.isfinite(vloss).all()
    trainer.step(signal[:, None, :], targets, lens, 2e-3)               # the trainer goes on after a publish
    trainer.close()
    assert model(signal[:, None, :]).tobytes() != after.tobytes()
    model._drop_context()


def test_ten_steps_bring_the_loss_down():
    F, n = 64, 6
    model = model_of(F, n, weights(F, seed=11))
    signal, targets, lens = batch(n, seed=11)
    trainer = model.top_trainer(2, CHUNK, n)
    losses = [trainer.step(signal[:, None, :], targets, lens, 2e-3)[0] for _ in range(10)]
    print("losses", " ".join("%.4f" % v for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    trainer.close()
    model._drop_context()
