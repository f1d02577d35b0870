"""GPU: the parts of a head-training step and the trainer that chains them (csrc/xb_head.hip).

  xb_adamw_step_dev    bit-equal to tests/adamw_ref.py over 5 consecutive steps at lengths 1, 63, 64, 65 and 99 533, with a clip
                       below 1 and a gradient of zeros among them
  xb_grad_norm_dev     1e-6 relative against float64
  xb_head_repack_dev   the three images and the bias equal xb::split_rows / xb::fragment_major (tests/host_logic.py) of the same
                       floats byte for byte, at heads of 64, 125, 216, 625, 1024, 1296, 3125 and 4096 columns and features 32
                       and 768
  xb_head_train_step   bit-equal, in loss, norm, weights and images, to the step composed from the public entry points on a
                       second context, at 256 columns and features 96, and two steps each at 3125 and 4096 columns and features 32;
                       a fresh context loaded with the trained floats encodes the same bytes; 30 steps on 32
                       chunks with fixed label rows bring the loss down; the refusals"""
import numpy as np
import pytest
import torch

import adamw_ref as A
import host_logic as HL
from conftest import encoder_shapes, seeded_state_dict
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
HEADS = {64: (4, 2), 125: (5, 2), 256: (4, 3), 1296: (6, 3), 216: (6, 2), 625: (5, 3), 1024: (4, 4), 3125: (5, 4), 4096: (4, 5)}
W_KEY, B_KEY = "encoder.9.linear.weight", "encoder.9.linear.bias"


def _context(F, O, chunk_len=100, n=1, precision=_lib.XB_PREC_MIXED, seed=3, sd=None):
    nb, sl = HEADS[O]
    ctx = _lib.Context(0, nb, sl, F, 19, 5, 5.0, 2.0, chunk_len, n, precision=precision)
    if sd is None:
        keys, shapes = encoder_shapes(F, nb, sl)
        sd = seeded_state_dict(keys, shapes, seed=seed)
    ctx.load_state_dict(sd)
    return ctx, sd


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


@pytest.fixture(scope="module")
def small_ctx():
    ctx, _ = _context(32, 64)
    yield ctx
    ctx.close()


@pytest.mark.parametrize("n", [1, 63, 64, 65, 99533])
def test_adamw_is_the_restatement_bit_for_bit(small_ctx, n):
    rng = np.random.default_rng(n)
    p = (rng.standard_normal(n) * 0.1).astype(np.float32)
    m, v = np.zeros(n, np.float32), np.zeros(n, np.float32)
    d_p, d_m, d_v = _dev(p), _dev(m), _dev(v)
    for t in range(1, 6):
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-7, -2, n)).astype(np.float32)
        if t == 3:
            g[:] = 0.0
        clip = np.float32(0.4321) if t in (2, 3) else np.float32(1.0)
        lr = 2e-3 * t / 5
        sc = A.scalars(lr, t)
        d_g = _dev(g)
        torch.cuda.synchronize()
        small_ctx.adamw_step_dev(d_p.data_ptr(), d_g.data_ptr(), d_m.data_ptr(), d_v.data_ptr(), n, clip, *sc)
        small_ctx.synchronize()
        p, g, m, v = A.step(p, g, m, v, clip, *sc)
        for name, got, ref in (("p", d_p, p), ("g", d_g, g), ("m", d_m, m), ("v", d_v, v)):
            assert got.cpu().numpy().tobytes() == ref.tobytes(), (name, t, n)


def test_grad_norm(small_ctx):
    rng = np.random.default_rng(0)
    for nw, nb in ((1296 * 768, 1296), (1, 0), (63, 1), (70001, 65)):
        w = (rng.standard_normal(nw) * 1e-3).astype(np.float32)
        b = (rng.standard_normal(nb) * 1e-2).astype(np.float32)
        d_w, d_b, d_n = _dev(w), _dev(b), torch.zeros(1, dtype=torch.float32, device=DEV)
        torch.cuda.synchronize()
        small_ctx.grad_norm_dev(d_w.data_ptr(), nw, d_b.data_ptr() if nb else None, nb, d_n.data_ptr())
        small_ctx.synchronize()
        ref = np.sqrt((w.astype(np.float64) ** 2).sum() + (b.astype(np.float64) ** 2).sum())
        assert abs(float(d_n.cpu()[0]) - ref) <= 1e-6 * ref, (nw, nb)


def _expected_image(w, b):
    O, F = w.shape
    hi, lo, _ = HL.split_rows(w, F)
    image, _ = HL.fragment_major(hi, lo, O, F, 3)
    return hi.view(np.uint16), lo.view(np.uint16), np.frombuffer(bytes(image), np.uint8), b


def _same_image(got, want, what):
    for name, g, w in zip(("hi", "lo", "image", "bias"), got, want):
        assert g.tobytes() == np.ascontiguousarray(w).tobytes(), (what, name)


@pytest.mark.parametrize("O", [64, 125, 1296, 216, 625, 1024, 3125, 4096])
@pytest.mark.parametrize("F", [32, 768])
def test_repack_is_the_host_packer_byte_for_byte(F, O):
    ctx, sd = _context(F, O)
    _same_image(ctx.head_image(), _expected_image(sd[W_KEY], sd[B_KEY]), "as uploaded")
    rng = np.random.default_rng(F + O)
    w = (sd[W_KEY] * (1 + 0.3 * rng.standard_normal(sd[W_KEY].shape))).astype(np.float32)
    w[0, :8] = [0.0, -0.0, 1e-8, 65504.0, -1.0, 2.0 ** -25, 1.0 + 2.0 ** -12, 3.14159]
    b = (sd[B_KEY] + 0.1 * rng.standard_normal(O)).astype(np.float32)
    d_w, d_b = _dev(w), _dev(b)
    torch.cuda.synchronize()
    ctx.head_repack_dev(d_w.data_ptr(), d_b.data_ptr())
    ctx.synchronize()
    _same_image(ctx.head_image(), _expected_image(w, b), "after the repack")
    ctx.close()


# ---- the trainer ------------------------------------------------------------------------------------------------------------
F_T, O_T, L_T, LT = 96, 256, 500, 24


def _batch(n, seed, O=O_T, chunk_len=L_T):
    rng = np.random.default_rng(seed)
    nb, sl = HEADS[O]
    signal = rng.standard_normal((n, chunk_len)).astype(np.float32)
    lens = rng.integers(sl + 5, LT + 1, n).astype(np.int32)
    lens[0] = LT
    targets = np.zeros((n, LT), np.uint8)
    for i in range(n):
        targets[i, :lens[i]] = rng.integers(1, nb + 1, lens[i])
    return signal, targets, lens


def _composed_step(ctx, state, batch, lr, t):
    """One step from the public entry points: encode, loss gradient, head gradient, norm, AdamW on W and on b, repack."""
    signal, targets, lens = batch
    n = signal.shape[0]
    y = ctx.encode(signal, expand_blanks=False)
    losses, dy = ctx.ctc_loss_grad(y, targets, lens, has_blank=False, reduction="mean")
    dw, db = ctx.head_grad(y, dy)
    d_norm = torch.zeros(1, dtype=torch.float32, device=DEV)
    d_gw, d_gb = _dev(dw), _dev(db)
    torch.cuda.synchronize()
    ctx.grad_norm_dev(d_gw.data_ptr(), dw.size, d_gb.data_ptr(), db.size, d_norm.data_ptr())
    ctx.synchronize()
    norm = np.float32(d_norm.cpu()[0])
    clip, sc = A.clip_factor(norm), A.scalars(float(np.float32(lr)), t)
    for key, d_g in (("w", d_gw), ("b", d_gb)):
        d_p, d_m, d_v = state[key]
        ctx.adamw_step_dev(d_p.data_ptr(), d_g.data_ptr(), d_m.data_ptr(), d_v.data_ptr(), d_p.numel(), clip, *sc)
    ctx.head_repack_dev(state["w"][0].data_ptr(), state["b"][0].data_ptr())
    ctx.synchronize()
    total = 0.0
    for x in losses:
        total += float(x)
    return np.float32(total / n), norm


def _steps_are_their_parts(F, O, chunk_len, n, steps):
    """`steps` xb_head_train_step calls on context a against the composed step on context b; both left open, the trainer too."""
    a, sd = _context(F, O, chunk_len=chunk_len, n=n)
    b, _ = _context(F, O, chunk_len=chunk_len, n=n, sd=sd)
    assert a.T >= LT - HEADS[O][1]                                       # every label row has a path
    a.head_train_begin(sd[W_KEY], sd[B_KEY])
    state = {"w": [_dev(sd[W_KEY]), _dev(np.zeros_like(sd[W_KEY])), _dev(np.zeros_like(sd[W_KEY]))],
             "b": [_dev(sd[B_KEY]), _dev(np.zeros_like(sd[B_KEY])), _dev(np.zeros_like(sd[B_KEY]))]}
    torch.cuda.synchronize()
    lr = 2e-3
    for t in range(1, steps + 1):
        batch = _batch(n, seed=t, O=O, chunk_len=chunk_len)
        loss, norm = a.head_train_step(*batch, lr)
        ref_loss, ref_norm = _composed_step(b, state, batch, lr, t)
        print("step %d: loss %.6f norm %.6g" % (t, loss, norm))
        assert np.isfinite(loss) and np.isfinite(norm) and norm > 0
        assert np.float32(loss).tobytes() == ref_loss.tobytes() and np.float32(norm).tobytes() == ref_norm.tobytes(), (t, loss, ref_loss)
        w, bias = a.head_get_weights()
        assert w.tobytes() == state["w"][0].cpu().numpy().tobytes() and bias.tobytes() == state["b"][0].cpu().numpy().tobytes(), t
        assert not np.array_equal(w, sd[W_KEY]) and not np.array_equal(bias, sd[B_KEY])
        _same_image(a.head_image(), b.head_image(), "step %d" % t)
        _same_image(a.head_image(), _expected_image(w, bias), "step %d, master weights" % t)
    return a, b, sd


def test_step_is_its_parts_and_the_trained_floats_reload():
    n = 8
    a, b, sd = _steps_are_their_parts(F_T, O_T, L_T, n, 3)
    signal = _batch(n, seed=9)[0]
    trained = a.encode(signal, expand_blanks=False)
    w, bias = a.head_get_weights()
    fresh, _ = _context(F_T, O_T, chunk_len=L_T, n=n, sd=dict(sd, **{W_KEY: w, B_KEY: bias}))
    assert fresh.encode(signal, expand_blanks=False).tobytes() == trained.tobytes()
    a.head_train_end()
    assert a.encode(signal, expand_blanks=False).tobytes() == trained.tobytes()        # the trained head stays until weights are loaded
    for c in (a, b, fresh):
        c.close()


@pytest.mark.parametrize("O", [3125, 4096])
def test_step_is_its_parts_at_the_widest_heads(O):
    """Features 32, chunks of 200 samples (T = 40), three chunks, two steps: 49 column tiles with rows that are not 16-byte aligned,
    and 64 tiles."""
    a, b, _ = _steps_are_their_parts(32, O, 200, 3, 2)
    a.head_train_end()
    for c in (a, b):
        c.close()


def test_thirty_steps_bring_the_loss_down():
    n = 32
    ctx, sd = _context(F_T, O_T, chunk_len=L_T, n=n)
    ctx.head_train_begin(sd[W_KEY], sd[B_KEY])
    batch = _batch(n, seed=4)
    losses = [ctx.head_train_step(*batch, 2e-3)[0] for _ in range(30)]
    print("loss: first %.4f, last %.4f" % (losses[0], losses[-1]))
    assert np.isfinite(losses).all() and losses[-1] < losses[0]
    ctx.head_train_end()
    ctx.close()


def test_refusals():
    ctx, sd = _context(32, 64, precision=_lib.XB_PREC_F16F8)
    with pytest.raises(_lib.XbError, match="three fp16 products"):
        ctx.head_train_begin(sd[W_KEY], sd[B_KEY])
    ctx.close()
    ctx, sd = _context(F_T, O_T, chunk_len=L_T, n=2)
    batch = _batch(2, seed=1)
    for call in (lambda: ctx.head_train_step(*batch, 2e-3), ctx.head_get_weights, ctx.head_train_end):
        with pytest.raises(_lib.XbError, match="no trainer is open") as e:
            call()
        assert e.value.code == _lib.XB_ERR_STATE
    ctx.head_train_begin(sd[W_KEY], sd[B_KEY])
    with pytest.raises(_lib.XbError, match="xb_head_train_end") as e:
        ctx.load_state_dict(sd)
    assert e.value.code == _lib.XB_ERR_STATE
    with pytest.raises(_lib.XbError, match="already open"):
        ctx.head_train_begin(sd[W_KEY], sd[B_KEY])
    bad = (batch[0], batch[1], np.array([LT + 1, 5], np.int32))
    with pytest.raises(_lib.XbError, match="target_lengths"):
        ctx.head_train_step(*bad, 2e-3)
    ctx.head_train_step(*batch, 2e-3)
    ctx.head_train_end()
    ctx.load_state_dict(sd)
    ctx.close()
