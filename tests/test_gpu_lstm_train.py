"""GPU: xb_lstm_train_forward_dev / xb_lstm_train_backward_dev (csrc/xb_lstm_train.hip) and the autograd layer on top of them
(crf/lstm.py, crf.model.LSTM.forward).

The reference is the float64 restatement tests/lstm_train_ref.py (itself held to torch.nn.LSTM in float64 by
tests/test_lstm_train_host.py).  The tolerance is measured, not chosen: the error of torch.nn.LSTM in float32 on the CPU against
the same float64 reference on the same (float32) inputs, per tensor, relative to the tensor's maximum -- the device must stay
within MARGIN = 8 times that (its exp-based sigma / tanh against libm-grade ones, another k order).  A wrong gate, a shifted time
index or a lost carry is off by four orders of magnitude or more.  torch keeps neither the gates nor the cell states of the
steps: they are held to the yardstick of y, which is computed from them (y = o tanh(c), |o|, |tanh| <= 1: an error in them of the
size of y's own is what torch's y carries too).  The backward is fed the DEVICE's own gates and c, so its error is its own.
Every test prints both errors.

  kernels    T in {1, 2, 5} x n in {1, 17, 65} (a lone row, a ragged row tile, one past a workgroup's 64 rows: the launch with
             four row tiles per workgroup) x F in {16, 48, 96}, T = 3, n = 5, F = 768 (the real K = 3072 of the backward), and
             T = 64, n = 65, F = 48 (a long chain in the four-tile launch); both directions
  widths     every F the entry points accept (16, 32, .. 1024: nk = F / 16 chunks of k, 1 .. 64), T = 3 (the middle step has a
             recurrent product, a c_prev and a carry at once), both directions: n = 100 (four row tiles per workgroup, k in groups
             of 4 chunks and a tail) against the restatement, and its rows 0..16 against the bytes of an n = 17 call (one row
             tile, groups of 8 and a tail) -- every nk through both variants' grouped and tail loops, and "a row's bytes do not
             depend on the rows beside it" at every width
  row tiles  F in {48, 144, 768}, T = 2, n in {16, 64, 100, 129, 200} (64: the last size with one tile per workgroup; 129: a
             third workgroup with one row; 200: four workgroups, the last with a full, a ragged and two skipped tiles) against the
             restatement, rows 0..15 of each the bytes of the n = 16 call
  bytes      rows 0..16 of an n = 65 call equal an n = 17 call; a repeated call; dy = 0 gives zero bytes; gin of +-1e4 stays finite
  workspace  one context through (n = 100, F = 1024), (n = 17, F = 16) and the first again: each the bytes of a fresh context's
  refusals   F = 24, F = 1040, T = 0, a null pointer: XB_ERR_INVALID, and the context still works
  layer      encoder[7](x) and encoder[8](x) of a small Model, a scalar loss, .backward(): y, x.grad and the three parameter
             gradients against the reference; ten AdamW steps on top LSTM + head bring the loss down"""
import functools

import numpy as np
import pytest
import torch

import lstm_train_ref as R
from conftest import encoder_shapes, make_config, seeded_state_dict
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MARGIN = 8.0
SHAPES = [(T, n, F) for T in (1, 2, 5) for n in (1, 17, 65) for F in (16, 48, 96)] + [(3, 5, 768), (64, 65, 48)]
WIDTHS = list(range(16, 1025, 16))                                  # every F check_shape accepts
TILING = [(F, rev, n) for F in (48, 144, 768) for rev in (False, True) for n in (16, 64, 100, 129, 200)]
RATIOS = []


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0, 4, 2, 32, 19, 5, 5.0, 2.0, 100, 1)        # the recurrence uses the context's stream and workspace only
    yield c
    c.close()
    if RATIOS:
        print("largest ratio to torch float32: %.2f (%s)" % max(RATIOS))


def draw(T, n, F, reverse):
    """float32 inputs (gin, W_hh, dy), the float64 reference of both entry points and the yardstick: torch.nn.LSTM in float32 on
    the CPU, fed gin through an identity input projection (exact), whose x.grad is dgin.  Computed once, never modified."""
    rng = np.random.default_rng(100000 * T + 1000 * n + F + (7 if reverse else 0))
    k = 2.0 / np.sqrt(F)
    gin = (1.5 * rng.standard_normal((T, n, 4 * F))).astype(np.float32)
    w_hh = rng.uniform(-k, k, (4 * F, F)).astype(np.float32)
    dy = rng.standard_normal((T, n, F)).astype(np.float32)
    y, gates, c = R.forward(gin, w_hh, reverse)
    dgin = R.backward(dy, w_hh, gates, c, reverse)
    t32 = R.torch_layer(gin, np.eye(4 * F, dtype=np.float32), w_hh, np.zeros(4 * F, np.float32), dy, reverse, torch.float32)
    yard = dict(y=R.rel(t32["y"], y), dgin=R.rel(t32["dx"], dgin))
    for a in (gin, w_hh, dy, y, gates, c, dgin):
        a.setflags(write=False)
    return dict(gin=gin, w_hh=w_hh, dy=dy, y=y, gates=gates, c=c, dgin=dgin, yard=yard, t32=dict(y=t32["y"], dgin=t32["dx"]))


case = functools.lru_cache(maxsize=None)(draw)
wide_case = functools.lru_cache(maxsize=2)(draw)                    # up to 50 MB a case: used by the test that asks, then dropped


def _dev(a):
    return torch.tensor(np.asarray(a, dtype=np.float32), device=DEV)


def dev_forward(ctx, gin, w_hh, reverse):
    T, n, G = gin.shape
    F = G // 4
    d_gin, d_w = _dev(gin), _dev(w_hh)
    out = [torch.full(s, float("nan"), dtype=torch.float32, device=DEV) for s in ((T, n, F), (T, n, G), (T, n, F))]
    torch.cuda.synchronize()
    ctx.lstm_train_forward_dev(d_gin.data_ptr(), d_w.data_ptr(), T, n, F, reverse, *[o.data_ptr() for o in out])
    ctx.synchronize()
    return tuple(o.cpu().numpy() for o in out)


def dev_backward(ctx, dy, w_hh, gates, c, reverse):
    T, n, F = dy.shape
    d = [_dev(a) for a in (dy, w_hh, gates, c)]
    dgin = torch.full((T, n, 4 * F), float("nan"), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    ctx.lstm_train_backward_dev(*[a.data_ptr() for a in d], T, n, F, reverse, dgin.data_ptr())
    ctx.synchronize()
    return dgin.cpu().numpy()


def held(what, got, ref, yard):
    err = R.rel(got, ref)
    RATIOS.append((err / yard if yard else (0.0 if err == 0.0 else float("inf")), what))
    print("%-28s device %.3g  torch float32 %.3g  ratio %.2f" % (what, err, yard, RATIOS[-1][0]))
    assert np.isfinite(got).all(), what
    assert err <= MARGIN * yard, (what, err, yard)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("T,n,F", SHAPES)
def test_kernels_against_the_restatement(ctx, T, n, F, reverse):
    k = case(T, n, F, reverse)
    tag = "T%d n%d F%d %s" % (T, n, F, "rev" if reverse else "fwd")
    y, gates, c = dev_forward(ctx, k["gin"], k["w_hh"], reverse)
    held(tag + " y", y, k["y"], k["yard"]["y"])
    held(tag + " gates", gates, k["gates"], k["yard"]["y"])
    held(tag + " c", c, k["c"], k["yard"]["y"])
    dgin = dev_backward(ctx, k["dy"], k["w_hh"], gates, c, reverse)
    own = R.backward(k["dy"], k["w_hh"], gates, c, reverse)            # the device's own stash: the backward's error alone
    held(tag + " dgin", dgin, own, k["yard"]["dgin"])


@pytest.mark.parametrize("reverse", [False, True])
def test_rows_do_not_depend_on_the_batch(ctx, reverse):
    k = case(5, 65, 96, reverse)
    y, gates, c = dev_forward(ctx, k["gin"], k["w_hh"], reverse)
    dgin = dev_backward(ctx, k["dy"], k["w_hh"], gates, c, reverse)
    sub = dev_forward(ctx, k["gin"][:, :17], k["w_hh"], reverse)
    for name, whole, part in zip(("y", "gates", "c"), (y, gates, c), sub):
        assert np.ascontiguousarray(whole[:, :17]).tobytes() == part.tobytes(), name
    dsub = dev_backward(ctx, k["dy"][:, :17], k["w_hh"], sub[1], sub[2], reverse)
    assert np.ascontiguousarray(dgin[:, :17]).tobytes() == dsub.tobytes()


def _rows_equal(whole, part, what):
    """The first rows of every step of `whole` (T, n, ..) are the bytes of `part` (T, m, ..)."""
    assert np.ascontiguousarray(whole[:, :part.shape[1]]).tobytes() == part.tobytes(), what


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("F", WIDTHS)
def test_every_width_in_both_launches(ctx, F, reverse):
    k = wide_case(3, 100, F, reverse)
    tag = "sweep F%d %s" % (F, "rev" if reverse else "fwd")
    y, gates, c = dev_forward(ctx, k["gin"], k["w_hh"], reverse)
    held(tag + " y", y, k["y"], k["yard"]["y"])
    held(tag + " gates", gates, k["gates"], k["yard"]["y"])
    held(tag + " c", c, k["c"], k["yard"]["y"])
    dgin = dev_backward(ctx, k["dy"], k["w_hh"], gates, c, reverse)
    held(tag + " dgin", dgin, R.backward(k["dy"], k["w_hh"], gates, c, reverse), k["yard"]["dgin"])
    sub = dev_forward(ctx, k["gin"][:, :17], k["w_hh"], reverse)                # one row tile a workgroup, k in groups of 8
    for name, whole, part in zip(("y", "gates", "c"), (y, gates, c), sub):
        _rows_equal(whole, part, tag + " " + name)
    _rows_equal(dgin, dev_backward(ctx, k["dy"][:, :17], k["w_hh"], sub[1], sub[2], reverse), tag + " dgin")


@pytest.mark.parametrize("F,reverse,n", TILING)
def test_row_tiling(ctx, F, reverse, n):
    k = wide_case(2, 200, F, reverse)                                   # n rows of the case are its first n
    tag = "tiles n%d F%d %s" % (n, F, "rev" if reverse else "fwd")
    gin, dy = k["gin"][:, :n], k["dy"][:, :n]
    y, gates, c = dev_forward(ctx, gin, k["w_hh"], reverse)
    yard = R.rel(k["t32"]["y"][:, :n], k["y"][:, :n])
    held(tag + " y", y, k["y"][:, :n], yard)
    held(tag + " gates", gates, k["gates"][:, :n], yard)
    held(tag + " c", c, k["c"][:, :n], yard)
    dgin = dev_backward(ctx, dy, k["w_hh"], gates, c, reverse)
    held(tag + " dgin", dgin, R.backward(dy, k["w_hh"], gates, c, reverse), R.rel(k["t32"]["dgin"][:, :n], k["dgin"][:, :n]))
    first = dev_forward(ctx, gin[:, :16], k["w_hh"], reverse)
    for name, whole, part in zip(("y", "gates", "c"), (y, gates, c), first):
        _rows_equal(whole, part, tag + " " + name)
    _rows_equal(dgin, dev_backward(ctx, dy[:, :16], k["w_hh"], first[1], first[2], reverse), tag + " dgin")


def test_the_workspace_serves_calls_of_any_size_in_any_order():
    """The carry and the transposed W_hh lie in the context and grow with the calls: a large call, a small one in the large
    one's buffers and the large one again each give the bytes of the same call on a context of its own."""
    big, small = wide_case(3, 100, 1024, False), wide_case(3, 17, 16, True)
    calls = [(big, False), (small, True), (big, False)]

    def run(c, k, reverse):                                             # the backward takes any stash: the reference's, in float32
        return dev_backward(c, k["dy"], k["w_hh"], k["gates"], k["c"], reverse)

    shared = _lib.Context(0, 4, 2, 32, 19, 5, 5.0, 2.0, 100, 1)
    try:
        got = [run(shared, k, reverse) for k, reverse in calls]
    finally:
        shared.close()
    for i, (k, reverse) in enumerate(calls[:2]):
        fresh = _lib.Context(0, 4, 2, 32, 19, 5, 5.0, 2.0, 100, 1)
        try:
            alone = run(fresh, k, reverse)
        finally:
            fresh.close()
        own = R.backward(k["dy"], k["w_hh"], k["gates"].astype(np.float32), k["c"].astype(np.float32), reverse)
        held("workspace, call %d dgin" % i, alone, own, k["yard"]["dgin"])      # the right call, not only the same one
        assert got[i].tobytes() == alone.tobytes(), i
        if i == 0:
            assert got[2].tobytes() == alone.tobytes()


@pytest.mark.parametrize("n", [17, 65])
def test_a_repeated_call_gives_the_same_bytes(ctx, n):
    k = case(5, n, 96, True)
    a = dev_forward(ctx, k["gin"], k["w_hh"], True)
    b = dev_forward(ctx, k["gin"], k["w_hh"], True)
    assert all(p.tobytes() == q.tobytes() for p, q in zip(a, b))
    assert dev_backward(ctx, k["dy"], k["w_hh"], a[1], a[2], True).tobytes() == dev_backward(ctx, k["dy"], k["w_hh"], a[1], a[2], True).tobytes()


@pytest.mark.parametrize("reverse", [False, True])
def test_saturated_gates_stay_finite(ctx, reverse):
    k = case(5, 17, 48, reverse)
    rng = np.random.default_rng(5)
    gin = k["gin"].copy()
    hit = rng.random(gin.shape) < 0.3
    gin[hit] = np.where(rng.random(hit.sum()) < 0.5, np.float32(1e4), np.float32(-1e4))
    y, gates, c = dev_forward(ctx, gin, k["w_hh"], reverse)
    dgin = dev_backward(ctx, k["dy"], k["w_hh"], gates, c, reverse)
    for name, a in (("y", y), ("gates", gates), ("c", c), ("dgin", dgin)):
        assert np.isfinite(a).all(), name
    assert np.abs(y).max() <= 1.0 and gates.min() >= -1.0 and gates.max() <= 1.0
    ry, rg, _ = R.forward(gin, k["w_hh"], reverse)
    print("saturated: y off by %.3g, gates by %.3g of the maximum" % (R.rel(y, ry), R.rel(gates, rg)))
    assert R.rel(y, ry) < 1e-4 and R.rel(gates, rg) < 1e-4              # the right function where it saturates, not only finite


@pytest.mark.parametrize("n", [17, 65])
def test_a_gradient_of_zeros_gives_zero_bytes(ctx, n):
    k = case(5, n, 96, False)
    _, gates, c = dev_forward(ctx, k["gin"], k["w_hh"], False)
    dgin = dev_backward(ctx, np.zeros_like(k["dy"]), k["w_hh"], gates, c, False)
    assert dgin.tobytes() == bytes(dgin.nbytes)


def test_refusals_leave_the_context_usable(ctx):
    k = case(2, 17, 48, False)
    big = [torch.zeros(2 * 17 * 4 * 1040, dtype=torch.float32, device=DEV) for _ in range(6)]
    p = [b.data_ptr() for b in big]
    torch.cuda.synchronize()
    for T, n, F in ((2, 17, 24), (2, 17, 1040), (0, 17, 48), (2, 0, 48), (2, 17, 0)):
        with pytest.raises(_lib.XbError, match="F = %d" % F) as e:
            ctx.lstm_train_forward_dev(p[0], p[1], T, n, F, 0, p[2], p[3], p[4])
        assert e.value.code == _lib.XB_ERR_INVALID and "T = %d" % T in str(e.value)
        with pytest.raises(_lib.XbError, match="F = %d" % F) as e:
            ctx.lstm_train_backward_dev(p[0], p[1], p[2], p[3], T, n, F, 0, p[4])
        assert e.value.code == _lib.XB_ERR_INVALID
    for hole in range(5):
        q = [None if i == hole else p[i] for i in range(5)]
        with pytest.raises(_lib.XbError, match="null") as e:
            ctx.lstm_train_forward_dev(q[0], q[1], 2, 17, 48, 0, q[2], q[3], q[4])
        assert e.value.code == _lib.XB_ERR_INVALID
        with pytest.raises(_lib.XbError, match="null") as e:
            ctx.lstm_train_backward_dev(q[0], q[1], q[2], q[3], 2, 17, 48, 0, q[4])
        assert e.value.code == _lib.XB_ERR_INVALID
    with pytest.raises(_lib.XbError, match="aligned"):
        ctx.lstm_train_forward_dev(p[0] + 4, p[1], 2, 17, 48, 0, p[2], p[3], p[4])
    y, gates, c = dev_forward(ctx, k["gin"], k["w_hh"], False)
    held("after the refusals, y", y, k["y"], k["yard"]["y"])


# ---- the layer through Model ---------------------------------------------------------------------------------------------------
F_T, L_T, LT, N_T = 96, 500, 24, 6


@pytest.fixture(scope="module")
def model():
    from xna_basecaller_amd.crf import Model
    config = make_config(F_T)
    config["basecaller"]["batchsize"] = N_T
    m = Model(config).to("cuda")
    m.precision = _lib.PRECISIONS["f16x3"]
    keys, shapes = encoder_shapes(F_T, m.seqdist.n_base, 3)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_state_dict(keys, shapes, seed=3).items()})
    yield m
    m._drop_context()


@pytest.mark.parametrize("index", [7, 8])
def test_layer_against_the_restatement(model, index):
    T = L_T // model.stride
    layer = model.encoder[index].to(DEV)
    rng = np.random.default_rng(index)
    x = rng.standard_normal((T, N_T, F_T)).astype(np.float32)
    dy = rng.standard_normal((T, N_T, F_T)).astype(np.float32)
    w_ih, w_hh, b = (getattr(layer.rnn, k).detach().cpu().numpy() for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0"))
    ref = R.layer(x, w_ih, w_hh, b, dy, layer.reverse)
    t32 = R.torch_layer(x, w_ih, w_hh, b, dy, layer.reverse, torch.float32)
    assert layer.reverse == (index == 8)

    for p in layer.parameters():
        p.grad = None
    xt = torch.tensor(x, device=DEV, requires_grad=True)
    y = layer(xt)
    assert y.grad_fn is not None and y.shape == (T, N_T, F_T) and y.device == xt.device
    (y * _dev(dy)).sum().backward()
    got = dict(y=y.detach(), dx=xt.grad, dw_ih=layer.rnn.weight_ih_l0.grad, dw_hh=layer.rnn.weight_hh_l0.grad, db=layer.rnn.bias_ih_l0.grad)
    assert layer.rnn.bias_hh_l0.grad is None
    for k in ("y", "dx", "dw_ih", "dw_hh", "db"):
        held("encoder[%d] %s" % (index, k), got[k].cpu().numpy(), ref[k], R.rel(t32[k], ref[k]))

    with pytest.raises(TypeError, match="float32"):
        layer(xt.detach().double())
    with pytest.raises(ValueError, match="contiguous"):
        layer(xt.detach().transpose(0, 1).contiguous().transpose(0, 1))
    with pytest.raises(ValueError, match="model.encoder"):
        model.encoder[4](xt.detach())                                   # its parameters were never moved to the device


def test_ten_adamw_steps_on_top_lstm_and_head_bring_the_loss_down(model):
    """--num-unfreeze-top 2 by hand: the frozen encoder's layer-3 output (hi + residual of the three-product precision) feeds
    encoder[8] (this package's backward) and the head (torch's linear and tanh); the criterion is model.seqdist.ctc_loss."""
    rng = np.random.default_rng(11)
    nb, sl = model.seqdist.n_base, model.seqdist.state_len
    signal = rng.standard_normal((N_T, L_T)).astype(np.float32)
    lens = rng.integers(sl + 5, LT + 1, N_T).astype(np.int32)
    targets = np.zeros((N_T, LT), np.uint8)
    for i in range(N_T):
        targets[i, :lens[i]] = rng.integers(1, nb + 1, lens[i])
    model(signal[:, None, :])
    hi, lo = model.context(L_T, N_T).debug_layer_output(0, N_T)
    x = _dev(hi.view(np.float16).astype(np.float32) + lo.view(np.float16).astype(np.float32))
    top, head = model.encoder[8].to(DEV), model.encoder[9].to(DEV)
    scale = float(head.scale)
    params = [p for p in list(top.parameters()) + list(head.parameters()) if p.requires_grad]
    assert len(params) == 5
    before = [p.detach().clone() for p in params]
    opt = torch.optim.AdamW(params, lr=2e-3)
    losses = []
    for _ in range(10):
        opt.zero_grad()
        scores = scale * torch.tanh(torch.nn.functional.linear(top(x), head.linear.weight, head.linear.bias))
        loss = model.seqdist.ctc_loss(scores, targets, lens)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
    print("losses", " ".join("%.4f" % v for v in losses))
    assert np.isfinite(losses).all() and losses[-1] < losses[0], losses
    assert all(not torch.equal(p.detach(), q) for p, q in zip(params, before))
    with torch.no_grad():                                               # the fixture's model is shared: put the floats back
        for p, q in zip(params, before):
            p.copy_(q)
