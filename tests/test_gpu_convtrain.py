"""GPU: the training forward and backward of one `Convolution` layer (csrc/xb_conv_train.hip: xb_conv_train_forward_dev,
xb_conv_train_backward_dev) against the float64 restatement tests/convtrain_ref.py.  The tolerance is the rule of
tests/test_gpu_toptrain.py: per tensor, the error relative to the tensor's maximum stays within MARGIN = 8 times that of
torch.nn.functional.conv1d + silu with autograd in float32 on the CPU on the same float32 inputs.  tests/test_convtrain_host.py
runs a float32 numpy stand-in through the same cases and the same rule on the CPU.

  cases      convtrain_ref.CASES: both routes, edges, Lin < K, a stride that does not divide Lin, a ragged and the real Cout, dw over
             several workgroups' partials (narrow) and past xb_wgrad_f32's 1024-row block (wide), gradients of 1e-9 .. 1e-4; the
             narrow kernels' three templates with Cout at and below the template's width; even windows on both routes (narrow:
             the backward's tile count comes from Lout = Lin + 1); strides above the window (dx holds exact zeros, written as +0);
             windows 1 and 31, Lout 1; the wide cases with tnc = 0 and 1
  bytes      dx = NULL leaves dw and db as they are; a chunk's z, y and dx are the same alone and inside a batch; a repeated call
             gives the same bytes
  refusals   every malformed argument is XB_ERR_INVALID, and nothing is written

Largest ratio to torch float32 measured on an MI355X: see DESIGN.md 4.2.9."""
import functools

import numpy as np
import pytest
import torch

import convtrain_dev as CD
import convtrain_ref as CR
from lstm_train_ref import rel
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda", 0)
MARGIN = 8.0
RATIOS = []
TENSORS = ("z", "y", "dx", "dw", "db")


@pytest.fixture(scope="module")
def ctx():
    c = _lib.Context(0, 5, 2, 32, 19, 5, 5.0, 2.0, 200, 6)             # no weights are loaded: the entry points need none
    yield c
    c.close()
    if RATIOS:
        print("largest ratio to torch float32: %.2f (%s)" % max(RATIOS))


@functools.lru_cache(maxsize=None)
def reference(case):
    """The inputs of a case, its float64 tensors and the errors of torch float32 against them: computed once, never changed."""
    x, w, b, dy = CR.draw(case)
    z, y = CR.forward(x, w, b, case.stride)
    ref = dict(zip(TENSORS, (z, y) + CR.backward(dy, x, z, w, case.stride)))
    t32 = CR.torch_run(x, w, b, dy, case.stride, torch.float32)
    return (x, w, b, dy), ref, {k: rel(t32[k], ref[k]) for k in TENSORS}


def _dev(a):
    return torch.tensor(np.ascontiguousarray(a, dtype=np.float32), device=DEV)


def device_run(ctx, inputs, stride, tnc, want_dx=True):
    x, w, b, dy = (_dev(a) for a in inputs)
    if tnc:
        dy = dy.permute(2, 0, 1).contiguous()
    z, y = CD.layer_forward(ctx, x, w, b, stride, tnc)
    dx, dw, db = CD.layer_backward(ctx, dy, x, z, w, stride, tnc, want_dx)
    torch.cuda.current_stream().synchronize()
    out = dict(z=z.cpu().numpy(), y=y.cpu().numpy(), dx=None if dx is None else dx.cpu().numpy(), dw=dw.cpu().numpy(), db=db.cpu().numpy())
    if tnc:
        out["z"], out["y"] = CR.untnc(out["z"]), CR.untnc(out["y"])
    return out


def held(tag, got, ref, yards):
    """Every tensor against the restatement, with torch float32 as the yardstick; all are printed before any fails."""
    failed = []
    for name in TENSORS:
        g, r, yard = got[name], ref[name], yards[name]
        assert g.shape == r.shape, (name, g.shape, r.shape)
        err = rel(g, r)
        ratio = err / yard if yard else (0.0 if err == 0.0 else float("inf"))
        RATIOS.append((ratio, "%s %s" % (tag, name)))
        print("%-34s %-3s device %.3g  torch float32 %.3g  ratio %.2f" % (tag, name, err, yard, ratio))
        if not np.isfinite(g).all() or not err <= MARGIN * yard:
            failed.append((name, err, yard))
        if np.signbit(g[g == 0]).any():
            failed.append((name, "a zero written as -0"))
        if name == "dx" and (g[r == 0] != 0).any():                     # a stride above the window: positions no window covers
            failed.append((name, "a position no window covers is not zero"))
    assert not failed, failed


def runs():
    for c in CR.CASES:
        yield pytest.param(c, 0, id=CR.case_id(c))
        if not CR.is_narrow(c.Cin, c.Cout, c.K, c.stride):
            yield pytest.param(c, 1, id=CR.case_id(c) + "-tnc")


@pytest.mark.parametrize("case,tnc", list(runs()))
def test_layer_against_the_restatement(ctx, case, tnc):
    inputs, ref, yards = reference(case)
    got = device_run(ctx, inputs, case.stride, tnc)
    held(CR.case_id(case) + ("-tnc" if tnc else ""), got, ref, yards)


def test_narrow_layer_in_the_time_major_layout(ctx):
    case = CR.CASES[1]                                                  # the layout is the entry point's, not the route's
    inputs, ref, yards = reference(case)
    held(CR.case_id(case) + "-tnc", device_run(ctx, inputs, case.stride, 1), ref, yards)


@pytest.mark.parametrize("case", [CR.CASES[3], CR.CASES[4]], ids=CR.case_id)
def test_bytes(ctx, case):
    inputs, _, _ = reference(case)
    x, w, b, dy = inputs
    full = device_run(ctx, inputs, case.stride, 0)
    again = device_run(ctx, inputs, case.stride, 0)
    for name in TENSORS:                                                # a repeated call gives the same bytes
        assert np.isfinite(full[name]).all() and full[name].tobytes() == again[name].tobytes(), name
    no_dx = device_run(ctx, inputs, case.stride, 0, want_dx=False)      # dx = NULL: dw and db as they were
    assert no_dx["dx"] is None
    for name in ("z", "y", "dw", "db"):
        assert no_dx[name].tobytes() == full[name].tobytes(), name
    i = case.n - 1                                                      # a chunk alone and inside the batch
    alone = device_run(ctx, (x[i:i + 1], w, b, dy[i:i + 1]), case.stride, 0)
    for name in ("z", "y", "dx"):
        assert alone[name].tobytes() == full[name][i:i + 1].tobytes(), name
    assert alone["dw"].tobytes() != full["dw"].tobytes()


def test_malformed_arguments_are_refused_before_anything_is_launched(ctx):
    n, Cin, Lin, Cout, K, stride = 2, 4, 23, 16, 5, 1
    x, w, b = (torch.zeros(s, dtype=torch.float32, device=DEV) for s in ((n, Cin, Lin), (Cout, Cin, K), (Cout,)))
    outs = [torch.full(s, 7.0, dtype=torch.float32, device=DEV) for s in ((n, Cout, Lin), (n, Cout, Lin), (n, Cin, Lin), (Cout, Cin, K), (Cout,))]
    z, y, dx, dw, db = outs
    dy = torch.zeros((n, Cout, Lin), dtype=torch.float32, device=DEV)
    torch.cuda.synchronize()
    good = dict(n=n, Cin=Cin, Lin=Lin, Cout=Cout, K=K, stride=stride)

    def fwd(x=x, w=w, b=b, z=z, y=y, off=0, **k):
        a = dict(good, **k)
        p = lambda t: None if t is None else t.data_ptr() + off
        ctx.conv_train_forward_dev(p(x), p(w), p(b), a["n"], a["Cin"], a["Lin"], a["Cout"], a["K"], a["stride"], 0, p(z), p(y))

    def bwd(dy=dy, x=x, z=z, w=w, dx=dx, dw=dw, db=db, off=0, **k):
        a = dict(good, **k)
        p = lambda t: None if t is None else t.data_ptr() + off
        ctx.conv_train_backward_dev(p(dy), p(x), p(z), p(w), a["n"], a["Cin"], a["Lin"], a["Cout"], a["K"], a["stride"], 0, p(dx), p(dw), p(db))

    bad = [dict(n=0), dict(Cin=0), dict(Lin=0), dict(Cout=0), dict(K=0), dict(stride=0), dict(n=-1), dict(Lin=-5), dict(Cin=256, K=17), dict(off=4)]
    calls = [lambda k=k: fwd(**k) for k in bad] + [lambda k=k: bwd(**k) for k in bad]
    calls += [lambda t=t: fwd(**{t: None}) for t in ("x", "w", "b", "z", "y")]
    calls += [lambda t=t: bwd(**{t: None}) for t in ("dy", "x", "z", "w", "dw", "db")]
    calls.append(lambda: bwd(n=1 << 20, Cin=16, Lin=1 << 20, Cout=16, K=19, stride=5))             # 2^44 elements of x
    for call in calls:
        with pytest.raises(_lib.XbError, match="xb_conv_train_(forward|backward)") as e:
            call()
        assert e.value.code == _lib.XB_ERR_INVALID
    ctx.synchronize()
    for t in outs:                                                      # nothing was launched: every output is as it was
        assert bool((t == 7.0).all())
    fwd()                                                               # ... and the well-formed calls go through
    bwd(dx=None)
    ctx.synchronize()
    assert bool((z == b[0]).all()) and bool((dx == 7.0).all()) and bool((dw == 0).all())
