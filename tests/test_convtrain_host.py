"""CPU: groundwork of the convolutions' training -- the float64 restatement tests/convtrain_ref.py against torch float64 autograd
(conv1d + silu), and the layout header csrc/xb_conv_plan.h against its Python restatement (through tools/conv_plan_check.cpp,
which is also run on its own under the address and undefined-behaviour sanitizers).

The device test (tests/test_gpu_convtrain.py) holds z, y, dx, dw and db within MARGIN = 8 times the error of torch float32 on the
CPU, per tensor, relative to the tensor's maximum.  That rule is only worth something where the yardstick is not degenerate, so a
naive float32 numpy stand-in (im2col and matmul in float32, db as a product with a row of ones) runs through the same cases under the
same rule here."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import convtrain_ref as CR
import train_geometry_cases as G
from lstm_train_ref import rel

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARGIN = 8.0
f32 = np.float32
TENSORS = ("z", "y", "dx", "dw", "db")


@pytest.mark.parametrize("case", [c for c in CR.CASES if c.n * c.Lin <= 1000] + [CR.Case(2, 3, 5, 4, 2, 11, False), CR.Case(2, 2, 3, 1, 1, 9, False)],
                         ids=CR.case_id)
def test_restatement_against_torch_float64(case):
    x, w, b, dy = (a.astype(np.float64) for a in CR.draw(case))
    z, y = CR.forward(x, w, b, case.stride)
    dx, dw, db = CR.backward(dy, x, z, w, case.stride)
    ref = CR.torch_run(x, w, b, dy, case.stride, torch.float64)
    assert z.shape == (case.n, case.Cout, CR.out_len(case.Lin, case.K, case.stride))
    for name, got in zip(TENSORS, (z, y, dx, dw, db)):
        assert got.shape == ref[name].shape and np.abs(ref[name]).max() > 0, name
        assert rel(got, ref[name]) <= 1e-12, (name, rel(got, ref[name]))
    assert np.array_equal(CR.untnc(CR.tnc(z)), z) and CR.tnc(z).shape == (z.shape[2], case.n, case.Cout)


@pytest.mark.parametrize("case,zeros", [(CR.Case(2, 16, 32, 3, 8, 50, False), 0.60), (CR.Case(3, 16, 32, 1, 3, 40, False), 0.65)], ids=lambda v: CR.case_id(v) if isinstance(v, tuple) else None)
def test_a_stride_above_the_window_leaves_exact_zeros_in_dx(case, zeros):
    """The positions no window covers: what the device test's check of dx's zeros (tests/test_gpu_convtrain.py: held) acts on."""
    assert case in CR.CASES and case.stride > case.K
    x, w, b, dy = CR.draw(case)
    z, _ = CR.forward(x, w, b, case.stride)
    dx = CR.backward(dy, x, z, w, case.stride)[0]
    t = np.arange(z.shape[2])[:, None] * case.stride + np.arange(case.K)[None, :] - case.K // 2
    covered = np.zeros(case.Lin, bool)
    covered[t[(t >= 0) & (t < case.Lin)]] = True
    assert (dx[:, :, ~covered] == 0).all() and (dx[:, :, covered] != 0).all() and abs((dx == 0).mean() - zeros) < 1e-12
    assert (CR.torch_run(x, w, b, dy, case.stride, torch.float64)["dx"][:, :, ~covered] == 0).all()


def run32(x, w, b, dy, stride):
    """The layer with every array float32: im2col and matmul, numpy's float32 sums."""
    Cout, Cin, K = w.shape
    n, _, Lin = x.shape
    pad = K // 2
    col = CR.windows(x, K, stride)                                             # (n, Lout, Cin, K) float32
    Lout = col.shape[1]
    c2 = col.reshape(n * Lout, Cin * K)
    z2 = c2 @ w.reshape(Cout, Cin * K).T + b
    s = (f32(1) / (f32(1) + np.exp(-z2))).astype(f32)
    y2 = z2 * s
    dz = dy.transpose(0, 2, 1).reshape(n * Lout, Cout) * (s * (f32(1) + z2 * (f32(1) - s)))
    dw, db = (dz.T @ c2).reshape(Cout, Cin, K), np.ones(n * Lout, f32) @ dz             # db as a product too
    dcol = (dz @ w.reshape(Cout, Cin * K)).reshape(n, Lout, Cin, K)
    dxp = np.zeros((n, Cin, Lin + 2 * pad + stride), f32)
    for t in range(Lout):
        dxp[:, :, t * stride:t * stride + K] += dcol[:, t]
    out = dict(z=z2.reshape(n, Lout, Cout).transpose(0, 2, 1), y=y2.reshape(n, Lout, Cout).transpose(0, 2, 1), dx=dxp[:, :, pad:pad + Lin], dw=dw, db=db)
    assert all(a.dtype == f32 for a in out.values())
    return out


@pytest.mark.parametrize("case", CR.CASES, ids=CR.case_id)
def test_float32_stand_in_passes_the_device_tests_rule(case):
    x, w, b, dy = CR.draw(case)
    z, y = CR.forward(x, w, b, case.stride)
    ref = dict(zip(TENSORS, (z, y) + CR.backward(dy, x, z, w, case.stride)))
    t32 = CR.torch_run(x, w, b, dy, case.stride, torch.float32)
    got = run32(x, w, b, dy, case.stride)
    worst = 0.0
    for name in TENSORS:
        err, yard = rel(got[name], ref[name]), rel(t32[name], ref[name])
        print("%-3s stand-in %.3g  torch float32 %.3g  ratio %.2f" % (name, err, yard, err / yard if yard else 0.0))
        assert np.abs(ref[name]).max() > 0 and yard > 0, name          # torch float32 bit-equal to float64 would make the rule empty
        worst = max(worst, err / yard)
        assert err <= MARGIN * yard, (name, err, yard)
    print("largest ratio %.2f" % worst)
    assert worst <= 6.0                                                # room between honest float32 arithmetic and the margin


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the check program needs the C++ compiler the oracle is built with"
    exe = str(tmp_path_factory.mktemp("plan") / "conv_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "conv_plan_check.cpp"), "-o", exe])
    return exe


def test_plan_check_program_passes_under_the_sanitizers(plan_check):
    out = subprocess.run([plan_check], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("chunk,F,W,S,n", [(200, 32, 19, 5, 6), (1000, 32, 19, 5, 16), (3600, 768, 19, 5, 98), (4000, 96, 9, 3, 384), (23, 48, 19, 5, 3)]
                         + [(c.chunk, c.F, c.W, c.S, c.n) for c in G.CASES])        # the geometries the trainers run at on the device
def test_plan_against_its_restatement(plan_check, chunk, F, W, S, n):
    out = subprocess.run([plan_check] + [str(v) for v in (chunk, F, W, S, n)], capture_output=True, text=True, check=True).stdout.split("\n")
    want = CR.table(chunk, F, W, S, n)
    assert [int(v) for v in out[:6]] == [0, want["params"], want["L1"], want["L2"], want["T"], want["act_floats"]]
    assert want["params"] == 360 + F * (16 * W + 1)
    pairs = [tuple(int(v) for v in line.split()) for line in out[6:12]]
    assert pairs == list(zip(want["off"], want["len"]))
    assert [int(v) for v in out[12].split()] == want["act"]


def test_route_rule_against_its_restatement(plan_check):
    shapes = [(c.Cin, c.Cout, c.K, c.stride) for c in CR.CASES] + [(4, 16, 5, 2), (4, 17, 5, 1), (17, 4, 1, 1), (1, 16, 64, 1), (1, 16, 65, 1), (16, 16, 4, 1)]
    for s in shapes:
        out = subprocess.run([plan_check] + [str(v) for v in s], capture_output=True, text=True, check=True).stdout.split()
        assert out == [str(int(CR.is_narrow(*s)))], s
    assert [CR.is_narrow(c.Cin, c.Cout, c.K, c.stride) for c in CR.CASES[:10]] == [True] * 4 + [False] * 6
    assert CR.narrow_blocks(6, 1000, 5) == 24                           # several workgroups' partials at the cases of 1000 samples


def test_plan_refuses_what_it_cannot_lay_out(plan_check):
    for args in ((0, 32, 19, 5, 1), (200, 32, 257, 5, 1), (200, 32, 19, 0, 1)):
        assert subprocess.run([plan_check] + [str(v) for v in args], capture_output=True, text=True, check=True).stdout.split() == ["1"]
