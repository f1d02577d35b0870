"""CPU: groundwork of a trainer for the head and the top LSTM layers -- the float64 restatement tests/toptrain_ref.py of its
arithmetic against torch float64 autograd, and the layout header csrc/xb_top_plan.h against its Python restatement (through
tools/top_plan_check.cpp, which is also run on its own under the address and undefined-behaviour sanitizers).

The device test of the composed step (tests/test_gpu_toptrain.py) holds every tensor within MARGIN = 8 times the error of torch
float32 on the CPU.  That rule is only worth something where the yardstick is not degenerate -- where honest float32 arithmetic
of another order passes it with room -- so a float32 numpy stand-in for the device's chain (the operations of toptrain_ref.run
with every array float32, the derivatives grouped as the kernels group them) runs through the same cases under the same rule
here, wherever the suite runs."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import lstm_train_ref as R
import toptrain_ref as TR
import train_geometry_cases as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("L", [1, 2, 5])
def test_restatement_against_torch_float64(L):
    T, n, F, C, scale = 5, 3, 16, 25, 5.0
    rng = np.random.default_rng(40 + L)
    k = 2.0 / np.sqrt(F)
    tensors = []
    for _ in range(L):
        tensors += [rng.uniform(-k, k, (4 * F, F)), rng.uniform(-k, k, (4 * F, F)), rng.uniform(-k, k, 4 * F), rng.uniform(-k, k, 4 * F)]
    tensors += [rng.uniform(-k, k, (C, F)), rng.uniform(-k, k, C)]
    x0, dscores = rng.standard_normal((T, n, F)), rng.standard_normal((T, n, C))
    got, ref = TR.run(x0, tensors, scale, dscores), TR.torch_run(x0, tensors, scale, dscores, torch.float64)
    assert np.abs(got["scores"] - ref["scores"]).max() <= 1e-10 * np.abs(ref["scores"]).max()
    assert len(got["grads"]) == 4 * L + 2
    for i, (g, r) in enumerate(zip(got["grads"], ref["grads"])):
        assert g.shape == r.shape and np.abs(r).max() > 0, i
        assert np.abs(g - r).max() <= 1e-10 * np.abs(r).max(), (i, np.abs(g - r).max())
    for i in range(L):                                    # bias_ih and bias_hh receive the same gradient
        assert np.array_equal(got["grads"][4 * i + 2], got["grads"][4 * i + 3])
    assert TR.reverse_of(L, L - 1) and not TR.reverse_of(2, 0)           # encoder.8 runs backwards in time, encoder.7 forwards


# ---- the float32 stand-in ------------------------------------------------------------------------------------------------------
MARGIN = 8.0
f32 = np.float32


def _sigmoid32(x):
    return (f32(1) / (f32(1) + np.exp(-x))).astype(f32)


def forward32(gin, w_hh, reverse):
    T, n, G = gin.shape
    F = G // 4
    y, gates, c = np.zeros((T, n, F), f32), np.zeros((T, n, G), f32), np.zeros((T, n, F), f32)
    h, cc = np.zeros((n, F), f32), np.zeros((n, F), f32)
    for t in (range(T - 1, -1, -1) if reverse else range(T)):
        pre = gin[t] + h @ w_hh.T
        i, f, o = _sigmoid32(pre[:, :F]), _sigmoid32(pre[:, F:2 * F]), _sigmoid32(pre[:, 3 * F:])
        g = np.tanh(pre[:, 2 * F:3 * F])
        cc = f * cc + i * g
        h = o * np.tanh(cc)
        gates[t], c[t], y[t] = np.concatenate([i, f, g, o], axis=1), cc, h
    return y, gates, c


def backward32(dy, w_hh, gates, c, reverse):
    T, n, F = dy.shape
    one = f32(1)
    dgin = np.zeros((T, n, 4 * F), f32)
    order = list(range(T - 1, -1, -1) if reverse else range(T))
    carry, later = np.zeros((n, F), f32), None
    for k in range(T - 1, -1, -1):
        t = order[k]
        i, f, g, o = (gates[t][:, a * F:(a + 1) * F] for a in range(4))
        c_prev = c[order[k - 1]] if k else np.zeros((n, F), f32)
        dh = dy[t] + dgin[later] @ w_hh if later is not None else dy[t]
        th = np.tanh(c[t])
        dc = (dh * o) * ((one - th) * (one + th)) + carry
        carry = dc * f
        dgin[t] = np.concatenate([(dc * g) * (i * (one - i)), (dc * c_prev) * (f * (one - f)), (dc * i) * ((one - g) * (one + g)),
                                  (dh * th) * (o * (one - o))], axis=1)
        later = t
    return dgin


def run32(x0, tensors, scale, dscores):
    """toptrain_ref.run with every array float32."""
    t = [np.asarray(a, f32) for a in tensors]
    L = (len(t) - 2) // 4
    x, scale = np.asarray(x0, f32), f32(scale)
    T, n, F = x.shape
    rows = T * n
    keep = []
    for i in range(L):
        w_ih, w_hh, b_ih, b_hh = t[4 * i:4 * i + 4]
        rev = TR.reverse_of(L, i)
        y, gates, c = forward32(x @ w_ih.T + (b_ih + b_hh), w_hh, rev)
        keep.append((x, y, gates, c, rev))
        x = y
    W, b = t[-2], t[-1]
    scores = scale * np.tanh(x @ W.T + b)
    dz = np.asarray(dscores, f32) * ((scale - scores) * (scale + scores) / scale)
    d2 = dz.reshape(rows, -1)
    grads = [None] * len(t)
    grads[-2], grads[-1] = d2.T @ x.reshape(rows, F), d2.sum(axis=0)
    dy = dz @ W
    for i in range(L - 1, -1, -1):
        w_ih, w_hh = t[4 * i], t[4 * i + 1]
        xin, y, gates, c, rev = keep[i]
        dgin = backward32(dy, w_hh, gates, c, rev)
        g2 = dgin.reshape(rows, 4 * F)
        db = g2.sum(axis=0)
        grads[4 * i:4 * i + 4] = [g2.T @ xin.reshape(rows, F), g2.T @ R.h_prev(y, rev).reshape(rows, F), db, db.copy()]
        dy = dgin @ w_ih
    assert scores.dtype == f32 and all(g.dtype == f32 for g in grads)
    return dict(scores=scores, grads=grads)


@pytest.mark.parametrize("case", TR.CASES, ids=TR.case_id)
def test_float32_stand_in_passes_the_device_tests_rule(case):
    x0, tensors, dscores = TR.draw(case)
    ref = TR.run(x0, tensors, 5.0, dscores)
    t32 = TR.torch_run(x0, tensors, 5.0, dscores, torch.float32)
    got = run32(x0, tensors, 5.0, dscores)
    rows = [("scores", got["scores"], ref["scores"], t32["scores"])] + [("grad %d" % i, g, r, t) for i, (g, r, t) in
                                                                        enumerate(zip(got["grads"], ref["grads"], t32["grads"]))]
    worst = 0.0
    for what, g, r, t in rows:
        err, yard = R.rel(g, r), R.rel(t, r)
        print("%-10s stand-in %.3g  torch float32 %.3g  ratio %.2f" % (what, err, yard, err / yard if yard else 0.0))
        if np.abs(r).max() > 0:
            assert yard > 0, what                          # torch float32 bit-equal to float64 would make the rule empty
            worst = max(worst, err / yard)
        assert err <= MARGIN * yard, (what, err, yard)
    print("largest ratio %.2f" % worst)


@pytest.fixture(scope="module")
def plan_check(tmp_path_factory):
    cxx = shutil.which("g++") or shutil.which("c++")
    assert cxx is not None, "the check program needs the C++ compiler the oracle is built with"
    exe = str(tmp_path_factory.mktemp("plan") / "top_plan_check")
    subprocess.check_call([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                           os.path.join(ROOT, "tools", "top_plan_check.cpp"), "-o", exe])
    return exe


def test_plan_check_program_passes_under_the_sanitizers(plan_check):
    out = subprocess.run([plan_check], capture_output=True, text=True)
    assert out.returncode == 0 and "all checks passed" in out.stdout, out.stdout + out.stderr


@pytest.mark.parametrize("L,F,C,rows", [(1, 16, 25, 15), (2, 32, 125, 120), (5, 96, 1296, 120), (2, 768, 1296, 720 * 98), (5, 768, 625, 720 * 384)]
                         + [(L, c.F, G.columns(c), G.steps(c)[2] * c.n) for c in G.CASES for L in (2, 5)])      # the trainers' geometries on the device
def test_plan_against_its_restatement(plan_check, L, F, C, rows):
    out = subprocess.run([plan_check, str(L), str(F), str(C), str(rows)], capture_output=True, text=True, check=True).stdout.split("\n")
    want = TR.table(L, F, C, rows)
    assert [int(v) for v in out[:5]] == [0, 4 * L + 2, want["params"], want["stride"], want["bytes"]]
    pairs = [tuple(int(v) for v in line.split()) for line in out[5:5 + 4 * L + 2]]
    assert pairs == list(zip(want["off"], want["len"]))


def test_plan_refuses_what_it_cannot_lay_out(plan_check):
    for L in (0, 6):
        assert subprocess.run([plan_check, str(L), "16", "25", "1"], capture_output=True, text=True, check=True).stdout.split() == ["1"]
