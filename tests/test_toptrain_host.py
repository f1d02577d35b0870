"""CPU: groundwork of a trainer for the head and the top LSTM layers -- the float64 restatement tests/toptrain_ref.py of its
arithmetic against torch float64 autograd, and the layout header csrc/xb_top_plan.h against its Python restatement (through
tools/top_plan_check.cpp, which is also run on its own under the address and undefined-behaviour sanitizers)."""
import os
import shutil
import subprocess

import numpy as np
import pytest
import torch

import toptrain_ref as TR

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


@pytest.mark.parametrize("L,F,C,rows", [(1, 16, 25, 15), (2, 32, 125, 120), (5, 96, 1296, 120), (2, 768, 1296, 720 * 98), (5, 768, 625, 720 * 384)])
def test_plan_against_its_restatement(plan_check, L, F, C, rows):
    out = subprocess.run([plan_check, str(L), str(F), str(C), str(rows)], capture_output=True, text=True, check=True).stdout.split("\n")
    want = TR.table(L, F, C, rows)
    assert [int(v) for v in out[:5]] == [0, 4 * L + 2, want["params"], want["stride"], want["bytes"]]
    pairs = [tuple(int(v) for v in line.split()) for line in out[5:5 + 4 * L + 2]]
    assert pairs == list(zip(want["off"], want["len"]))


def test_plan_refuses_what_it_cannot_lay_out(plan_check):
    for L in (0, 6):
        assert subprocess.run([plan_check, str(L), "16", "25", "1"], capture_output=True, text=True, check=True).stdout.split() == ["1"]
