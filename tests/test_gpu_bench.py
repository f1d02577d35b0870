"""GPU: bench.py end to end at a small workload -- one JSON line whose steps and ms_per_step are those of the timed steps, and
--dump-outputs writes what the library's host API computes from the same seeded signal and weights."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from conftest import ROOT
from xna_basecaller_amd import _lib
from xna_basecaller_amd.synthetic import seeded_weights

pytestmark = pytest.mark.gpu


def test_bench_dump_outputs_are_the_timed_paths_results(tmp_path):
    import torch
    N, L, F, nb, K = 64, 2000, 768, 6, 3
    out = tmp_path / "dump"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(K), "--warmup", "1",
                        "--batch", str(N), "--chunksize", str(L), "--cpu-chunks", "0", "--dump-outputs", str(out)],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-4000:]
    res = json.loads(lines[0])
    assert res["steps"] == K and res["ms_per_step"] > 0
    assert res["value"] == pytest.approx(N * L / (1e-3 * res["ms_per_step"]))
    T = res["config"]["T"]
    assert sorted(os.listdir(out)) == ["seq.npy", "seq_len.npy"]
    seq, lens = np.load(out / "seq.npy"), np.load(out / "seq_len.npy")
    assert seq.dtype == lens.dtype == np.float32 and seq.shape == (N, T) and lens.shape == (N,)

    # bench.py's inputs: the signal from a device generator seeded with 25 (rank 0), seeded_weights
    gen = torch.Generator(device="cuda:0")
    gen.manual_seed(25)
    x = torch.randn((N, L), dtype=torch.float32, device="cuda:0", generator=gen).cpu().numpy()
    ctx = _lib.Context(0, nb, 3, F, 19, 5, 5.0, 2.0, L, N, precision=_lib.XB_PREC_MIXED)
    ctx.load_state_dict(seeded_weights(F, nb))
    want_seq, want_len = ctx.basecall_chunks(x, "NACGTXY")
    ctx.close()
    assert np.array_equal(lens, want_len) and np.array_equal(seq, want_seq)
    assert res["called_bases_last_step"] == int(want_len.sum())


def _bench_line(*args):
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "2", "--warmup", "1",
                        "--batch", "64", "--chunksize", "2000"] + list(args), cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-4000:]
    lines = r.stdout.strip().splitlines()
    assert len(lines) == 1, r.stdout[-4000:]
    return json.loads(lines[0])


def test_bench_cpu_baseline_only_under_full():
    """A plain run prints the headline line without the CPU baseline; --full adds it (a small sample here) and nothing else."""
    plain = _bench_line()
    assert "cpu_baseline" not in plain
    full = _bench_line("--full", "--cpu-chunks", "2", "--cpu-repeats", "1")
    assert set(full) - set(plain) == {"cpu_baseline"} and set(plain) <= set(full)
    base = full["cpu_baseline"]
    assert base["value"] > 0 and base["unit"] == "samples/s" and base["kind"] == "port"
