#!/usr/bin/env python
"""GPU tool: the cost of the per-base letter probabilities (xb_decode_ub).
  1. xb_decode_dev, xb_decode_q_dev and xb_decode_ub_dev on HBM-resident 5*tanh scores (no blank column = the fused path's
     layout), device events of the decode stage, the three interleaved, median of REPS;
  2. Model.basecall_chunks plain and with ub_probs (one synchronous basecall step: H2D of the signal, encoder, decode, D2H),
     host clock around calls that end in a device synchronise, interleaved, median of REPS.
NB / N / T (decode) and F / L / BATCH (basecall) from the environment; defaults are the bench shape (nb 6, 512 chunks of 10 000
samples, T = 2000)."""
import json
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

from xna_basecaller_amd import _lib

QS, QO = 0.9722, 0.3498
REPS = int(os.environ.get("REPS", 7))


def decode_times(nb, N, T):
    S = nb ** 3
    alphabet = "NACGTXY"[:nb + 1]
    ctx = _lib.Context(0, nb, 3, 32, 19, 5, 5.0, 2.0, T * 5, N)
    g = torch.Generator(device="cuda")
    g.manual_seed(1)
    sc = 5 * torch.tanh(torch.randn((T, N, S * nb), device="cuda", generator=g))
    d_seq = torch.empty((N, T), dtype=torch.int8, device="cuda")
    d_q = torch.empty((N, T), dtype=torch.int8, device="cuda")
    d_mv = torch.empty((N, T), dtype=torch.uint8, device="cuda")
    d_len = torch.empty((N,), dtype=torch.int32, device="cuda")
    d_p = torch.empty((N, nb, T), dtype=torch.uint8, device="cuda")
    torch.cuda.synchronize()
    ctx.set_profiling(True)

    def plain():
        ctx.decode_dev(sc.data_ptr(), T, N, False, alphabet, None, d_seq.data_ptr(), d_len.data_ptr())

    def qual():
        ctx.decode_q_dev(sc.data_ptr(), T, N, False, alphabet, QS, QO, d_seq.data_ptr(), d_q.data_ptr(), d_mv.data_ptr(),
                         d_len.data_ptr())

    def ub():
        ctx.decode_ub_dev(sc.data_ptr(), T, N, False, alphabet, QS, QO, d_seq.data_ptr(), d_q.data_ptr(), d_mv.data_ptr(),
                          d_p.data_ptr(), d_len.data_ptr())

    out = {"plain": [], "q": [], "ub": []}
    for rep in range(REPS + 1):
        for name, fn in (("plain", plain), ("q", qual), ("ub", ub)):
            ctx.reset_stage_times()
            fn()
            ctx.synchronize()
            if rep:                                   # the first round warms up
                out[name].append(ctx.stage_times()["decode"][0])
    ctx.close()
    return {k: float(np.median(v)) for k, v in out.items()}, out


def basecall_times(F, nb, L, n):
    from conftest import make_config
    from xna_basecaller_amd.crf.model import Model
    from xna_basecaller_amd.synthetic import seeded_weights
    cfg = make_config(F, "NACGTXY"[:nb + 1])
    cfg["basecaller"] = {"batchsize": n, "chunksize": L, "overlap": 500}
    model = Model(cfg)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in seeded_weights(F, nb).items()})
    batch = np.random.default_rng(0).standard_normal((n, 1, L)).astype(np.float32)
    out = {"plain": [], "ub": []}
    for rep in range(REPS + 1):
        for name, u in (("plain", False), ("ub", True)):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            model.basecall_chunks(batch, ub_probs=u)           # returns after the device synchronise and the D2H copies
            dt = (time.perf_counter() - t0) * 1e3
            if rep:
                out[name].append(dt)
    return {k: float(np.median(v)) for k, v in out.items()}, out


def main():
    nb, N, T = int(os.environ.get("NB", 6)), int(os.environ.get("N", 512)), int(os.environ.get("T", 2000))
    F, L, n = int(os.environ.get("F", 768)), int(os.environ.get("L", 10000)), int(os.environ.get("BATCH", 512))
    res = {"source_digest": _lib.source_digest(), "reps": REPS}
    med, raw = decode_times(nb, N, T)
    res["decode"] = {"nb": nb, "N": N, "T": T, "plain_ms": med["plain"], "q_ms": med["q"], "ub_ms": med["ub"],
                     "ratio": med["ub"] / med["plain"], "ratio_to_q": med["ub"] / med["q"], "target_ratio": 1.15, "raw_ms": raw}
    print("decode   nb %d N %d T %d: xb_decode_dev %.3f ms, xb_decode_q_dev %.3f ms, xb_decode_ub_dev %.3f ms -> %.3fx the plain "
          "decode (target <= 1.15x), %.3fx the quality decode"
          % (nb, N, T, med["plain"], med["q"], med["ub"], med["ub"] / med["plain"], med["ub"] / med["q"]), flush=True)
    if os.environ.get("SKIP_BASECALL", "0") != "1":
        med, raw = basecall_times(F, nb, L, n)
        res["basecall"] = {"features": F, "nb": nb, "chunk_len": L, "batch": n, "plain_ms": med["plain"], "ub_ms": med["ub"],
                           "ratio": med["ub"] / med["plain"], "target_ratio": 1.03, "raw_ms": raw}
        print("basecall F %d nb %d L %d batch %d: basecall_chunks %.2f ms, with ub_probs %.2f ms -> %.3fx (target <= 1.03x)"
              % (F, nb, L, n, med["plain"], med["ub"], med["ub"] / med["plain"]), flush=True)
    print(json.dumps(res))


if __name__ == "__main__":
    main()
