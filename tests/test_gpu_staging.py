"""GPU: the host-pointer forms of the ctc-data tools share one staging buffer (xb_ctx::staging).  On ONE context they run back
to back -- small, then large enough that the buffer is regrown, then small again inside the larger buffer -- and every
result is bit-equal to the same call on a fresh context.  What each call computes is the feature tests' business."""
import numpy as np
import pytest

import dtw_cases
import map_ref
import splice_cases
from test_gpu_map import KEYS
from test_gpu_savectc import LENIENT, _ctx, _library

pytestmark = pytest.mark.gpu

TEMPLATES = ["ACGTTGCANGTCAGGCTAAC", "TTGACCATGGNCATGCAAGTCCGATTAGCA", "GGCATCAGTTNACGGTCAATGCCGTANTGCAAGCTTGACC"]    # 20, 30, 40
W = 32
ALPHABET = list("NACGTXY")


def _revcomp(s):
    return s[::-1].translate(str.maketrans("ACGTXY", "TGCAYX"))


def _reads(count, seed):
    """Calls off the templates, at most W letters: the N called X, a substitution here and there, both strands."""
    rng = np.random.default_rng(seed)
    reads = []
    for k in range(count):
        s = list(TEMPLATES[k % 3].replace("N", "X"))
        for at in np.flatnonzero(rng.random(len(s)) < 0.05):
            s[at] = str(rng.choice(list("ACGT")))
        s = "".join(s)[int(rng.integers(0, 4)):][:W]
        reads.append(_revcomp(s) if k % 2 else s)
    return reads


def _arrays(result):
    if isinstance(result, dict):
        return [(k, result[k]) for k in sorted(result)]
    if isinstance(result, tuple):
        return [(str(i), a) for i, a in enumerate(result)]
    return [(k, getattr(result, k)) for k in ("reads", "err", "cm")]              # the UB accumulators


def _same(got, want, what):
    assert [k for k, _ in _arrays(got)] == [k for k, _ in _arrays(want)], what
    for (k, a), (_, b) in zip(_arrays(got), _arrays(want)):
        if not isinstance(a, np.ndarray):
            _same(a, b, (what, k))
            continue
        assert a.dtype == b.dtype and a.shape == b.shape, (what, k, a.dtype, b.dtype, a.shape, b.shape)
        assert a.tobytes() == b.tobytes(), (what, k, np.flatnonzero(a.ravel() != b.ravel())[:8])


def test_host_forms_back_to_back_on_one_context_equal_fresh_contexts():
    import torch
    lib, off = _library(TEMPLATES)
    rows, lens = map_ref.pack_rows(_reads(3, 1), W)
    big_rows, big_lens = map_ref.pack_rows(_reads(300, 2), W)
    rng = np.random.default_rng(3)
    signal, levels = dtw_cases.batch(rng, 64, [8, 8])
    band = np.array([12.0, -1.0])
    chunks = splice_cases.random_set(4, 2, 64)
    xna = splice_cases.library("full")
    calls_signal = rng.standard_normal((2, 200)).astype(np.float32)
    state = {}                                          # "mapped": what step 1 gave on the shared context

    def splice(ctx):
        ctx.splice_library(xna.pool, xna.rows, xna.table)
        return ctx.splice_chunks(*chunks, 0, 77, ubs_mask=3, prop=0.3, var_prop=0.0, cand_sample_size=10, pad=2)

    steps = [
        ("map", lambda ctx: ctx.map_templates(rows, lens, lib, off)),
        ("ub_tally", lambda ctx: ctx.ub_tally(rows, lens, state["mapped"], lib, off)),
        ("ctc_targets", lambda ctx: ctx.ctc_targets(lens, W, state["mapped"], lib, off, min_accuracy=0.8, min_coverage=0.5)),
        ("dtw", lambda ctx: ctx.dtw_segment(signal, levels, 1)),
        ("dtw band", lambda ctx: ctx.dtw_segment(signal, levels, 1, band)),
        ("splice", splice),
        ("map 300 rows", lambda ctx: ctx.map_templates(big_rows, big_lens, lib, off)),
        ("dtw again", lambda ctx: ctx.dtw_segment(signal, levels, 1)),
        ("ctc_chunks", lambda ctx: ctx.ctc_chunks(calls_signal, ALPHABET, lib, off, LENIENT, min_accuracy=0.5, min_coverage=0.3)),
    ]
    ctx = _ctx(max_batch=2, chunk_len=200, weights=True)
    main_stream = ctx.result_stream()                   # no _dev call yet: the main stream
    shared = []
    for name, call in steps:
        shared.append(call(ctx))
        state.setdefault("mapped", shared[0])
        if name == "ctc_targets":                       # a _dev call between two host calls: it leaves the staging alone
            dev = torch.device("cuda:0")
            d_seq, d_len = torch.from_numpy(rows).to(dev), torch.from_numpy(lens).to(dev)
            d_out = {k: torch.zeros(shared[0][k].shape, dtype=getattr(torch, str(shared[0][k].dtype)), device=dev) for k in KEYS}
            torch.cuda.synchronize()
            ctx.map_templates_dev(d_seq.data_ptr(), d_len.data_ptr(), 3, W, lib, off, (2, 4, 4, 2, 1), {k: v.data_ptr() for k, v in d_out.items()})
            ctx.synchronize()
            _same({k: v.cpu().numpy() for k, v in d_out.items()}, shared[0], "map _dev")
    assert ctx.result_stream() == main_stream and main_stream != 0
    ctx.close()
    assert (shared[0]["tmpl"] >= 0).all() and (shared[6]["tmpl"] >= 0).sum() > 250 and shared[3][1].all() and shared[5][3].sum() > 0
    for (name, call), got in zip(steps, shared):
        fresh = _ctx(max_batch=2, chunk_len=200, weights=name == "ctc_chunks")
        _same(got, call(fresh), name)
        fresh.close()
