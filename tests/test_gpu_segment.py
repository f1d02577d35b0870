"""GPU: xb_dtw_segment through the C ABI and the `segment` CLI against the CPU restatement of its contract (tests/dtw_ref.py):
breakpoints, ok and the bit pattern of the cost EQUAL, no case excluded.  dtw-python is in no image: parity unpinned, the
contract is the header's."""
import os
import subprocess
import sys

import numpy as np
import pytest

import dtw_cases
import dtw_ref
from conftest import ROOT

pytestmark = pytest.mark.gpu


def _ctx():
    from xna_basecaller_amd import _lib
    _lib.require_gpu()
    return _lib.Context(0, 6, 3, 64, 19, 5, 5.0, 2.0, 1000, 4)


def _check(ctx, signal, levels, rep, window=None, kmax=None):
    """The device call equals dtw_ref on every output; returns (breakpoints, ok, cost, ties)."""
    got_bp, got_ok, got_cost = ctx.dtw_segment(signal, levels, rep, window, kmax)
    bp, ok, cost, ties = dtw_ref.dtw_batch(signal, levels, rep, window, kmax)
    assert np.array_equal(got_ok, ok), (np.flatnonzero(got_ok != ok)[:5], [len(v) for v in levels])
    bad = np.flatnonzero(got_cost.view(np.uint64) != cost.view(np.uint64))
    assert bad.size == 0, (bad[:5], got_cost[bad[:5]], cost[bad[:5]])
    bad = np.flatnonzero((got_bp != bp).any(axis=1))
    assert bad.size == 0, (bad[:5], [(len(levels[b]), got_bp[b][:12], bp[b][:12]) for b in bad[:2]])
    return bp, ok, cost, ties


@pytest.mark.parametrize("rep", [1, 2, 3, 6])
@pytest.mark.parametrize("N", [1, 2, 63, 64, 65, 1000, 3600])
def test_sizes_and_level_counts(N, rep):
    """Mixed K within one call, from one level to more than fit (M > N fails and gives the naive split): one, two and four
    columns per lane, stripes exactly full and one column over."""
    ctx = _ctx()
    rng = np.random.default_rng(1000 * N + rep)
    Ks = dtw_cases.level_counts(N, rep)
    signal, levels = dtw_cases.batch(rng, N, Ks)
    bp, ok, cost, _ = _check(ctx, signal, levels, rep, kmax=max(Ks) + 2)
    for c, K in enumerate(Ks):
        assert ok[c] == (K * rep <= N)
        assert bp[c, K - 1] == N and (bp[c, K:] == 0).all()
        if ok[c]:
            assert (np.diff(np.concatenate(([0], bp[c, :K]))) >= rep).all()
        else:
            assert np.array_equal(bp[c, :K], dtw_ref.naive_breakpoints(N, K)) and np.isinf(cost[c])
    ctx.close()


@pytest.mark.parametrize("rep", [1, 2, 3, 6])
def test_ten_thousand_samples(rep):
    ctx = _ctx()
    N = 10000
    rng = np.random.default_rng(rep)
    Ks = [1, 400, N // rep // 2, N // rep, N // rep + 1]
    signal, levels = dtw_cases.batch(rng, N, Ks)
    _check(ctx, signal, levels, rep)
    ctx.close()


@pytest.mark.parametrize("n", [1, 3, 257])
def test_batches_span_several_launches(n, monkeypatch):
    """A scratch bound of 1 MB (XB_DTW_SCRATCH_MB) holds 16 of these chunks: 257 chunks take 17 launches; the bytes equal the
    default bound's."""
    ctx = _ctx()
    rng = np.random.default_rng(n)
    Ks = [int(k) for k in rng.integers(1, 340, n)]
    signal, levels = dtw_cases.batch(rng, 1000, Ks)
    whole = ctx.dtw_segment(signal, levels, 3)
    monkeypatch.setenv("XB_DTW_SCRATCH_MB", "1")
    _check(ctx, signal, levels, 3)
    split = ctx.dtw_segment(signal, levels, 3)
    for a, b in zip(whole, split):
        assert np.array_equal(a, b)
    ctx.close()


@pytest.mark.parametrize("N,rep", [(65, 1), (1000, 3), (3600, 3), (3600, 1)])
def test_quantised_inputs_tie(N, rep):
    """fp16 chunk values and levels in quarters: predecessors tie outside the repeated columns too (rep = 1 has no repeated
    columns at all), and the stay-first rule decides."""
    ctx = _ctx()
    rng = np.random.default_rng(7 * N + rep)
    Ks = [max(1, N // rep // 3), max(1, N // rep // 2), max(1, N // rep - 3)]
    signal, levels = dtw_cases.batch(rng, N, Ks, quantised=True)
    _, ok, _, ties = _check(ctx, signal, levels, rep)
    assert ok.all() and ties > 100 * len(Ks), ties
    ctx.close()


def test_bands():
    """No band, a band wider than the lattice (equal to none), and bands narrow enough that some chunks fail and others do
    not; a failed chunk does not disturb its neighbours."""
    ctx = _ctx()
    rng = np.random.default_rng(5)
    N, rep = 1000, 3
    Ks = [100, 333, 50, 200, 7, 300, 120]
    signal, levels = dtw_cases.batch(rng, N, Ks)
    free = _check(ctx, signal, levels, rep)
    wide = _check(ctx, signal, levels, rep, window=np.full(len(Ks), 5000.0))
    for a, b in zip(free[:3], wide[:3]):
        assert np.array_equal(a, b)
    mixed = np.array([(N / K) * w for K, w in zip(Ks, [30, 30, 0, -1, 1, 0, 2])])      # window_size in mean samples per base
    bp, ok, cost, _ = _check(ctx, signal, levels, rep, window=mixed)
    assert ok.any() and not ok.all(), ok
    assert np.array_equal(bp[3], free[0][3]) and cost[3] == free[2][3]                  # the unbanded chunk among them
    narrow = np.array([(N / K) * 1.0 for K in Ks])
    bp1, ok1, _, _ = _check(ctx, signal, levels, rep, window=narrow)
    # every chunk on its own gives what it gave inside the batch
    for c in range(len(Ks)):
        one = ctx.dtw_segment(signal[c:c + 1], levels[c:c + 1], rep, narrow[c:c + 1], bp1.shape[1])
        assert np.array_equal(one[0][0], bp1[c]) and one[1][0] == ok1[c]
    # full-size chunks under the CLI's kind of band
    signal, levels = dtw_cases.batch(rng, 3600, [400, 380, 1200])
    _check(ctx, signal, levels, rep, window=np.array([(3600 / K) * 5.0 for K in (400, 380, 1200)]))
    ctx.close()


def test_host_and_dev_forms_agree():
    import torch
    ctx = _ctx()
    rng = np.random.default_rng(2)
    N, rep = 1000, 3
    Ks = [100, 400, 333, 1, 150]                                # one chunk that fails (400 x 3 > 1000)
    signal, levels = dtw_cases.batch(rng, N, Ks)
    window = np.array([-1.0, 10.0, 40.0, -1.0, 2.0])
    host = ctx.dtw_segment(signal, levels, rep, window)
    flat, off = ctx._dtw_offsets(levels)
    dev = torch.device("cuda:0")
    d_sig, d_lev, d_win = (torch.from_numpy(a).to(dev) for a in (signal, flat, window))
    kmax = host[0].shape[1]
    d_bp = torch.full((len(Ks), kmax), -7, dtype=torch.int32, device=dev)
    d_ok = torch.full((len(Ks),), -7, dtype=torch.int8, device=dev)
    d_cost = torch.zeros(len(Ks), dtype=torch.float64, device=dev)
    torch.cuda.synchronize()
    for _ in range(3):                                          # back to back: the offsets' pinned slots rotate
        ctx.dtw_segment_dev(d_sig.data_ptr(), len(Ks), N, d_lev.data_ptr(), off, rep, d_win.data_ptr(), kmax, d_bp.data_ptr(),
                            d_ok.data_ptr(), d_cost.data_ptr())
    ctx.synchronize()
    assert np.array_equal(d_bp.cpu().numpy(), host[0]) and np.array_equal(d_ok.cpu().numpy().astype(bool), host[1])
    assert np.array_equal(d_cost.cpu().numpy().view(np.uint64), host[2].view(np.uint64))
    assert ctx.dtw_scratch_bytes() > 0
    ctx.close()


def test_invalid_arguments_leave_the_context_usable():
    from xna_basecaller_amd import _lib
    ctx = _ctx()
    rng = np.random.default_rng(0)
    signal, levels = dtw_cases.batch(rng, 100, [10, 20])
    for kwargs, word in ((dict(ref_rep=0), "ref_rep"), (dict(ref_rep=3, kmax=19), "19 entries")):
        with pytest.raises(_lib.XbError) as e:
            ctx.dtw_segment(signal, levels, **kwargs)
        assert e.value.code == _lib.XB_ERR_INVALID and word in str(e.value), str(e.value)
    with pytest.raises(_lib.XbError) as e:                      # 30000 levels x 3 columns
        ctx.dtw_segment(signal[:1], [np.zeros(30000)], 3)
    assert e.value.code == _lib.XB_ERR_INVALID and "90000 columns" in str(e.value)
    with pytest.raises(_lib.XbError) as e:                      # a chunk without levels
        ctx.dtw_segment(signal, [levels[0], np.zeros(0)], 3, kmax=10)
    assert e.value.code == _lib.XB_ERR_INVALID
    with pytest.raises(_lib.XbError) as e:
        ctx.dtw_segment(np.zeros((1, 65536), np.float32), [np.zeros(4)], 3)
    assert e.value.code == _lib.XB_ERR_INVALID and "65535" in str(e.value)
    _check(ctx, signal, levels, 3)
    ctx.close()


def test_cli_end_to_end(tmp_path):
    """A synthetic ctc-data directory -> `segment` -> breakpoints.npy equals segment.py driven with dtw_ref in place of the
    device; with a band and a suffix too.  Sanity, not contract: the recovered breakpoints lie within 3 samples of the planted
    ones for most bases -- dtw_ref alone, on the host, measures 0.9443 on these inputs (dtw_cases.PLANTED_WITHIN_3 = 0.93 is
    that with a small margin; test_segment_host.py asserts it without a device)."""
    from xna_basecaller_amd import segment as seg
    model = dtw_cases.write_poremodel(str(tmp_path / "synthetic.model"))
    poremodel = seg.load_kmer_poremodel(model)
    ctc = str(tmp_path / "ctc")
    planted = dtw_cases.write_ctc_dir(ctc, poremodel)
    chunks, targets, lengths = (np.load(os.path.join(ctc, f)) for f in ("chunks.npy", "references.npy", "reference_lengths.npy"))
    base = [sys.executable, "-m", "xna_basecaller_amd", "segment", ctc, "-r", model]
    for extra, name, kwargs in (([], "breakpoints.npy", {}),
                                (["-w", "4", "-S", "w4", "--seed", "3", "--batchsize", "5"], "breakpoints-w4.npy",
                                 dict(window_size=4, seed=3))):
        r = subprocess.run(base + extra, cwd=ROOT, capture_output=True, text=True, timeout=600)
        assert r.returncode == 0, r.stderr
        got = np.load(os.path.join(ctc, name))
        want, ok = seg.segment(chunks, targets, lengths, poremodel, dtw=dtw_ref.device_stand_in, **kwargs)
        assert got.dtype == np.uint16 and got.shape == targets.shape and np.array_equal(got, want)
        assert ok.all()
    got = np.load(os.path.join(ctc, "breakpoints.npy"))
    close = np.concatenate([np.abs(got[c, :len(p)].astype(int) - p) <= 3 for c, p in enumerate(planted)])
    assert close.mean() >= dtw_cases.PLANTED_WITHIN_3, close.mean()
