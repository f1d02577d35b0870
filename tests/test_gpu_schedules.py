"""GPU: every encoder schedule the host scheduler (plan_layer, executed by run_lstm_layer) can pick, at the shapes the CLI runs, against the serial
one-launch-per-step order -- byte for byte -- and, on a few seam chunks, against the fp32 oracle.

The table (tests/schedule_plan.py ROWS / PAIR_ROWS) covers uneven time slabs (T 800 / 720 in 6 / 5 slabs), one and two
slabs, T = 1..3, the batch seams of the wide placement, the two-groups-per-workgroup kernel, several chunk slabs with a
single-group tail, batches above 64 group slots, signal mode off its default, 64 and 80 time slabs, the documented knobs
and co-scheduled pairs of calls.

  * reference: a fresh context in the serial order (schedule_plan.REFERENCE_ENV, lstm_mode 1) over a bank of chunks per
    geometry; a chunk's result does not depend on its place in the batch, so every row compares with slices of the bank;
  * schedule: a fresh context with the row's knobs gets two different batches A = bank[0:N] and B = bank[1:N + 1] back to
    back with one synchronize at the end (a schedule that reads the previous call's rows shows up in B);
  * the scores (encode_dev) and the fused path's seq / len (basecall_chunks_dev) are compared on the device;
  * the stage counters show that the row took the plan schedule_plan.plan() predicts for it (launch counts per stage).
"""
import numpy as np
import pytest

import oracle
import schedule_plan as sp
from xna_basecaller_amd import _lib
from xna_basecaller_amd.synthetic import encoder_shapes, seeded_state_dict

pytestmark = pytest.mark.gpu

SL, SEED = 3, 31
ALPHABET = "NACGTXY"
COUNTED = ("conv", "lstm_in", "lstm_rec", "linear")


def _key(F, nb, L):
    return (F, nb, L)


def _bank_sizes():
    """Chunks each geometry's bank needs: N + 1 for a row (A and B), the sum of the calls for a pairing row."""
    need = {}
    for _, F, nb, L, N, _, _, _ in sp.ROWS:
        need[_key(F, nb, L)] = max(need.get(_key(F, nb, L), 0), N + 1)
    for _, F, nb, L, _, calls, _ in sp.PAIR_ROWS:
        need[_key(F, nb, L)] = max(need.get(_key(F, nb, L), 0), sum(calls))
    return need


BANK = _bank_sizes()
_cache = {}


def _clear_knobs(monkeypatch):
    for name in sp.DEFAULTS:
        monkeypatch.delenv(name, raising=False)


def _context(F, nb, L, max_batch, lstm_mode=0):
    ctx = _lib.Context(0, nb, SL, F, 19, 5, 5.0, 2.0, L, max_batch, precision=_lib.XB_PREC_MIXED, lstm_mode=lstm_mode)
    keys, shapes = encoder_shapes(F, nb)
    ctx.load_state_dict(seeded_state_dict(keys, shapes, seed=SEED))
    return ctx


def _expected(F, n_list, T, env, **device):
    """Summed stage launches of encoder passes over the batches n_list (plan() per pass; conv: two launches per pass)."""
    cu = _cu_count()
    out = dict.fromkeys(COUNTED, 0)
    for n in n_list:
        p = sp.plan(F, n, T, cu, env, **device)
        out["conv"] += 2
        for k in ("lstm_in", "lstm_rec", "linear"):
            out[k] += p[k]
    return out


def _check_plan(got, F, n_list, T, env, label):
    """The launch counts of the passes must be the ones plan() predicts.  Where they are those of a plan without the
    two-groups-per-workgroup kernel or without signal mode -- what the device or the process can withhold (the occupancy query,
    hipStreamWaitValue32 support, rocprofv3 counter collection) and plan() cannot see -- the row does not reach its branch
    here and is skipped with that reason."""
    if got == _expected(F, n_list, T, env):
        return
    for device, why in (({"dual_ok": False}, "the occupancy query rejects the two-groups-per-workgroup kernel"),
                        ({"signal_ok": False}, "signal mode is unavailable (no hipStreamWaitValue32, or counter collection)"),
                        ({"dual_ok": False, "signal_ok": False}, "neither the two-groups kernel nor signal mode is available")):
        if got == _expected(F, n_list, T, env, **device):
            pytest.skip("%s: %s, so the row cannot take %s" % (why, got, label))
    assert False, ("launch counts are not those of the planned %s" % label, got, _expected(F, n_list, T, env))


def _counts(ctx):
    st = ctx.stage_times()
    return {k: st[k][1] for k in COUNTED}


def _where(got, ref):
    """Where two (T, n, C) score tensors differ: how many values, which time steps and chunks (for the failure message)."""
    import torch
    t, c = torch.nonzero((got != ref).any(dim=2), as_tuple=True)
    if t.numel() == 0:
        return "no value differs"
    steps, chunks = torch.unique(t).tolist(), torch.unique(c).tolist()
    return "%d values, steps %s (%d), chunks %s (%d), max |diff| %.3g" % (
        int((got != ref).sum()), steps[:12], len(steps), chunks[:12], len(chunks), float((got - ref).abs().max()))


def _cu_count():
    import torch
    return torch.cuda.get_device_properties(0).multi_processor_count


def _reference(F, nb, L):
    """The bank of a geometry and its serial-order results: (signal (NB, L), scores (T, NB, C), seq (NB, T), len (NB,))."""
    import torch
    key = _key(F, nb, L)
    if key in _cache:
        return _cache[key]
    with pytest.MonkeyPatch.context() as mp:
        _clear_knobs(mp)
        for name, v in sp.REFERENCE_ENV.items():
            mp.setenv(name, v)
        NB = BANK[key]
        dev = torch.device("cuda", 0)
        gen = torch.Generator(device=dev)
        gen.manual_seed(1000 * nb + L + F)
        sig = torch.randn((NB, L), dtype=torch.float32, device=dev, generator=gen)
        batch = min(NB, 64 * sp.LG_BN)           # the one-launch-per-step order refuses more than 64 groups
        ctx = _context(F, nb, L, batch, lstm_mode=1)
        T, C = ctx.T, ctx.C_noblank
        scores = torch.empty((T, NB, C), dtype=torch.float32, device=dev)
        seq = torch.full((NB, T), -1, dtype=torch.int8, device=dev)
        lens = torch.full((NB,), -1, dtype=torch.int32, device=dev)
        tmp = torch.empty((T * batch * C,), dtype=torch.float32, device=dev)
        ctx.reset_stage_times()
        parts = [(b0, min(NB, b0 + batch)) for b0 in range(0, NB, batch)]
        for b0, b1 in parts:
            n = b1 - b0
            ctx.encode_dev(sig[b0].data_ptr(), n, False, tmp.data_ptr())
            ctx.synchronize()
            scores[:, b0:b1] = tmp[:T * n * C].view(T, n, C)
            torch.cuda.synchronize()                 # (the next part's encode writes tmp on the context's stream)
            ctx.basecall_chunks_dev(sig[b0].data_ptr(), n, ALPHABET[:nb + 1], seq[b0].data_ptr(), lens[b0].data_ptr())
        ctx.synchronize()
        got = _counts(ctx)
        ctx.close()
        del tmp
        want = _expected(F, [b1 - b0 for b0, b1 in parts] * 2, T, sp.REFERENCE_ENV)
        assert got == want, ("the reference did not run one launch per step", got, want)
        assert int(lens.min()) >= 0
    _cache[key] = (sig, scores, seq, lens)
    return _cache[key]


@pytest.fixture(scope="module", autouse=True)
def _free_references():
    yield
    _cache.clear()


@pytest.mark.parametrize("row", sp.ROWS, ids=[r[0] for r in sp.ROWS])
def test_schedule_matches_serial_order(row, monkeypatch):
    import torch
    name, F, nb, L, N, env, label, anchors = row
    T = sp.chunk_T(L)
    p = sp.plan(F, N, T, _cu_count(), env)
    if p["label"] != label:
        pytest.skip("on %d CUs this row plans %s, not %s" % (_cu_count(), p["label"], label))
    sig, ref_scores, ref_seq, ref_len = _reference(F, nb, L)
    _clear_knobs(monkeypatch)
    for k, v in env.items():
        monkeypatch.setenv(k, v)                # XB_LSTM_SPREAD is read per layer: it stays set while the row runs
    ctx = _context(F, nb, L, N)
    assert ctx.T == T
    dev = sig.device
    a, b = sig[0].data_ptr(), sig[1].data_ptr()     # A = bank[0:N], B = bank[1:N + 1]

    # ---- scores of A and B, back to back
    sA = torch.empty((T, N, ctx.C_noblank), dtype=torch.float32, device=dev)
    sB = torch.empty_like(sA)
    ctx.reset_stage_times()
    ctx.encode_dev(a, N, False, sA.data_ptr())
    ctx.encode_dev(b, N, False, sB.data_ptr())
    ctx.synchronize()
    got = _counts(ctx)
    _check_plan(got, F, [N, N], T, env, p["label"])
    assert torch.equal(sA, ref_scores[:, 0:N]), "scores of A differ from the serial order: " + _where(sA, ref_scores[:, 0:N])
    assert torch.equal(sB, ref_scores[:, 1:N + 1]), "scores of B differ from the serial order: " + _where(sB, ref_scores[:, 1:N + 1])
    picks = list(anchors)
    sc = sA[:, picks].cpu().numpy() if picks else None
    del sA, sB

    # ---- fused basecall of A and B, back to back
    seqs = [torch.full((N, T), -1, dtype=torch.int8, device=dev) for _ in range(2)]
    lens = [torch.full((N,), -1, dtype=torch.int32, device=dev) for _ in range(2)]
    torch.cuda.synchronize()                    # the fills run on torch's stream, the calls on the context's streams
    ctx.reset_stage_times()
    for ptr, s, ln in zip((a, b), seqs, lens):
        ctx.basecall_chunks_dev(ptr, N, ALPHABET[:nb + 1], s.data_ptr(), ln.data_ptr())
    ctx.synchronize()
    got = _counts(ctx)
    ctx.close()
    _check_plan(got, F, [N, N], T, env, p["label"])
    print("\n%s: %s, launches per pass %s" % (name, p["label"], {k: v // 2 for k, v in got.items()}))
    for i, (s, ln) in enumerate(zip(seqs, lens)):
        assert torch.equal(ln, ref_len[i:i + N]), "called lengths of %s differ" % "AB"[i]
        assert torch.equal(s, ref_seq[i:i + N]), "sequences of %s differ" % "AB"[i]

    # ---- oracle on the seam chunks: its fp32 encoder within the mixed bound, its decode of the GPU's scores exactly
    if picks:
        ref = oracle.encode(sig[picks].cpu().numpy(), seeded_state_dict(*encoder_shapes(F, nb), seed=SEED), F, nb, SL,
                            expand_blanks=False)
        err = float(np.abs(ref - sc).max())
        assert err < 2e-4, err
        lab = oracle.decode(sc, nb, SL, blank_score=2.0)["labels"]
        oseq, _, olen = oracle.pack(lab, ALPHABET[:nb + 1])
        assert np.array_equal(olen, lens[0][picks].cpu().numpy())
        assert np.array_equal(oseq, seqs[0][picks].cpu().numpy())


@pytest.mark.parametrize("row", sp.PAIR_ROWS, ids=[r[0] for r in sp.PAIR_ROWS])
def test_paired_calls_match_unpaired(row, monkeypatch):
    """Calls co-scheduled two at a time (xb_reserve_pairing) give each call what the call alone gives in the serial order."""
    import torch
    name, F, nb, L, max_batch, calls, labels = row
    T = sp.chunk_T(L)
    passes = sp.pair_passes(calls)
    planned = tuple(sp.plan(F, n, T, _cu_count())["label"] for n in passes)
    if planned != labels:
        pytest.skip("on %d CUs the passes plan %s, not %s" % (_cu_count(), planned, labels))
    sig, _, ref_seq, ref_len = _reference(F, nb, L)
    _clear_knobs(monkeypatch)
    ctx = _context(F, nb, L, max_batch)
    assert ctx.reserve_pairing(), "this context does not pair calls"
    dev = sig.device
    offs = np.concatenate([[0], np.cumsum(calls)[:-1]]).tolist()
    seqs = [torch.full((n, T), -1, dtype=torch.int8, device=dev) for n in calls]
    lens = [torch.full((n,), -1, dtype=torch.int32, device=dev) for n in calls]
    torch.cuda.synchronize()                    # the fills run on torch's stream, the calls on the context's streams
    ctx.reset_stage_times()
    for o, n, s, ln in zip(offs, calls, seqs, lens):
        ctx.basecall_chunks_dev(sig[o].data_ptr(), n, ALPHABET[:nb + 1], s.data_ptr(), ln.data_ptr())
    ctx.synchronize()
    got = _counts(ctx)
    ctx.close()
    _check_plan(got, F, passes, T, {}, planned)
    print("\n%s: passes %s %s, launches %s" % (name, passes, planned, got))
    for j, (o, n, s, ln) in enumerate(zip(offs, calls, seqs, lens)):
        assert torch.equal(ln, ref_len[o:o + n]), "called lengths of call %d differ" % j
        assert torch.equal(s, ref_seq[o:o + n]), "sequences of call %d differ" % j
