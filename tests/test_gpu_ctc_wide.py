"""GPU: the CTC lattice kernels at every width up to 2048 positions (the table is tests/ctc_wide_cases.py; its CPU tier,
tests/test_ctc_wide_host.py, says what the reference is worth there).

ctc_scan_kernel (xb_ctc_logz, xb_ctc_alignments) and ctc_loss_kernel (xb_ctc_loss, xb_validate_chunks), both in xb_ctc.hip on
one pair of sweeps, put position l on thread l % threads, slot l // threads, up to 8 slots.  Every slot holds a live position
somewhere in the table, both sides of 64 / 65, 128 / 129, 256 / 257, 512 / 513 and 1024 / 1025 occur, and 2048 is the limit;
the PMAX 1, 2, 4 and 8 instantiations of both run by the rule ctc_loss_threads, ctc_loss_kernel's in both score layouts and
under XB_CTC_LOSS_THREADS too.  The contract is bit-equality: with
oracle.ctc_logz for the scans, with the host composition (xb_crf_logz, `scores - logz / T`, oracle.ctc_logz, `-(logz / length)`)
for the loss, and, without any oracle, with the float32 running sum of a single path's scores and with Log.zero for a row that
has no path."""
import numpy as np
import pytest
import torch

import oracle
import ctc_wide_cases as W
from conftest import encoder_shapes, seeded_state_dict
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu

NB, SL = 4, 3                                   # the main table's geometry


def _context(nb, sl, T, N):
    ctx = _lib.Context(0, nb, sl, 32, 19, 5, 5.0, W.BLANK, T * 5, N)
    assert ctx.T == T
    return ctx


def _same(what, got, ref, lens, sl, np_):
    """Bit-equality of a per-chunk vector (N,) or a per-cell array (T, N, positions); the message names the chunk, the first
    differing position and its slot in the launch a row of np_ positions gets by the rule."""
    assert got.shape == ref.shape and got.dtype == ref.dtype, (what, got.shape, ref.shape)
    if np.array_equal(got, ref):
        return
    threads = W.loss_launch(np_)[0]
    if got.ndim == 1:
        b = int(np.flatnonzero(got != ref)[0])
        l = int(lens[b]) - sl
        pytest.fail("%s: chunk %d (end position %d, slot %d): %r, reference %r" % (what, b, l, l // threads, got[b], ref[b]))
    bad = np.argwhere(got != ref)
    b = int(bad[:, 1].min())
    l = int(bad[bad[:, 1] == b][:, 2].min())
    t = int(bad[(bad[:, 1] == b) & (bad[:, 2] == l)][:, 0].min())
    pytest.fail("%s: chunk %d, first differing position %d (slot %d), first at step %d: %r, reference %r; %d cells differ, in slots %s"
                % (what, b, l, l // threads, t, got[t, b, l], ref[t, b, l], len(bad), sorted(set((bad[:, 2] // threads).tolist()))))


def _main_case(np_):
    return [c for c in W.LOSS_CASES if c.np == np_ and (c.nb, c.sl) == (NB, SL)][0]


# ---- ctc_scan_kernel --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("c", W.SCAN_CASES, ids=W.case_id)
def test_scans_are_the_oracles_bit_for_bit(c):
    sc, targets, lens = W.build(c)
    ctx = _context(c.nb, c.sl, c.T, 3)
    ref = oracle.ctc_logz(sc, targets, lens, c.nb, c.sl, want_grads=True)
    got = ctx.ctc_logz(sc, targets, lens, want_grads=True)
    _same("logz", got["logz"], ref["logz"], lens, c.sl, c.np)
    _same("stay", got["stay"], ref["stay"], lens, c.sl, c.np)
    _same("move", got["move"], ref["move"], lens, c.sl, c.np)
    del got
    _same("logz of the forward sweep alone", ctx.ctc_logz(sc, targets, lens)["logz"], ref["logz"], lens, c.sl, c.np)
    del ref
    refm = oracle.ctc_logz(sc, targets, lens, c.nb, c.sl, semiring="max", want_grads=True)
    al, best = ctx.ctc_alignments(sc, targets, lens)
    _same("best score", best, refm["logz"], lens, c.sl, c.np)
    _same("alignment", al, refm["stay"], lens, c.sl, c.np)
    ctx.close()


@pytest.mark.parametrize("np_", W.PROPERTY_POSITIONS)
def test_scan_of_a_single_path_and_of_no_path(np_):
    """Independent of the oracle.  T = np - 1: every step moves, logz is the float32 running sum of the diagonal's move scores in
    time order (the other branch of sum2 is Log.zero, and log(1 + 0) = 0), the Max semiring gives the same bits and the alignment
    is the diagonal.  T = np - 2: no path, logz is Log.zero exactly, and the neighbour one label shorter is a single path."""
    sc, targets, lens = W.build_single_path(np_)
    ctx = _context(NB, SL, np_ - 1, 2)
    want = np.array([W.diagonal_sum(sc, targets, 0, NB, SL, np_ - 1), W.stay_sum(sc, targets, 1, NB, SL)], np.float32)
    _same("single path, logz", ctx.ctc_logz(sc, targets, lens)["logz"], want, lens, SL, np_)
    _same("single path, logz beside the gradients", ctx.ctc_logz(sc, targets, lens, want_grads=True)["logz"], want, lens, SL, np_)
    al, best = ctx.ctc_alignments(sc, targets, lens)
    _same("single path, best score", best, want, lens, SL, np_)
    diagonal = np.zeros((np_ - 1, 2, np_), np.float32)
    diagonal[np.arange(np_ - 1), 0, np.arange(np_ - 1)] = 1.0
    diagonal[:, 1, 0] = 1.0
    _same("single path, alignment", al, diagonal, lens, SL, np_)

    sc, targets, lens = W.build_infeasible(np_)
    want = np.array([W.ZERO, W.diagonal_sum(sc, targets, 1, NB, SL, np_ - 2)], np.float32)
    assert want[1] > -1e30
    _same("no path, logz", ctx.ctc_logz(sc, targets, lens)["logz"], want, lens, SL, np_)
    al, best = ctx.ctc_alignments(sc, targets, lens)
    _same("no path, best score", best, want, lens, SL, np_)
    _same("no path, the neighbour's alignment", al[:, 1:, :], diagonal[:np_ - 2, :1, :], lens[1:], SL, np_)
    ctx.close()


# ---- ctc_loss_kernel --------------------------------------------------------------------------------------------------------------
def _loss_both_layouts(c):
    """[(has_blank, scores, targets uint8, lens)] of a table case."""
    out = []
    for hb in (True, False):
        sc, targets, lens = W.build(c, with_blank=hb)
        out.append((hb, sc, targets.astype(np.uint8), lens))
    return out


@pytest.mark.parametrize("c", W.LOSS_CASES, ids=W.case_id)
def test_loss_is_the_host_composition_bit_for_bit(c):
    ctx = _context(c.nb, c.sl, c.T, 3)
    for hb, sc, targets, lens in _loss_both_layouts(c):
        what = "with blank" if hb else "blank-less"
        ref, ref_logz = W.loss_reference(ctx, sc, targets, lens, c.nb, c.sl, hb)
        assert np.all(ref_logz > -1e30)
        loss, logz = ctx.ctc_loss(sc, targets, lens, has_blank=hb, want_logz=True)
        print("%s <%d threads, PMAX %d>: max |loss - ref| = %g" % ((what,) + W.loss_launch(c.np) + (np.abs(loss - ref).max(),)))
        _same(what + ", logz", logz, ref_logz, lens, c.sl, c.np)
        _same(what + ", loss", loss, ref, lens, c.sl, c.np)
        # the one-position chunk without the oracle: the running sum of its stay scores, blank-less T additions of `blank - c`
        x, cn = W.normalised(ctx, sc, c.nb, hb)
        assert logz[2] == W.stay_sum(x, targets, 2, c.nb, c.sl)
        if not hb:
            assert logz[2] == W.running_sum(np.full(c.T, np.float32(W.BLANK) - cn[2], np.float32))
    ctx.close()


# (np, XB_CTC_LOSS_THREADS, threads and PMAX of the launch it must give): six accepted overrides, two ignored ones (64 * 8 < 513; 100
# is no allowed workgroup size), which leave the rule's 256 threads
OVERRIDES = [(129, 64, 64, 4), (257, 64, 64, 8), (257, 128, 128, 4), (512, 64, 64, 8), (1024, 128, 128, 8), (1025, 256, 256, 8),
             (513, 64, 256, 4), (257, 100, 256, 2)]


@pytest.mark.parametrize("np_,value,threads,pmax", OVERRIDES, ids=["np%d-%d" % o[:2] for o in OVERRIDES])
def test_loss_threads_override_returns_the_same_bits(monkeypatch, np_, value, threads, pmax):
    assert [o[:2] for o in OVERRIDES] == W.THREAD_OVERRIDES
    assert W.loss_launch(np_, value) == (threads, pmax)
    c = _main_case(np_)
    ctx = _context(c.nb, c.sl, c.T, 3)
    for hb, sc, targets, lens in _loss_both_layouts(c):
        monkeypatch.delenv("XB_CTC_LOSS_THREADS", raising=False)
        loss0, logz0 = ctx.ctc_loss(sc, targets, lens, has_blank=hb, want_logz=True)
        assert np.all(logz0 > -1e30)
        monkeypatch.setenv("XB_CTC_LOSS_THREADS", str(value))        # the library reads it on every call
        loss1, logz1 = ctx.ctc_loss(sc, targets, lens, has_blank=hb, want_logz=True)
        what = "%s, %d threads" % ("with blank" if hb else "blank-less", value)
        _same(what + ", logz", logz1, logz0, lens, c.sl, c.np)
        _same(what + ", loss", loss1, loss0, lens, c.sl, c.np)
    ctx.close()


@pytest.mark.parametrize("np_", W.PROPERTY_POSITIONS)
def test_loss_of_a_single_path_and_of_no_path(np_):
    """Independent of the oracle: logz is the float32 running sum of `row[cm] - c` on the diagonal, c = logz_crf / T as the kernel
    computes it; a row without a path gives Log.zero and the loss -(Log.zero / length), its neighbour is unaffected."""
    ctx = _context(NB, SL, np_ - 1, 2)
    for hb in (True, False):
        what = "with blank" if hb else "blank-less"
        sc, targets, lens = W.build_single_path(np_, with_blank=hb)
        x, cn = W.normalised(ctx, sc, NB, hb)
        want = np.array([W.diagonal_sum(x, targets, 0, NB, SL, np_ - 1), W.stay_sum(x, targets, 1, NB, SL)], np.float32)
        if not hb:
            assert want[1] == W.running_sum(np.full(np_ - 1, np.float32(W.BLANK) - cn[1], np.float32))
        loss, logz = ctx.ctc_loss(sc, targets.astype(np.uint8), lens, has_blank=hb, want_logz=True)
        _same(what + ", single path, logz", logz, want, lens, SL, np_)
        _same(what + ", single path, loss", loss, -(want / lens.astype(np.float32)), lens, SL, np_)

        sc, targets, lens = W.build_infeasible(np_, with_blank=hb)
        x, cn = W.normalised(ctx, sc, NB, hb)
        want = np.array([W.ZERO, W.diagonal_sum(x, targets, 1, NB, SL, np_ - 2)], np.float32)
        assert want[1] > -1e30
        loss, logz = ctx.ctc_loss(sc, targets.astype(np.uint8), lens, has_blank=hb, want_logz=True)
        _same(what + ", no path, logz", logz, want, lens, SL, np_)
        _same(what + ", no path, loss", loss, -(want / lens.astype(np.float32)), lens, SL, np_)
        assert loss[0] == -(W.ZERO / np.float32(np_ + SL - 1))
    ctx.close()


def test_device_form_at_2048_positions_validates_on_the_device():
    """xb_ctc_loss_dev on a 2050-wide row (tests/test_gpu_valloss.py::test_device_form_validates_on_the_device at the limit): the
    kernel's own label check strides over the row, so a bad label at an index a thread reaches in its fifth round and later must
    still be seen, and one beyond the chunk's length must not."""
    c = _main_case(2048)
    N, Lt, np_ = 3, c.np + SL - 1, c.np
    assert Lt == 2050
    ctx = _context(NB, SL, c.T, N)
    nbl, targets, lens = W.build(c, with_blank=False)
    targets = targets.astype(np.uint8)
    ref, ref_logz = W.loss_reference(ctx, nbl, targets, lens, NB, SL, False)
    dev = torch.device("cuda", 0)
    d_sc = torch.from_numpy(nbl).to(dev)
    d_t, d_l = torch.from_numpy(targets).to(dev), torch.from_numpy(lens).to(dev)
    d_loss = torch.full((N,), -7.0, dtype=torch.float32, device=dev)
    d_logz = torch.zeros((N,), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def run(t, l):
        ctx.ctc_loss_dev(d_sc.data_ptr(), c.T, N, False, t.data_ptr(), Lt, l.data_ptr(), d_loss.data_ptr(), d_logz.data_ptr())
        ctx.synchronize()

    def correct_call_matches():
        run(d_t, d_l)
        _same("device form, logz", d_logz.cpu().numpy(), ref_logz, lens, SL, np_)
        _same("device form, loss", d_loss.cpu().numpy(), ref, lens, SL, np_)

    correct_call_matches()
    assert lens[1] < 1500 < lens[0]
    beyond = targets.copy()
    beyond[1, 1500] = beyond[1, Lt - 1] = beyond[2, 1024] = NB + 1          # beyond these chunks' lengths: not read
    run(torch.from_numpy(beyond).to(dev), d_l)
    _same("labels beyond the length, loss", d_loss.cpu().numpy(), ref, lens, SL, np_)

    def with_label(i):
        t = targets.copy()
        t[0, i] = NB + 1
        return t

    def with_length(v):
        l = lens.copy()
        l[1] = v
        return l

    for t, l, row in ((with_label(1024), lens, 0), (with_label(1500), lens, 0), (with_label(Lt - 1), lens, 0),
                      (targets, with_length(Lt + 1), 1), (targets, with_length(SL - 1), 1)):
        d_loss.fill_(-7.0)
        torch.cuda.synchronize()
        with pytest.raises(_lib.XbError) as e:
            run(torch.from_numpy(t).to(dev), torch.from_numpy(l).to(dev))
        assert e.value.code == _lib.XB_ERR_INVALID
        got = d_loss.cpu().numpy()
        assert got[row] == -7.0                              # no loss written for the offending chunk
        keep = np.arange(N) != row
        assert np.array_equal(got[keep], ref[keep])
        correct_call_matches()                               # the context works afterwards
    ctx.close()


def test_validate_chunks_with_a_2050_wide_row():
    """xb_validate_chunks where the label row is as wide as the API takes it: the loss is xb_ctc_loss of the encoder's own
    blank-less scores, the calls are xb_basecall_chunks' (what tests/test_gpu_valloss.py asserts at 12 labels)."""
    F, L, N, Lt, np_ = 32, 10250, 2, 2050, 2048
    alphabet = "NACGT"
    ctx = _lib.Context(0, NB, SL, F, 19, 5, 5.0, W.BLANK, L, N)
    assert ctx.T == Lt
    keys, shapes = encoder_shapes(F, NB)
    ctx.load_state_dict(seeded_state_dict(keys, shapes, 3))
    rng = np.random.default_rng(2050)
    x = rng.standard_normal((N, L)).astype(np.float32)
    targets, lens = W.label_rows(rng, N, Lt, NB, SL, lens=[Lt, 1025 + SL - 1], dtype=np.uint8)
    want_seq, want_lens = ctx.basecall_chunks(x, alphabet)
    want, want_logz = ctx.ctc_loss(ctx.encode(x, expand_blanks=False), targets, lens, has_blank=False, want_logz=True)
    assert np.all(want_logz > -1e30)                         # T = 2050 steps reach position 2047
    seq, slen, loss = ctx.validate_chunks(x, alphabet, targets, lens)
    assert np.array_equal(seq, want_seq) and np.array_equal(slen, want_lens)
    _same("loss", loss, want, lens, SL, np_)
    ctx.close()
