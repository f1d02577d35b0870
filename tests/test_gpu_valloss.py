"""GPU: the validation loss from device-resident scores (xb_ctc_loss, xb_validate_chunks, `evaluate --loss`).

The kernel reads RAW scores in either layout, derives the gather columns from uint8 labels and normalises as it fetches;
the contract is bit-equality with the composition the parent commit ran on the host: xb_crf_logz, `scores - logz / T` in
float32, oracle.ctc_logz on the result, `-(logz / length)`.  Shapes are tests/test_ctc.py's GPU_CASES (T not a multiple of
the prefetch depth, more than 256 positions, a single position, length = Lt, every state length and base count) plus T = 3 on
a larger context and a batch of one."""
import functools

import numpy as np
import pytest
import torch

import oracle
from conftest import encoder_shapes, make_config, random_scores, seeded_state_dict
from ctc_wide_cases import BLANK, ctc_logz_f64 as _ctc_logz_f64, label_rows, loss_reference as _reference
from test_ctc import GPU_CASES
from xna_basecaller_amd import _lib

pytestmark = pytest.mark.gpu

# (nb, T, N, Lt, sl, T of the context): the shapes above on a context of their own T, then the two added cases
CASES = [c + (c[1],) for c in GPU_CASES] + [(5, 3, 3, 9, 3, 64), (6, 50, 1, 20, 3, 50)]
IDS = ["%d-%d-%d-%d-sl%d-ctx%d" % c for c in CASES]
_targets = functools.partial(label_rows, dtype=np.uint8)        # the ragged label rows as references.npy holds them


def _case(nb, T, N, Lt, sl):
    rng = np.random.default_rng(Lt + nb)
    targets, lens = _targets(rng, N, Lt, nb, sl, lens=None if sl == 3 else [Lt, sl + 1, sl])
    return targets, lens


@pytest.mark.parametrize("nb,T,N,Lt,sl,Tctx", CASES, ids=IDS)
def test_loss_of_given_scores_is_the_host_composition_bit_for_bit(nb, T, N, Lt, sl, Tctx):
    targets, lens = _case(nb, T, N, Lt, sl)
    ctx = _lib.Context(0, nb, sl, 32, 19, 5, 5.0, BLANK, Tctx * 5, N)
    assert ctx.T == Tctx
    sc = random_scores(T, N, nb, sl=sl, seed=T)
    ref, ref_logz = _reference(ctx, sc, targets, lens, nb, sl, True)
    loss, logz = ctx.ctc_loss(sc, targets, lens, has_blank=True, want_logz=True)
    print("with blank: max |loss - ref| = %g" % np.abs(loss - ref).max())
    assert np.array_equal(logz, ref_logz)
    assert np.array_equal(loss, ref)
    assert np.array_equal(ctx.ctc_loss(sc, targets, lens, has_blank=True), ref)          # without the optional output
    nbl = random_scores(T, N, nb, sl=sl, seed=T + 1, with_blank=False)
    ref0, ref0_logz = _reference(ctx, nbl, targets, lens, nb, sl, False)
    loss0, logz0 = ctx.ctc_loss(nbl, targets, lens, has_blank=False, want_logz=True)
    print("blank-less: max |loss - ref| = %g" % np.abs(loss0 - ref0).max())
    assert np.array_equal(logz0, ref0_logz)
    assert np.array_equal(loss0, ref0)
    ctx.close()


@pytest.mark.parametrize("labels", ["NACGT", "NACGTXY"])
def test_loss_against_float64(labels):
    """The whole expression -logZ_ctc(scores - logZ_crf(scores) / T) / length in float64 (CRF logZ by the dense recursion over
    the idx table, then the lattice), at tests/test_ctc.py::test_gpu_model_ctc_loss_and_gradient's shape and within its 2e-4 --
    here per chunk, which bounds the mean that test compares."""
    from xna_basecaller_amd.crf.model import CTC_CRF
    nb, sl, T, N, Lt = len(labels) - 1, 3, 30, 3, 10
    rng = np.random.default_rng(7)
    sc = random_scores(T, N, nb, seed=11)
    targets, lens = _targets(rng, N, Lt, nb, sl)
    ctx = _lib.Context(0, nb, sl, 32, 19, 5, 5.0, BLANK, T * 5, N)
    loss = ctx.ctc_loss(sc, targets, lens)
    idx = CTC_CRF(sl, list(labels)).idx.numpy().astype(np.int64)
    S, E = nb ** sl, nb + 1
    x = torch.tensor(sc, dtype=torch.float64)
    a = torch.zeros((N, S), dtype=torch.float64)
    for t in range(T):
        a = torch.logsumexp(x[t].reshape(N, S, E) + a[:, torch.as_tensor(idx)], dim=2)
    xn = x - (torch.logsumexp(a, dim=1) / T)[None, :, None]
    stay_idx, move_idx = oracle.ctc_indices(targets.astype(np.int32), nb, sl)
    ref = -(_ctc_logz_f64(xn, stay_idx, move_idx, lens + 1 - sl) / torch.as_tensor(lens, dtype=torch.float64)).numpy()
    print("max |loss - float64| = %g" % np.abs(loss - ref).max())
    assert np.abs(loss - ref).max() < 2e-4
    assert abs(float(loss.mean(dtype=np.float64)) - float(ref.mean())) < 2e-4
    ctx.close()


def test_bad_lengths_and_labels_are_refused_and_the_context_carries_on():
    nb, T, N, Lt, sl = 5, 40, 4, 14, 3
    rng = np.random.default_rng(1)
    targets, lens = _targets(rng, N, Lt, nb, sl)
    ctx = _lib.Context(0, nb, sl, 32, 19, 5, 5.0, BLANK, T * 5, N)
    sc = random_scores(T, N, nb, seed=2)
    ref, _ = _reference(ctx, sc, targets, lens, nb, sl, True)

    def still_works():
        assert np.array_equal(ctx.ctc_loss(sc, targets, lens), ref)

    still_works()
    for bad_len in (sl - 1, Lt + 1):
        bad = lens.copy()
        bad[2] = bad_len
        with pytest.raises(_lib.XbError) as e:
            ctx.ctc_loss(sc, targets, bad)
        assert e.value.code == _lib.XB_ERR_INVALID and "target_lengths[2]" in str(e.value)
        still_works()
    bad_t = targets.copy()
    bad_t[0, lens[0] - 1] = nb + 1                           # the last label inside the row's length
    with pytest.raises(_lib.XbError) as e:
        ctx.ctc_loss(sc, bad_t, lens)
    assert e.value.code == _lib.XB_ERR_INVALID and "targets[0]" in str(e.value)
    still_works()
    beyond = targets.copy()
    beyond[1, lens[1]:] = nb + 1                             # (padding beyond a row's length is not read)
    if lens[1] < Lt:
        assert np.array_equal(ctx.ctc_loss(sc, beyond, lens), ref)
    wide = np.ones((N, 2048 + sl), np.uint8)                 # 2049 positions
    with pytest.raises(_lib.XbError) as e:
        ctx.ctc_loss(sc, wide, lens)
    assert e.value.code == _lib.XB_ERR_INVALID and "2049 positions" in str(e.value)
    still_works()
    ctx.close()


def test_every_host_form_refuses_a_bad_label_batch_alike_and_carries_on():
    """The five host forms that take label rows -- xb_ctc_loss, xb_ctc_loss_grad, xb_validate_chunks, xb_head_train_step and
    xb_top_train_step -- hold one contract on them: a width one short of a single position, a length one above the width and a
    label above n_base are each refused with XB_ERR_INVALID and one text behind the entry point's own name, and the good
    batch right after each refusal gives the bytes of the same calls on a context that never saw a bad one.  One context, the
    first four under an open head trainer, the last under a top trainer of one layer."""
    from xna_basecaller_amd.crf.trainer import B_KEY, W_KEY, top_keys
    nb, sl, F, L, B, Lt = 6, 3, 32, 200, 2, 12
    keys, shapes = encoder_shapes(F, nb)
    sd = seeded_state_dict(keys, shapes, seed=5)
    rng = np.random.default_rng(17)
    x = rng.standard_normal((B, L)).astype(np.float32)
    sc = random_scores(L // 5, B, nb, sl=sl, seed=4, with_blank=False)
    targets, lens = _targets(rng, B, Lt, nb, sl)
    long_l, high_t = lens.copy(), targets.copy()
    long_l[1] = Lt + 1
    high_t[0, 0] = nb + 1
    bad = [(np.ones((B, sl - 1), np.uint8), lens, "target width %d gives 0 positions" % (sl - 1)),
           (targets, long_l, "target_lengths[1] = %d" % (Lt + 1)),
           (high_t, lens, "targets[0][0] = %d" % (nb + 1))]
    calls = {
        "xb_ctc_loss": lambda c, t, l: (c.ctc_loss(sc, t, l, has_blank=False),),
        "xb_ctc_loss_grad": lambda c, t, l: c.ctc_loss_grad(sc, t, l, has_blank=False),
        "xb_validate_chunks": lambda c, t, l: c.validate_chunks(x, "NACGTXY", t, l),
        "xb_head_train_step": lambda c, t, l: c.head_train_step(x, t, l, 2e-3) + c.head_get_weights() + c.head_image(),
        "xb_top_train_step": lambda c, t, l: c.top_train_step(x, t, l, 2e-3) + (c.top_get_weights(),),
    }
    texts = [set() for _ in bad]

    def walk(with_bad):
        ctx = _lib.Context(0, nb, sl, F, 19, 5, 5.0, BLANK, L, B, precision=_lib.XB_PREC_MIXED)
        assert ctx.T == 40
        ctx.load_state_dict(sd)
        out = []

        def go(name):
            for k, (t, l, what) in enumerate(bad):
                if with_bad:
                    with pytest.raises(_lib.XbError) as e:
                        calls[name](ctx, t, l)
                    front, _, text = str(e.value).partition(name + ": ")
                    assert e.value.code == _lib.XB_ERR_INVALID and front == "libxnacall error %d: " % _lib.XB_ERR_INVALID, (name, str(e.value))
                    assert text.startswith(what), (name, text)
                    texts[k].add(text)
                out.append((name, k, [np.array(a) for a in calls[name](ctx, targets, lens)]))

        ctx.head_train_begin(sd[W_KEY], sd[B_KEY])
        for name in list(calls)[:4]:
            go(name)
        ctx.head_train_end()
        ctx.top_train_begin(1, np.concatenate([sd[k].ravel() for k in top_keys(1)]))
        go("xb_top_train_step")
        ctx.top_train_end()
        ctx.close()
        return out

    got, want = walk(True), walk(False)
    assert [len(t) for t in texts] == [1, 1, 1], texts          # five entry points, one text each
    assert len(got) == len(want) == 15
    for (name, k, a), (_, _, b) in zip(got, want):
        assert len(a) == len(b) and all(p.dtype == q.dtype and p.tobytes() == q.tobytes() for p, q in zip(a, b)), (name, k)


def test_device_form_validates_on_the_device():
    """xb_ctc_loss_dev has nothing on the host to check: the kernel flags a bad length or label in the context's error word,
    writes no loss for that chunk, and the next xb_synchronize reports XB_ERR_INVALID; the context works afterwards."""
    nb, T, N, Lt, sl = 6, 33, 4, 20, 3
    rng = np.random.default_rng(5)
    targets, lens = _targets(rng, N, Lt, nb, sl)
    ctx = _lib.Context(0, nb, sl, 32, 19, 5, 5.0, BLANK, T * 5, N)
    nbl = random_scores(T, N, nb, seed=3, with_blank=False)
    ref, ref_logz = _reference(ctx, nbl, targets, lens, nb, sl, False)
    dev = torch.device("cuda", 0)
    d_sc = torch.from_numpy(nbl).to(dev)
    d_t, d_l = torch.from_numpy(targets).to(dev), torch.from_numpy(lens).to(dev)
    d_loss = torch.full((N,), -7.0, dtype=torch.float32, device=dev)
    d_logz = torch.zeros((N,), dtype=torch.float32, device=dev)
    torch.cuda.synchronize()

    def run(t, l):
        ctx.ctc_loss_dev(d_sc.data_ptr(), T, N, False, t.data_ptr(), Lt, l.data_ptr(), d_loss.data_ptr(), d_logz.data_ptr())
        ctx.synchronize()

    run(d_t, d_l)
    assert np.array_equal(d_loss.cpu().numpy(), ref) and np.array_equal(d_logz.cpu().numpy(), ref_logz)
    bad_t = targets.copy()
    bad_t[1, 0] = nb + 1
    bad_l = lens.copy()
    bad_l[2] = Lt + 1
    for t, l, row in ((bad_t, lens, 1), (targets, bad_l, 2), (targets, np.where(np.arange(N) == 3, sl - 1, lens).astype(np.int32), 3)):
        d_loss.fill_(-7.0)
        torch.cuda.synchronize()
        with pytest.raises(_lib.XbError) as e:
            run(torch.from_numpy(t).to(dev), torch.from_numpy(l).to(dev))
        assert e.value.code == _lib.XB_ERR_INVALID
        got = d_loss.cpu().numpy()
        assert got[row] == -7.0                              # no loss written for the offending chunk
        keep = np.arange(N) != row
        assert np.array_equal(got[keep], ref[keep])
        run(d_t, d_l)                                        # the context works afterwards
        assert np.array_equal(d_loss.cpu().numpy(), ref)
    ctx.close()


def _model(labels, features=32, batch=8, seed=3):
    from xna_basecaller_amd.crf import Model
    cfg = make_config(features, labels)
    cfg["basecaller"]["batchsize"] = batch
    model = Model(cfg)
    keys, shapes = encoder_shapes(features, len(labels) - 1)
    sd = seeded_state_dict(keys, shapes, seed)
    model.load_state_dict({k: torch.from_numpy(v) for k, v in sd.items()})
    return model.eval().to("cuda")


@pytest.mark.parametrize("labels", ["NACGT", "NACGTXY"])
def test_validate_chunks_is_basecall_plus_the_loss_of_the_same_scores(labels):
    nb, sl, L, Lt, B = len(labels) - 1, 3, 200, 12, 8
    model = _model(labels, batch=B)
    ctx = model.context(L, B)
    assert ctx.max_batch == B and ctx.T == 40
    rng = np.random.default_rng(len(labels))

    def check(N, before=None):
        x = rng.standard_normal((N, L)).astype(np.float32)
        targets, lens = _targets(rng, N, Lt, nb, sl)
        want_seq, want_lens = model.basecall_chunks(x[:, None, :])
        ref, _ = _reference(ctx, ctx.encode(x, expand_blanks=False), targets, lens, nb, sl, False)
        host = model.seqdist.ctc_loss(ctx.encode(x, expand_blanks=True), targets.astype(np.int32), lens, reduction="none")
        pending = before() if before else None
        seq, slen, loss = model.validate_chunks(x[:, None, :], targets, lens)
        print("N = %d: max |loss - composition| = %g, |loss - host route| = %g" % (N, np.abs(loss - ref).max(), np.abs(loss - host).max()))
        assert np.array_equal(seq, want_seq) and np.array_equal(slen, want_lens)
        assert np.array_equal(loss, ref)
        assert np.array_equal(loss, host)
        return pending

    check(5)
    check(B)                                                  # the context's max_batch
    # directly after a submission that has not been collected: the call joins it, and both results are what they are alone
    other = rng.standard_normal((3, L)).astype(np.float32)
    other_seq, other_lens = ctx.basecall_chunks(other, model.alphabet)
    check(5, before=lambda: ctx.submit_chunks(0, other.copy(), model.alphabet))
    got_seq, got_lens = ctx.collect_chunks(0, 3)
    assert np.array_equal(got_seq, other_seq) and np.array_equal(got_lens, other_lens)
    # ... and where the context holds an asynchronous call back for a partner: the held call runs on its own first
    if ctx.reserve_pairing():
        check(5, before=lambda: ctx.submit_chunks(1, other.copy(), model.alphabet))
        got_seq, got_lens = ctx.collect_chunks(1, 3)
        assert np.array_equal(got_seq, other_seq) and np.array_equal(got_lens, other_lens)
    assert model.context(L, B) is ctx


def test_evaluate_loss_weights_all_and_csv(tmp_path, capsys):
    """`evaluate --loss --weights all --csv`: per checkpoint the figure of validate_one_epoch through the old host path (scores
    to the host, model.seqdist.ctc_loss, mean of batch means), the CSV rows in ascending order; without the flags the lines of
    the evaluator as it was."""
    from xna_basecaller_amd import toml_lite, util
    from xna_basecaller_amd.cli import evaluate
    from xna_basecaller_amd.crf import Model
    F, L, N, B = 64, 2000, 30, 16
    labels = list("NACGTXY")
    cfg = make_config(F, labels)
    cfg["basecaller"] = {"batchsize": B, "chunksize": L, "overlap": 100}
    mdir = tmp_path / "model@v1"
    mdir.mkdir()
    (mdir / "config.toml").write_text(toml_lite.dumps(cfg))
    (mdir / "notes.txt").write_text("stray")
    keys, shapes = encoder_shapes(F, 6)
    sds = {w: seeded_state_dict(keys, shapes, seed=w) for w in (10, 2)}
    for w, sd in sds.items():
        torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, str(mdir / ("weights_%d.tar" % w)))
    x = np.random.default_rng(3).standard_normal((N, L)).astype(np.float32)

    def load(w):
        m = Model(cfg)
        m.load_state_dict({k: torch.from_numpy(v) for k, v in sds[w].items()})
        return m.to("cuda")

    model = load(2)
    seq, lens = model.basecall_chunks(x[:, None, :])
    assert min(lens) > 20
    code = {c: i for i, c in enumerate(labels)}
    refs = np.zeros((N, max(lens) + 5), np.int16)
    for i in range(N):
        r = [c for k, c in enumerate(seq[i, :lens[i]].tobytes().decode()) if i % 3 or k % 10 != 3]
        refs[i, :len(r)] = [code[c] for c in r]
    rlens = (refs != 0).sum(1).astype(np.int16)
    data = tmp_path / "ctc" / "validation"
    data.mkdir(parents=True)
    np.save(data / "chunks.npy", x)
    np.save(data / "references.npy", refs)
    np.save(data / "reference_lengths.npy", rlens)

    # what the parent commit could compute: scores to the host, the host route of the loss, the calls, the accuracies
    want = {}
    for w in (2, 10):
        m = load(w)
        means, accs = [], []
        for b0 in range(0, N, B):
            sc = m(x[b0:b0 + B, None, :])
            per = m.seqdist.ctc_loss(sc, refs[b0:b0 + B].astype(np.int32), rlens[b0:b0 + B].astype(np.int32), reduction="none")
            means.append(float(per.mean(dtype=np.float32)))
            s, l = m.basecall_chunks(x[b0:b0 + B, None, :])
            for i in range(len(l)):
                call = s[i, :l[i]].tobytes().decode()
                ref = util.decode_ref(refs[b0 + i], labels)
                accs.append(util.accuracy(ref, call, min_coverage=0.5) if call else 0.)
        want[w] = (float(np.mean(means)), accs)

    out_csv = tmp_path / "out.csv"
    argv = [str(mdir), "--directory", str(tmp_path / "ctc"), "--batchsize", str(B)]
    capsys.readouterr()
    evaluate.main(evaluate.argparser().parse_args(argv + ["--loss", "--weights", "all", "--csv", str(out_csv)]))
    out = capsys.readouterr().out.splitlines()
    assert [l for l in out if l.startswith("* loading model")] == ["* loading model 2", "* loading model 10"]
    assert [l for l in out if l.startswith("* loss")] == ["* loss      %.4f" % want[w][0] for w in (2, 10)]
    assert out.index("* loss      %.4f" % want[2][0]) == out.index("* median    %.2f%%" % np.median(want[2][1])) + 1
    rows = out_csv.read_text().splitlines()
    assert rows[0] == "weights,validation_loss,validation_mean,validation_median,chunks,duration" and len(rows) == 3
    for row, w in zip(rows[1:], (2, 10)):
        f = row.split(",")
        assert f[:5] == [str(w), "%.6f" % want[w][0], "%.4f" % np.mean(want[w][1]), "%.4f" % np.median(want[w][1]), str(N)]
        assert float(f[5]) >= 0.0

    # without the three flags: the evaluator's lines as they were, values of time and samples/s aside
    evaluate.main(evaluate.argparser().parse_args(argv + ["--weights", "10,2"]))
    out = capsys.readouterr().out.splitlines()
    expect = [("* loading data", True)]                       # (text, whole line) or (prefix of a line whose value is a time, False)
    for w in (10, 2):
        expect += [("* loading model %d" % w, True), ("* calling", True), ("* decoding refs", True), ("* computing accuracies", True),
                   ("* mean      %.2f%%" % np.mean(want[w][1]), True), ("* median    %.2f%%" % np.median(want[w][1]), True),
                   ("* time      ", False), ("* samples/s ", False)]
    assert len(out) == len(expect), out
    for got, (text, whole) in zip(out, expect):
        assert got == text if whole else got.startswith(text), (got, text)
