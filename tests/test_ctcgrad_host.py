"""CPU: what the reference of the gradient tests is worth.  tests/ctcgrad_ref.py (the restatement xb_ctc_loss_grad is held to bit
for bit on the GPU) against float64 torch autograd through the whole expression
-logZ_ctc(x - logZ_crf(x) / T) / length  (crf/model.py:118-131), at tests/test_ctc.py::test_gpu_model_ctc_loss_and_gradient's
shape and within its 2e-5; the same on label rows built to collide, where positions that share a score column add up."""
import numpy as np
import pytest
import torch

import oracle
import ctcgrad_ref as G
from conftest import random_scores
from ctc_wide_cases import BLANK, ctc_logz_f64, label_rows, with_blank

SL = 3


def _f64(sc, targets, lens, nb, sl, reduction="mean"):
    """(loss, d loss / d scores) in float64: the CRF's logZ by the dense recursion over the idx table, then the CTC lattice."""
    T, N, _ = sc.shape
    idx = torch.as_tensor(oracle.crf_idx(nb, sl).astype(np.int64))
    S, E = nb ** sl, nb + 1
    x = torch.tensor(sc, dtype=torch.float64, requires_grad=True)
    a = torch.zeros((N, S), dtype=torch.float64)
    for t in range(T):
        a = torch.logsumexp(x[t].reshape(N, S, E) + a[:, idx], dim=2)
    xn = x - (torch.logsumexp(a, dim=1) / T)[None, :, None]
    stay_idx, move_idx = oracle.ctc_indices(np.ascontiguousarray(targets, np.int32), nb, sl)
    lz = ctc_logz_f64(xn, stay_idx, move_idx, np.asarray(lens) + 1 - sl)
    per = -(lz / torch.as_tensor(np.asarray(lens), dtype=torch.float64))
    (per.mean() if reduction == "mean" else per.sum()).backward()
    return per.detach().numpy(), x.grad.numpy()


@pytest.mark.parametrize("nb", [4, 6])
def test_restatement_against_float64_autograd(nb):
    T, N, Lt = 30, 3, 10
    sc = random_scores(T, N, nb, seed=11)
    targets, lens = label_rows(np.random.default_rng(7), N, Lt, nb, SL)
    for reduction in ("mean", "none"):
        per, g64 = _f64(sc, targets, lens, nb, SL, reduction)
        loss, grad = G.reference(sc, targets, lens, nb, SL, True, reduction=reduction)
        print("nb %d, %s: max |loss - f64| = %.3g, max |grad - f64| = %.3g" % (nb, reduction, np.abs(loss - per).max(), np.abs(grad - g64).max()))
        assert np.abs(loss - per).max() < 2e-4
        assert np.abs(grad - g64).max() < 2e-5
    # the blank-less layout: the same gradient without the blank columns
    S, E = nb ** SL, nb + 1
    nbl = np.ascontiguousarray(sc.reshape(T, N, S, E)[..., 1:]).reshape(T, N, S * nb)
    assert np.array_equal(with_blank(nbl, nb), sc)
    loss_n, grad_n = G.reference(nbl, targets, lens, nb, SL, False)
    per, g64 = _f64(sc, targets, lens, nb, SL)
    assert np.array_equal(loss_n, G.reference(sc, targets, lens, nb, SL, True)[0])
    assert np.abs(grad_n - g64.reshape(T, N, S, E)[..., 1:].reshape(T, N, S * nb)).max() < 2e-5
    # clipping: the clipped chunks' gradient is zero and their loss clamped, the others keep theirs
    clip = float(np.sort(per)[1] + 1e-3)
    lc, gc = G.reference(sc, targets, lens, nb, SL, True, loss_clip=clip, reduction="none")
    l0, g0 = G.reference(sc, targets, lens, nb, SL, True, reduction="none")
    out = l0 > np.float32(clip)
    assert out.any() and not out.all()
    assert np.all(gc[:, out] == 0) and np.array_equal(gc[:, ~out], g0[:, ~out])
    assert np.all(lc[out] == np.float32(clip)) and np.array_equal(lc[~out], l0[~out])


@pytest.mark.parametrize("nb", [4, 6])
def test_colliding_rows_against_float64_autograd(nb):
    """Positions with the same k-mer share a stay column, with the same preceding base also a move column: their restricted
    posteriors add up.  An all-A row shares both among all its positions; the planted k-mer shares both three times."""
    T, Lt = 40, 24
    targets, lens = G.colliding_batch(nb, SL, Lt, seed=nb)
    share = G.sharing(targets, lens, nb, SL)
    assert share[0][0] >= 3 and share[0][1] >= 3, share          # all one letter
    assert share[0] == (Lt - SL + 1, Lt - SL)
    assert share[1][0] >= 3 and share[1][1] >= 3, share          # period 2
    assert share[2][0] >= 3 and share[2][1] >= 3, share          # planted three times
    assert share[3][0] >= 3 and share[3][1] >= 3, share          # the ragged mix
    assert G.has_path(T, lens, SL).all()
    sc = random_scores(T, 4, nb, seed=5)
    per, g64 = _f64(sc, targets, lens, nb, SL)
    loss, grad = G.reference(sc, targets, lens, nb, SL, True)
    print("nb %d: max |loss - f64| = %.3g, max |grad - f64| = %.3g" % (nb, np.abs(loss - per).max(), np.abs(grad - g64).max()))
    assert np.abs(loss - per).max() < 2e-4
    assert np.abs(grad - g64).max() < 2e-5
    # every time step carries one lattice edge and one CRF edge of a path: a chunk's gradient sums to zero per step
    assert np.abs(grad.sum(axis=2)).max() < 2e-5
