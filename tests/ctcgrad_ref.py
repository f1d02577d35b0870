"""The numpy restatement of xb_ctc_loss_grad (include/xna_basecaller.h), built from what the oracle already offers, and the label
rows the gradient tests share (no device; tests/test_ctcgrad_host.py is the CPU tier, tests/test_gpu_ctcgrad.py the GPU tier).

  logz_crf, P = oracle.decode(scores, want=('logz', 'post'))            the CRF's log partition function and edge posteriors
  x           = scores - logz_crf / T                                   float32, one division per chunk
  logz, gstay, gmove = oracle.ctc_logz(x, want_grads=True)              the lattice and its restricted posteriors
  R           = np.add.at over (stay_idx, move_idx) in row order        repeated k-mers add up in ascending position
  grad        = (R - P) * w,  w = -(1 / length) [/ N], 0 where clipped  three float32 operations

The blank-less layout expands the blank column with the blank score, runs the same and drops the blank columns."""
import numpy as np

import oracle
from ctc_wide_cases import BLANK, with_blank


def has_path(T, lens, sl):
    """The precondition of xb_ctc_loss_grad per chunk: T >= length - state_len (a row without a path gives unspecified values)."""
    return T >= np.asarray(lens) - sl


def reference(scores, targets, lens, nb, sl, has_blank, loss_clip=None, reduction="mean", blank=BLANK):
    """(loss (N,) float32, clamped when clipping; grad (T, N, C) float32 in the layout of scores)."""
    scores = np.ascontiguousarray(scores, np.float32)
    full = scores if has_blank else with_blank(scores, nb, blank)
    T, N, C = full.shape
    lens = np.asarray(lens, np.int32)
    targets = np.ascontiguousarray(targets, np.int32)
    d = oracle.decode(full, nb, sl, want=("logz", "post"))
    x = full - (d["logz"] / np.float32(T))[None, :, None]
    assert x.dtype == np.float32
    o = oracle.ctc_logz(x, targets, lens, nb, sl, want_grads=True)
    loss = -(o["logz"] / lens.astype(np.float32))
    stay, move = oracle.ctc_indices(targets, nb, sl)
    R = np.zeros_like(full)
    bi = np.arange(N)[:, None]
    for t in range(T):
        np.add.at(R[t], (bi, stay), o["stay"][t])
        np.add.at(R[t], (bi, move), o["move"][t])
    w = -(np.float32(1.0) / lens.astype(np.float32))
    if reduction == "mean":
        w = w / np.float32(N)
    if loss_clip:
        w = np.where((loss >= 0.0) & (loss <= np.float32(loss_clip)), w, np.float32(0.0))
        loss = np.clip(loss, np.float32(0.0), np.float32(loss_clip))
    grad = (R - d["post"]) * w.astype(np.float32)[None, :, None]
    assert grad.dtype == np.float32 and loss.dtype == np.float32
    if not has_blank:
        S = C // (nb + 1)
        grad = np.ascontiguousarray(grad.reshape(T, N, S, nb + 1)[..., 1:]).reshape(T, N, S * nb)
    return loss, grad


def sharing(targets, lens, nb, sl):
    """Per chunk (largest number of positions of the chunk's own length that share one stay column, ... one move column)."""
    stay, move = oracle.ctc_indices(np.ascontiguousarray(targets, np.int32), nb, sl)
    out = []
    for b, ln in enumerate(np.asarray(lens)):
        n = int(ln) + 1 - sl
        s = np.bincount(stay[b, :n]).max()
        m = np.bincount(move[b, :n - 1]).max() if n > 1 else 0
        out.append((int(s), int(m)))
    return out


# ---- label rows built to collide ----------------------------------------------------------------------------------------
def row_one_letter(Lt, letter=1):
    return np.full(Lt, letter, np.uint8)


def row_period_two(Lt):
    return np.where(np.arange(Lt) % 2 == 0, 1, 2).astype(np.uint8)          # ACACAC...


def row_planted(rng, Lt, nb, sl, at):
    """A random row with one (sl + 1)-mer planted at the offsets `at`: the same stay AND move column at each."""
    row = rng.integers(1, nb + 1, Lt).astype(np.uint8)
    kmer = rng.integers(1, nb + 1, sl + 1).astype(np.uint8)
    for a in at:
        row[a:a + sl + 1] = kmer
    return row


def colliding_batch(nb, sl, Lt, seed=0):
    """(targets (4, Lt) uint8, lens): all one letter, period 2, a k-mer planted three times far apart, and a ragged mix (a
    homopolymer run, then period 2, cut short)."""
    rng = np.random.default_rng(seed)
    mix = np.concatenate([row_one_letter(Lt // 3, 2), row_period_two(Lt - Lt // 3)])
    t = np.stack([row_one_letter(Lt), row_period_two(Lt), row_planted(rng, Lt, nb, sl, (1, Lt // 2, Lt - sl - 2)), mix])
    lens = np.array([Lt, Lt - 1, Lt, Lt - 5], np.int32)
    for b in range(4):
        t[b, lens[b]:] = 0
    return t, lens
