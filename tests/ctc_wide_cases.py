"""The CTC lattice kernels at every width up to 2048 positions: the table of cases, their builders and the helpers the CTC
tests share (no device; tests/test_ctc_wide_host.py is the CPU tier, tests/test_gpu_ctc_wide.py the GPU tier).

ctc_scan_kernel and ctc_loss_kernel (xb_ctc.hip) put lattice position l on thread l % threads and keep up to 8 positions per
thread, slot k = l // threads.  A case is (nb, sl, np, T): np positions, a label row of Lt = np + sl - 1 labels, T time steps.
Position l is unreachable before step l, so a full-width case takes T = np + 1 .. np + 4 (the row's end cell is live in the last
steps only, and T runs through all residues of the kernels' 4-deep prefetch ring).  Every case holds three chunks: the full row,
a chunk of about half the positions (from 256 positions on it ends one past a multiple of 256: a wide band of live cells in a
launch sized for the full row), and a chunk of exactly sl labels (one position)."""
import collections

import numpy as np
import torch

import oracle
from conftest import random_scores

BLANK = 2.0
THREADS = 256                       # the widest workgroup (every row above 128 positions): the slot of position l is l // THREADS
PMAX = 8                            # positions per thread at most, in both kernels
ZERO = np.float32(-1e38)            # seqdist's Log.zero / Max.zero

Case = collections.namedtuple("Case", "nb sl np T")

# (np, T - np) at nb 4, sl 3.  The scan table puts a lone position in slot 1 (257), 2 (513), 4 (1025) and 7 (1793) and fills all
# 8 slots at 2048; T mod 4 over it is 1, 3, 0, 2, 2, 0, 1, 0, 2.
_SCAN_MAIN = [(256, 1), (257, 2), (512, 4), (513, 1), (1024, 2), (1025, 3), (1793, 4), (2047, 1), (2048, 2)]
# both sides of every step of ctc_loss_threads (64 threads up to 64 positions, 128 up to 128, 256 above)
_LOSS_EXTRA = [(64, 3), (65, 4), (128, 1), (129, 2)]
# the other geometries: six bases, the shortest and the longest state
_GEOMETRY = [Case(6, 3, 1025, 1029), Case(5, 2, 513, 515), Case(4, 5, 513, 516)]

LOSS_CASES = [Case(4, 3, n, n + d) for n, d in _LOSS_EXTRA + _SCAN_MAIN] + _GEOMETRY
SCAN_CASES = LOSS_CASES             # the scan follows the loss's launch rule: one table
PROPERTY_POSITIONS = [257, 513, 1025, 2048]          # the single-path and the infeasible batches (nb 4, sl 3)
F64_POSITIONS = [513, 1025, 2048]                    # the main-table rows the oracle is held against float64 at

# XB_CTC_LOSS_THREADS (np, value): accepted where the value is 64 / 128 / 256 and value * 8 >= np, else the rule's choice holds
THREAD_OVERRIDES = [(129, 64), (257, 64), (257, 128), (512, 64), (1024, 128), (1025, 256), (513, 64), (257, 100)]

# The oracle (float32, xo_ctc_logz) against the float64 lattice on the F64_POSITIONS cases, measured on the CPU by
# tests/test_ctc_wide_host.py::test_oracle_against_float64_at_wide_rows (it prints the figures): the largest deviation of the
# Log and the Max logz relative to max(1, |logz|), and of the per-step sum of the restricted posteriors from 1.  The bound is
# 4 x the measured maximum, because another seed moves the figure by about that much.  The device is held to bit-equality with
# the oracle and never sets these numbers.
F64_LOGZ_MEASURED = 5.62e-7           # at 2048 positions (4.2e-7 at 513 and 1025)
F64_MAX_MEASURED = 5.52e-7            # at 2048 positions (2.32e-7 at 513, 5.18e-7 at 1025)
F64_GRADSUM_MEASURED = 3.95e-3        # at 2048 positions (7.75e-4 at 513, 2.38e-3 at 1025): logz is about 6100 there
F64_LOGZ_BOUND = 4 * F64_LOGZ_MEASURED
F64_MAX_BOUND = 4 * F64_MAX_MEASURED
F64_GRADSUM_BOUND = 4 * F64_GRADSUM_MEASURED


def case_id(c):
    return "nb%d-sl%d-np%d-T%d" % c


def half_positions(np_):
    """The second chunk's positions: the largest of 257 / 513 / 1025 below the row's, else just over half."""
    fit = [m for m in (257, 513, 1025) if m < np_]
    return max(fit) if fit else np_ // 2 + 1


def label_rows(rng, N, Lt, nb, sl, lens=None, dtype=np.int32):
    """Ragged label rows 1 .. nb, zero beyond each row's length.  Without lens: random lengths with the longest and the shortest
    legal targets first and last."""
    t = rng.integers(1, nb + 1, (N, Lt)).astype(dtype)
    if lens is None:
        lens = rng.integers(sl, Lt + 1, N)
        lens[0], lens[-1] = Lt, sl
    lens = np.asarray(lens, dtype=np.int32)
    for b in range(N):
        t[b, lens[b]:] = 0
    return t, lens


def build(c, with_blank=True):
    """A table case: (scores (T, 3, C) from conftest.random_scores, targets (3, Lt) int32, lengths (3,))."""
    Lt = c.np + c.sl - 1
    rng = np.random.default_rng(c.np * 8 + c.nb)
    targets, lens = label_rows(rng, 3, Lt, c.nb, c.sl, lens=[Lt, half_positions(c.np) + c.sl - 1, c.sl])
    return random_scores(c.T, 3, c.nb, sl=c.sl, seed=c.np + (0 if with_blank else 1), with_blank=with_blank), targets, lens


def build_single_path(np_, with_blank=True, nb=4, sl=3):
    """T = np - 1: the full row's only path moves at every step (the diagonal); beside it a one-position chunk."""
    Lt = np_ + sl - 1
    targets, lens = label_rows(np.random.default_rng(np_), 2, Lt, nb, sl, lens=[Lt, sl])
    return random_scores(np_ - 1, 2, nb, sl=sl, seed=np_ + 2, with_blank=with_blank), targets, lens


def build_infeasible(np_, with_blank=True, nb=4, sl=3):
    """T = np - 2: the full row has no path; its neighbour, one label shorter, has the diagonal alone."""
    Lt = np_ + sl - 1
    targets, lens = label_rows(np.random.default_rng(np_ + 1), 2, Lt, nb, sl, lens=[Lt, Lt - 1])
    return random_scores(np_ - 2, 2, nb, sl=sl, seed=np_ + 3, with_blank=with_blank), targets, lens


def with_blank(blankless, nb, blank=BLANK):
    """Blank-less scores (T, N, S nb) with the constant blank column put back: (T, N, S (nb + 1))."""
    T, N, C = blankless.shape
    full = np.empty((T, N, C // nb, nb + 1), np.float32)
    full[..., 0] = np.float32(blank)
    full[..., 1:] = blankless.reshape(T, N, C // nb, nb)
    return full.reshape(T, N, -1)


def normalised(ctx, scores, nb, has_blank):
    """What ctc_loss_kernel computes as it fetches: the blank-expanded scores minus c = logz_crf / T, in float32; and c."""
    c = ctx.crf_logz(scores, has_blank=has_blank) / np.float32(scores.shape[0])
    x = (scores if has_blank else with_blank(scores, nb)) - c[None, :, None]
    assert x.dtype == np.float32 and c.dtype == np.float32
    return x, c


def loss_reference(ctx, scores, targets, lens, nb, sl, has_blank):
    """The host composition xb_ctc_loss replaced: xb_crf_logz, `scores - logz / T` in float32, oracle.ctc_logz on the result,
    `-(logz / length)`: (loss, logz_ctc)."""
    x, _ = normalised(ctx, scores, nb, has_blank)
    logz = oracle.ctc_logz(x, targets.astype(np.int32), lens, nb, sl)["logz"]
    return -(logz / lens.astype(np.float32)), logz


def running_sum(values):
    """run = float32(run + v) in order, from 0."""
    run = np.float32(0.0)
    for v in np.asarray(values, np.float32):
        run = np.float32(run + v)
    return run


def diagonal_sum(x, targets, b, nb, sl, steps):
    """The float32 running sum of chunk b's move scores on the diagonal: step t moves from position t to t + 1."""
    _, move_idx = oracle.ctc_indices(targets, nb, sl)
    return running_sum(x[np.arange(steps), b, move_idx[b, :steps]])


def stay_sum(x, targets, b, nb, sl):
    """The float32 running sum of the stay scores of chunk b's position 0 over all steps."""
    stay_idx, _ = oracle.ctc_indices(targets, nb, sl)
    return running_sum(x[:, b, stay_idx[b, 0]])


def loss_launch(np_, override=None):
    """ctc_launch's arithmetic (xb_ctc_lattice.h) restated: (threads, the PMAX of the instantiation) for np positions under an
    XB_CTC_LOSS_THREADS of `override` (the loss and gradient calls; the scans take the rule alone)."""
    threads = 64 if np_ <= 64 else (128 if np_ <= 128 else 256)
    if override in (64, 128, 256) and override * PMAX >= np_:
        threads = override
    per = -(-np_ // threads)
    assert per <= PMAX
    return threads, (1 if per <= 1 else 2 if per <= 2 else 4 if per <= 4 else 8)


def ctc_logz_f64(x, stay_idx, move_idx, npos, semiring="log"):
    """float64 torch restatement over the dense scores x (T, N, C): returns logz (N,) as a differentiable tensor."""
    T, N, _ = x.shape
    n = stay_idx.shape[1]
    out = []
    zero = torch.full((1,), -1e38, dtype=torch.float64)
    for b in range(N):
        a = torch.full((n,), -1e38, dtype=torch.float64)
        a[0] = 0.0
        si = torch.as_tensor(stay_idx[b], dtype=torch.long)
        mi = torch.as_tensor(move_idx[b], dtype=torch.long)
        for t in range(T):
            x0 = a + x[t, b, si]
            x1 = torch.cat([zero, a[:-1] + x[t, b, mi]])
            st = torch.stack([x0, x1])
            a = torch.logsumexp(st, 0) if semiring == "log" else st.max(0).values
        out.append(a[npos[b] - 1])
    return torch.stack(out)


def lattice_f64(scores, stay_idx, move_idx, npos, semiring="log"):
    """The same lattice in float64 numpy, all chunks at once and without a graph (the wide rows take thousands of steps): logz (N,)."""
    x = np.asarray(scores, np.float64)
    T, N, _ = x.shape
    bi = np.arange(N)[:, None]
    a = np.full((N, stay_idx.shape[1]), -1e38)
    a[:, 0] = 0.0
    x1 = np.full_like(a, -1e38)
    for t in range(T):
        x0 = a + x[t][bi, stay_idx]
        x1[:, 1:] = a[:, :-1] + x[t][bi, move_idx]
        a = np.logaddexp(x0, x1) if semiring == "log" else np.maximum(x0, x1)
    return a[np.arange(N), np.asarray(npos) - 1]
