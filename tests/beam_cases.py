"""The inputs of the beam-search tests (tests/test_beam_cases_host.py on the CPU, tests/test_gpu_beam.py on the GPU): the score
generators and ONE table of named cases, numpy only.

  Case    name, (nb, sl, T, N, W, cut, with_blank, scale, offset), gen + seed + kw (the generator, its seed, its constants),
          need: the columns of the oracle's branch census (oracle.BEAM_CENSUS) that must be non-zero over the case's chunks,
          every: the columns that must equal the number of blocks (or, for start_tied, 1) in every chunk.
  CASES   the table; scores(case) builds a case's (T, N, C) float32 tensor, the same bytes on every call.
          blank_wins rows must call exactly one base per chunk, dominant rows only qualities of 50 (the host test knows).

A case exists FOR the branches it names: if an edit to a generator or a seed loses one, the CPU test fails, and the remedy is
another seed or other constants, never a shorter `need`.

Score layout (crf/model.py:31-36): row j of (S, nb) holds the steps INTO state j, column k from the state k * nb^(sl-1) + j // nb;
with the blank column the row is (stay on j, steps...).  The blank-less form stays at the constant BLANK.

  gauss       gain * N(0,1) steps; the learned blank is BLANK + 0.25 * N(0,1).  85-95 % of the blocks emit.
  ridge       noise * N(0,1) steps around one random path that stays on ~60 % of the blocks: on a block where it stays every
              step is lowered by `lift`, on a block where it steps its own edge is raised by 2 + lift.  40-50 % of the blocks emit, a
              base spans several blocks, and a stay is often better than the step it merges with.
  zero        all-zero steps and blanks: every candidate of a block is equal.
  grid        round(5 * tanh(N(0,1))): integer scores, so that a stay and the step it merges with tie exactly.
  steep       8 * 5 * tanh(N(0,1)): posteriors of 1, qualities at the upper clamp.
  blank_wins  every step -5, every blank +5: one base over T blocks.
  dominant    one path at +20 against -20 that steps every third block and stays (blank +20) between.
"""
import collections
import math

import numpy as np

from pairs import PAIRS

BLANK = 2.0
FLT_MAX = float(np.finfo(np.float32).max)
ALPHA = {4: "NACGT", 5: "NACGTX", 6: "NACGTXY", 2: "NAC", 3: "NACG"}
QS, QO = 0.9722, 0.3498          # the shipped model's [qscore] section

Case = collections.namedtuple("Case", "name nb sl T N W cut with_blank scale offset gen seed kw need every")


def _path(rng, nb, sl, T, stay):
    """One chunk's random path: per block (state after the block, leading digit of the state before it or -1 for a stay)."""
    S, hi = nb ** sl, nb ** (sl - 1)
    st, out = int(rng.integers(S)), []
    for t in range(T):
        if t and rng.random() < stay:
            out.append((st, -1))
        else:
            j = (st % hi) * nb + int(rng.integers(nb))
            out.append((j, st // hi))
            st = j
    return out


def gauss(rng, nb, sl, T, N, gain=3.0):
    S = nb ** sl
    steps = (gain * rng.standard_normal((T, N, S * nb))).astype(np.float32).reshape(T, N, S, nb)
    blank = (BLANK + 0.25 * np.random.default_rng(1).standard_normal((T, N, S))).astype(np.float32)
    return steps, blank


def ridge(rng, nb, sl, T, N, lift=1.5, noise=1.5, stay=0.6):
    S = nb ** sl
    steps = (noise * rng.standard_normal((T, N, S, nb))).astype(np.float32)
    blank = (BLANK + 0.25 * rng.standard_normal((T, N, S))).astype(np.float32)
    for n in range(N):
        for t, (j, k) in enumerate(_path(rng, nb, sl, T, stay)):
            if k < 0:
                steps[t, n] -= np.float32(lift)
            else:
                steps[t, n, j, k] += np.float32(2.0 + lift)
    return steps, blank


def zero(rng, nb, sl, T, N):
    S = nb ** sl
    return np.zeros((T, N, S, nb), np.float32), np.zeros((T, N, S), np.float32)


def grid(rng, nb, sl, T, N):
    S = nb ** sl
    steps = np.round(5.0 * np.tanh(rng.standard_normal((T, N, S, nb)))).astype(np.float32)
    return steps, np.full((T, N, S), BLANK, np.float32)


def steep(rng, nb, sl, T, N):
    S = nb ** sl
    steps = (8.0 * 5.0 * np.tanh(rng.standard_normal((T, N, S, nb)))).astype(np.float32)
    return steps, np.full((T, N, S), BLANK, np.float32)


def blank_wins(rng, nb, sl, T, N):
    S = nb ** sl
    return np.full((T, N, S, nb), -5.0, np.float32), np.full((T, N, S), 5.0, np.float32)


def dominant(rng, nb, sl, T, N):
    S = nb ** sl
    steps, blank = np.full((T, N, S, nb), -20.0, np.float32), np.full((T, N, S), -20.0, np.float32)
    for n in range(N):
        st = int(rng.integers(S))
        for t in range(T):
            if t % 3 == 0:
                j = (st % (S // nb)) * nb + int(rng.integers(nb))
                steps[t, n, j, st // (S // nb)] = 20.0
                st = j
            else:
                blank[t, n, st] = 20.0
    return steps, blank


GENERATORS = {f.__name__: f for f in (gauss, ridge, zero, grid, steep, blank_wins, dominant)}
NEEDS_BLANK_COLUMN = ("zero", "blank_wins", "dominant")      # their blank is no constant 2.0


def scores(c):
    """The case's (T, N, C) float32 scores: C = S * (nb + 1) with the blank column, else S * nb (stay = the constant BLANK)."""
    steps, blank = GENERATORS[c.gen](np.random.default_rng(c.seed), c.nb, c.sl, c.T, c.N, **dict(c.kw))
    if not c.with_blank:
        assert c.gen not in NEEDS_BLANK_COLUMN
        return np.ascontiguousarray(steps).reshape(c.T, c.N, -1)
    full = np.empty((c.T, c.N, c.nb ** c.sl, c.nb + 1), np.float32)
    full[..., 0], full[..., 1:] = blank, steps
    return full.reshape(c.T, c.N, -1)


def strings(plane):
    return [bytes(r[r != 0].astype(np.uint8)).decode() for r in plane]


CASES = []


def case(name, nb, sl, T, gen, seed, N=3, W=32, cut=100.0, with_blank=False, scale=QS, offset=QO, kw=(), need=(), every=()):
    assert name not in {c.name for c in CASES}, name
    CASES.append(Case(name, nb, sl, T, N, W, cut, with_blank, scale, offset, gen, seed, tuple(sorted(dict(kw).items())),
                      tuple(need), tuple(every)))


# ---- every pair x the edges of the 64-block trace-back tile and both parities of the double buffer x both blank forms: both DMA
# widths, every remainder of the row and of S modulo 64 and 256, the largest LDS carve ((4, 5) with the blank column)
SWEEP_T = (1, 2, 63, 64, 65, 129)
RESEED = {(4, 3, 64): 1, (4, 4, 63): 1}      # the formula's seed gives a chunk with fewer bases than 0.3 T there
for _nb, _sl in PAIRS:
    for _T in SWEEP_T:
        for _wb in (False, True):
            _ridge = _T >= 63
            case("sweep-%d-sl%d-T%d-%s" % (_nb, _sl, _T, "blank" if _wb else "const"), _nb, _sl, _T, "ridge" if _ridge else "gauss",
                 seed=1000 * _nb + 100 * _sl + _T + RESEED.get((_nb, _sl, _T), 0), with_blank=_wb, need=("merges", "bisect", "short") if _ridge else ())

# ---- no cut: merged-away candidates stay in the beam and are carried on, their hashes match several steps and several stays
# claim one step: the kernel's one-merge-at-a-time branch (reached with 4 bases only)
for _sl in (2, 3, 4, 5):
    for _T in (20, 65):
        case("nocut-4-sl%d-T%d" % (_sl, _T), 4, _sl, _T, "gauss", seed=40 + _sl + _T, cut=0.0, need=("multi", "clash", "merges"))

# ---- widths (kept counts from (W * 8) // 10 = 0, 1, 4, 24) and cuts (log cut = 0: only the maximum's equals survive; a narrow
# cut; a cut nothing falls under)
for _gen, _nb, _sl in (("ridge", 5, 3), ("gauss", 4, 2)):
    for _W in (1, 2, 5, 31):
        case("width-%s-W%d" % (_gen, _W), _nb, _sl, 100, _gen, seed=7 * _W + _nb, W=_W, need=("bisect", "merges") if _W > 1 else ("bisect",))
    for _cut in (1.0, 1.5, 1e30):
        case("cut-%s-%g" % (_gen, _cut), _nb, _sl, 100, _gen, seed=11 + _nb, cut=_cut, need=("bisect",) if _cut > 2 else ("short",))

# ---- extremes
EXTREME_PAIRS = ((6, 2), (4, 4), (4, 3))
for _nb, _sl in EXTREME_PAIRS:
    _id = "%d-sl%d" % (_nb, _sl)
    case("zero-" + _id, _nb, _sl, 50, "zero", seed=0, with_blank=True, every=("bisect", "ten_guesses", "start_tied"))
    case("grid-" + _id, _nb, _sl, 50, "grid", seed=3 + _nb + _sl, need=("tie", "merges"))
    case("steep-" + _id, _nb, _sl, 50, "steep", seed=5 + _nb, need=("q50",))
    case("blank_wins-" + _id, _nb, _sl, 50, "blank_wins", seed=0, with_blank=True)
    case("dominant-" + _id, _nb, _sl, 50, "dominant", seed=9 + _sl, with_blank=True, need=("q50",))
    case("gain10-" + _id, _nb, _sl, 50, "gauss", seed=20, kw={"gain": 10.0}, need=("far",))
# 625 states and one block of nearly flat scores: the path k-mer and its 10 neighbours hold ~ 11 / 625 of the mass, an error
# probability of 0.8, phred 0.96 -- below the lower clamp without the shipped calibration's offset
case("q1-5-sl4-T1", 5, 4, 1, "gauss", seed=2, scale=1.0, offset=0.0, kw={"gain": 0.5}, need=("q1",))

BY_NAME = {c.name: c for c in CASES}


def _beam_py(M, beta, nb, sl, W, log_cut):
    """float64 restatement of the search for one chunk; hypotheses are keyed by their state sequence (no hashes).
    M (T, S, E) with the stay score in column 0; returns (score, path states (T,), moves (T,))."""
    T, S, hi = M.shape[0], nb ** sl, nb ** (sl - 1)
    thr = sorted(beta[0], reverse=True)[W] if W < S else -math.inf
    front = [((s,), s, 0.0) for s in range(S) if beta[0][s] >= thr][:W]
    hist = [[(s, 0, False) for (_, s, _) in front]]
    for t in range(T):
        cands = []
        for p, (key, st, score) in enumerate(front):
            for b in range(nb):
                j, k = (st % hi) * nb + b, st // hi
                cands.append([key + (j,), j, score + M[t, j, 1 + k] + beta[t + 1][j], p, False])
        for p, (key, st, score) in enumerate(front):
            cands.append([key, st, score + M[t, st, 0] + beta[t + 1][st], p, True])
            si = len(cands) - 1
            for q in range(len(front)):
                ti = q * nb + st % nb
                if cands[ti][0] == key:
                    a, b = cands[si][2], cands[ti][2]
                    f = max(a, b) + (math.log1p(math.exp(-abs(a - b))) if abs(a - b) < 17.0 else 0.0)
                    if a > b:
                        cands[si][2], cands[ti][2] = f, -FLT_MAX
                    else:
                        cands[ti][2], cands[si][2] = f, -FLT_MAX
        mx = max(c[2] for c in cands)
        cutoff = mx - log_cut
        count = sum(c[2] >= cutoff for c in cands)
        if count > W:
            lo, hi_s, guesses = cutoff, mx, 1
            while (count > W or count < (W * 8) // 10) and guesses < 10:
                if count > W:
                    lo, cutoff = cutoff, (cutoff + hi_s) / 2
                else:
                    hi_s, cutoff = cutoff, (cutoff + lo) / 2
                count = sum(c[2] >= cutoff for c in cands)
                guesses += 1
            if guesses == 10:
                cutoff = hi_s
        kept = [c for c in cands if c[2] >= cutoff][:W]
        if t == T - 1:
            best = max(range(len(kept)), key=lambda i: (kept[i][2], -i))
            kept[0], kept[best] = kept[best], kept[0]
        hist.append([(c[1], c[3], c[4]) for c in kept])
        front = [(c[0], c[1], c[2] - beta[t + 1][c[1]]) for c in kept]
    path, moves, el = [0] * T, [0] * T, 0
    for t in range(T, 0, -1):
        st, prev, stay = hist[t][el]
        path[t - 1], moves[t - 1], el = st, 0 if stay else 1, prev
    moves[0] = 1
    return front[0][2], path, moves
