"""A plain-Python restatement of xb_splice_chunks' contract (include/xna_basecaller.h): the reference's per_kmer XNA
augmentation (ub-bonito/bonito/stitch_chunks.py: choose_positions, stitch_read_per_kmer, prepare_slice_chunk) over a
library that xna_basecaller_amd.splice.build_library made, with the contract's counter-based draws in place of a numpy
generator.  Test infrastructure only: slow, scalar, float64 written out operation by operation."""
import math

import numpy as np

MASK64 = (1 << 64) - 1
GOLDEN_GAMMA = 0x9E3779B97F4A7C15
KMER_LEN = 6
TEMPLATES = 7 ** 5


def mix(z):
    """splitmix64's finaliser."""
    z &= MASK64
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & MASK64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & MASK64
    return z ^ (z >> 31)


class Draws:
    """Draw k of chunk c: z = mix(mix(seed + G (c + 1)) + G (k + 1)); k counts the draws of the chunk from 0.  `uniform` and
    `choice` take what the reference passes to its numpy generator and spend one draw per value they return."""

    def __init__(self, seed, chunk):
        self.base = mix(int(seed) + GOLDEN_GAMMA * (int(chunk) + 1))
        self.k = 0

    def next(self):
        self.k += 1
        return mix(self.base + GOLDEN_GAMMA * self.k)

    def bounded(self, m):
        return ((self.next() >> 32) * int(m)) >> 32

    def unit(self):
        return (self.next() >> 11) * 2.0 ** -53

    def uniform(self, lo, hi):
        return lo + (hi - lo) * self.unit()

    def choice(self, a, size=None, replace=True, p=None):
        assert p is None
        items = None if isinstance(a, (int, np.integer)) else a
        n = int(a) if items is None else len(a)
        if size is None:
            j = self.bounded(n)
            return j if items is None else items[j]
        size = int(size)
        if replace:
            picks = [self.bounded(n) for _ in range(size)]
        else:                                    # partial Fisher-Yates over the virtual identity permutation
            moved, picks = {}, []
            for j in range(size):
                r = j + self.bounded(n - j)
                vj, vr = moved.get(j, j), moved.get(r, r)
                moved[r] = vj
                picks.append(vr)
        return np.array(picks if items is None else [items[j] for j in picks])


def rint(x):
    """Half to even, as Python's round of a float64 and numpy's .round()."""
    return int(round(float(x)))


def linspace(start, stop, num):
    """numpy.linspace(start, stop, num) in float64: i * step + start, the last value replaced by stop."""
    if num == 1:
        return [float(start)]
    step = (float(stop) - float(start)) / float(num - 1)
    out = [float(i) * step + float(start) for i in range(num)]
    out[-1] = float(stop)
    return out


def stretch_points(slice_len, ins_len, kmer_cnts):
    """prepare_slice_chunk's xp (:247-261): per k-mer evenly spread integer sample positions that never mix two k-mers."""
    xp = [int(math.floor(v)) for v in linspace(0, ins_len - 1, slice_len)]
    left, offset, new_xp = 0, 0, []
    for cnt in kmer_cnts[:-1]:
        right = int(math.floor((xp[offset + cnt - 1] + xp[offset + cnt]) / 2.0))
        new_xp += [rint(v) for v in linspace(left, right, cnt)]
        left = right + 1
        offset += cnt
    new_xp += [rint(v) for v in linspace(left, ins_len - 1, kmer_cnts[-1])]
    return new_xp


def interp(n_out, xp, fp):
    """numpy.interp(arange(n_out), xp, fp) for non-decreasing integer xp with xp[0] = 0 and xp[-1] = n_out - 1."""
    out, j = [], 0
    for x in range(n_out):
        while j + 1 < len(xp) and xp[j + 1] <= x:
            j += 1
        if j == len(xp) - 1 or xp[j] == x:
            out.append(float(fp[j]))
        else:
            slope = (float(fp[j + 1]) - float(fp[j])) / (float(xp[j + 1]) - float(xp[j]))
            out.append(slope * (float(x) - float(xp[j])) + float(fp[j]))
    return out


def prepare(values, ins_len, kmer_cnts):
    """prepare_slice_chunk (:241-271) -> (float64 values of the window, 'stretch' | 'shrink' | 'copy')."""
    slice_len = len(values)
    if slice_len < ins_len:
        return interp(ins_len, stretch_points(slice_len, ins_len, kmer_cnts), values), "stretch"
    if slice_len > ins_len:
        n_rmv = slice_len - ins_len
        drop = set(int(math.floor(v)) for v in linspace(0, slice_len - 1, n_rmv))
        return [float(v) for i, v in enumerate(values) if i not in drop], "shrink"
    return [float(v) for v in values], "copy"


def choose_positions(length, n_pos, pad, ubs_pos, draws):
    mask = [10 <= p < length - 10 for p in range(length)]
    for pos in ubs_pos:
        for p in range(max(0, pos - 2 * pad), min(length, pos + 2 * pad + 1)):
            mask[p] = False
    chosen = []
    for _ in range(n_pos):
        valid = [p for p in range(length) if mask[p]]
        if not valid:
            break
        pos = valid[draws.bounded(len(valid))]
        for p in range(max(0, pos - pad), min(length, pos + pad + 1)):
            mask[p] = False
        chosen.append(pos)
    return sorted(chosen)


def table_index(ub, tpl, kmer_ub_pos):
    t = 0
    for v in tpl:
        t = t * 7 + int(v)
    return ((int(ub) - 5) * TEMPLATES + t) * KMER_LEN + int(kmer_ub_pos)


def splice_chunk(signal, target, length, bkp, library, chunk_index, seed, ubs, prop, var_prop, cand_sample_size, pad,
                 stats=None):
    """One chunk -> (signal float32, target uint8, success, inserted).  library: splice.Library (pool float16, rows
    (n_rows, 2) int32 pool offset and length, table (2 * 7^5 * 6, 2) int32 first row and count); ubs: labels (5, 6) in the
    order of the choice; stats (a dict) collects 'positions', 'stretch', 'shrink', 'copy', 'abandoned'."""
    out = np.array(signal, dtype=np.float32)
    out_t = np.array(target, dtype=np.uint8)
    length = int(length)
    tgt = [int(v) for v in np.asarray(target)[:length]]
    b = [int(v) for v in np.asarray(bkp)[:length]]
    draws = Draws(seed, chunk_index)
    stats = {} if stats is None else stats
    for key in ("positions", "stretch", "shrink", "copy", "abandoned"):
        stats.setdefault(key, 0)
    if var_prop is not None and var_prop > 0:
        prop = draws.uniform(prop - var_prop, prop + var_prop)
    ubs_pos = [p for p in range(length) if tgt[p] > 4]
    n_pos = max(rint(float(length) * float(prop)) - len(ubs_pos), 1)
    positions = choose_positions(length, n_pos, pad, ubs_pos, draws)
    stats["positions"] += len(positions)
    inserted = 0
    for pos in positions:
        ins_st, ins_en = b[pos - KMER_LEN], b[pos]
        st = tgt[pos - KMER_LEN + 1:pos + KMER_LEN]
        ub = ubs[draws.bounded(len(ubs))]
        reps = [b[pos - KMER_LEN + i + 1] - b[pos - KMER_LEN + i] for i in range(KMER_LEN)]
        picked = []
        for i in range(KMER_LEN):
            first, count = (int(v) for v in library.table[table_index(ub, st[6:6 + i] + st[i:5], KMER_LEN - 1 - i)])
            if count == 0:
                picked = []
                break
            if cand_sample_size > 1:
                cand = draws.choice(count, size=min(count, cand_sample_size), replace=False)
                lens = [int(library.rows[first + int(c), 1]) for c in cand]
                diffs = [abs(v - reps[i]) for v in lens]
                row = first + int(cand[diffs.index(min(diffs))])
            else:
                row = first + draws.bounded(count)
            picked.append(row)
        if not picked:
            stats["abandoned"] += 1
            continue
        values, cnts = [], []
        for row in picked:
            off, n = (int(v) for v in library.rows[row])
            values += [float(v) for v in library.pool[off:off + n]]
            cnts.append(n)
        window, kind = prepare(values, ins_en - ins_st, cnts)
        stats[kind] += 1
        out[ins_st:ins_en] = np.asarray(window, dtype=np.float64).astype(np.float32)
        out_t[pos] = ub
        inserted += 1
    return out, out_t, inserted > 0, inserted


def splice_batch(library):
    """A stand-in for Context.splice_chunks over `library` (what splice.splice takes as `run=`)."""
    def run(signal, targets, lengths, bkps, first_index, seed, ubs_mask, prop, var_prop, cand_sample_size, pad):
        ubs = [u for u in (5, 6) if ubs_mask >> (u - 5) & 1]
        n = signal.shape[0]
        out, out_t = np.empty(signal.shape, np.float32), np.empty(targets.shape, np.uint8)
        ok, ins = np.zeros(n, np.int8), np.zeros(n, np.int32)
        for c in range(n):
            out[c], out_t[c], ok[c], ins[c] = splice_chunk(signal[c], targets[c], lengths[c], bkps[c], library, first_index + c,
                                                           seed, ubs, prop, var_prop, cand_sample_size, pad)
        return out, out_t, ok, ins
    return run
