"""Test infrastructure for the `segment` tests: seeded inputs shared by tests/test_segment_host.py and tests/test_gpu_segment.py."""
import itertools
import os

import numpy as np

# Share of the bases of write_ctc_dir's default directory whose recovered breakpoint lies within 3 samples of the planted one.
# A sanity figure, not a contract: the restatement alone (dtw_ref on the host, seed 25, no band; the same with -w 4, seed 3)
# measures 0.9443; asserted with a small margin.
PLANTED_WITHIN_3 = 0.93


def problem(rng, N, K, quantised=False):
    """One chunk of N samples and K levels.  quantised: fp16 chunk values on a grid of quarters and levels in quarters, so
    that path costs tie outside the repeated columns too."""
    q = rng.normal(0.0, 1.0, N)
    lev = rng.normal(0.0, 1.0, K)
    if quantised:
        q = np.round(q * 4.0) / 4.0
        lev = np.round(lev * 4.0) / 4.0
        return q.astype(np.float16).astype(np.float32), lev.astype(np.float64)
    return q.astype(np.float32), lev.astype(np.float64)


def batch(rng, N, Ks, quantised=False):
    sig, levels = [], []
    for K in Ks:
        q, lev = problem(rng, N, K, quantised)
        sig.append(q)
        levels.append(lev)
    return np.stack(sig), levels


def level_counts(N, rep):
    """K from 1 up to and beyond N / rep: 1, 2, a third and a half of the most that fits, the most that fits (M = N when rep
    divides N), one and several more than fit (those chunks fail)."""
    top = N // rep
    ks = {1, 2, max(1, top // 3), max(1, top // 2), max(1, top - 1), max(1, top), top + 1, top + 5}
    return sorted(ks)


def write_poremodel(path, seed=3, letters="ACGT"):
    """A seeded 6-mer pore model in the reference's file format (every 6-mer over `letters`)."""
    rng = np.random.RandomState(seed)
    with open(path, "w") as fh:
        fh.write("#model_name\tsynthetic.6mer\n#type\tbase\nkmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\n")
        for kmer in itertools.product(letters, repeat=6):
            fh.write("%s\t%.4f\t%.4f\t%.4f\t%.4f\n" % ("".join(kmer), rng.uniform(60.0, 125.0), rng.uniform(0.8, 3.0), 1.0, 0.3))
    return path


def write_ctc_dir(path, poremodel, n=12, N=1000, seed=9, noise=0.15):
    """A synthetic ctc-data directory: per chunk a random ACGT reference, every base's (normalised) level held for a random
    5-15 samples plus Gaussian noise.  Returns the planted breakpoints, a list of (length,) arrays."""
    from xna_basecaller_amd import segment as seg
    rng = np.random.RandomState(seed)
    os.makedirs(path, exist_ok=True)
    chunks = np.zeros((n, N), np.float32)
    seqs, planted = [], []
    for c in range(n):
        durations = []
        while sum(durations) < N:
            durations.append(int(rng.randint(5, 16)))
        over = sum(durations) - N
        durations[-1] -= over
        if durations[-1] < 5:                               # fold a short last base into the one before it
            last = durations.pop()
            durations[-1] += last
        labels = rng.randint(1, 5, len(durations))
        levels = seg.reference_levels(labels, len(labels), poremodel, rng=np.random.RandomState(1000 + c), chunk=c)
        chunks[c] = np.repeat(levels, durations) + rng.normal(0.0, noise, N)
        seqs.append(labels)
        planted.append(np.cumsum(durations))
    lengths = np.array([len(s) for s in seqs], np.uint16)
    refs = np.zeros((n, int(lengths.max()) + 3), np.uint8)
    for c, s in enumerate(seqs):
        refs[c, :len(s)] = s
    np.save(os.path.join(path, "chunks.npy"), chunks)
    np.save(os.path.join(path, "references.npy"), refs)
    np.save(os.path.join(path, "reference_lengths.npy"), lengths)
    return planted
