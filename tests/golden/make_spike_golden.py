"""Regenerates tests/golden/spike.npz and spike.json: what the reference's synthetic spiking computes on small synthetic
ctc-data, with the contract's draws (tests/spike_ref.py: Sequential, Stream) replayed through its random generator.

Run in the BUILD container only.  It imports, BY FILE PATH and as reference code, ub-bonito/bonito/spike_chunks.py (numpy,
pandas and scipy are all it needs) and runs spike_read with equal_kmer_reps=False.  Only DATA is stored: the inputs, a
synthetic k-mer model, the reference's chunks, labels, positions, unnatural bases, med and mad, and counts of what the cases
exercise.

The generator is an np.random.RandomState subclass whose uniform / choice / shuffle return the contract's draws: stream 0 in
spike_read and choose_positions, stream 1 in compute_med_mad_squiggly, stream 2 + j in the j-th call of sim_signals (the
shift choice is draw 0, the scalar uniform of the variable noise draw 1, the first array of uniforms draws 2 .., the second
2 + len ..).  scipy's truncnorm.rvs takes its uniforms from random_state.uniform(size=...) and applies its own ppf, so the
truncated-normal values are the reference's own route to the quantile: the restatement's (AS241) may differ from it in the
last bits of float64, which float32 rounding shows as at most one step; the json records how many values differ at all.

The DNA alphabet has two letters (labels 1, 2) and the tail adds T, so the model holds the 3^6 k-mers over A C T and those
with one X or Y among them.  Both files are byte-for-byte reproducible (the archive's time stamps are fixed).
"""
import importlib.util
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import spike_ref  # noqa: E402
from make_splice_golden import write_npz  # noqa: E402
from xna_basecaller_amd import spike as sk  # noqa: E402

REFTREE = "/root/reference"
SEED = 2012
N_CHUNKS, N_SAMPLES, LT = 30, 480, 64
CASES = [   # name, ubs, prop_ubs, var_prop_ubs, pad, std_dist, noise_std, variable_noise
    ("uniform_xy", "XY", 0.08, None, 5, "uniform", 0.0, False),
    ("shift_variable_noise_xy", "XY", 0.08, None, 5, "truncnorm_shift_1.5_0.5", 1.0, True),
    ("truncnorm_fixed_noise_y", "Y", 0.10, None, 5, "truncnorm", 0.5, False),
    ("resynthesis_n", "N", 0.10, None, 5, "uniform", 0.0, False),
    ("one_x_pad3", "X", 0.12, None, 3, "uniform", 0.0, False),
    ("var_prop_xy", "XY", 0.10, 0.05, 5, "uniform", 0.0, False),
    ("uniform_fixed_noise_xy", "XY", 0.08, 0.02, 5, "uniform", 1.0, False),
]


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_spike_chunks", os.path.join(REFTREE, "ub-bonito", "bonito", "spike_chunks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


class Replay(np.random.RandomState):
    """The contract's draws of one chunk behind numpy's generator interface."""

    def __init__(self, seed, chunk):
        super().__init__(0)
        self.at = (seed, chunk)
        self.sequential = spike_ref.Sequential(seed, chunk)
        self.stream, self.arrays = None, 0

    def begin(self, stream):
        self.stream, self.arrays = spike_ref.Stream(*self.at, stream), 0

    def uniform(self, low=0.0, high=1.0, size=None):
        if self.stream is None:
            assert size is None and np.ndim(low) == 0
            return low + (high - low) * self.sequential.unit()
        if size is None and np.ndim(low) == 0:               # the variable noise std
            return low + (high - low) * self.stream.unit(1)
        n = int(np.prod(size)) if size is not None else len(low)
        first = 0 if self.stream.base == spike_ref.stream_base(*self.at, 1) else 2 + self.arrays * n
        self.arrays += 1
        return low + (high - low) * self.stream.units(first, n)

    def choice(self, a, size=None, replace=True, p=None):
        assert p is None
        if self.stream is None:                              # choose_positions: rng.choice(valid_pos, 1)[0]
            assert size == 1
            return np.array([a[self.sequential.bounded(len(a))]])
        assert size is None                                  # the shift of sim_signals
        return a[self.stream.bounded(0, len(a))]

    def shuffle(self, x):
        assert self.stream is None
        for i in range(len(x) - 1, 0, -1):
            j = self.sequential.bounded(i + 1)
            x[i], x[j] = x[j], x[i]


def make_model(rng):
    """The k-mers over A C T and those with one X or Y among them: means 60 .. 120 (a few of mixed sign: shifted by -90),
    stdvs 0.8 .. 3.5, some exactly 0."""
    kmers = []
    for t in range(3 ** 6):
        kmers.append("".join("ACT"[t // 3 ** q % 3] for q in range(6)))
    for k in list(kmers):
        for q in range(6):
            for ub in "XY":
                kmers.append(k[:q] + ub + k[q + 1:])
    kmers = sorted(set(kmers))
    mean = np.round(rng.uniform(60.0, 120.0, len(kmers)), 6)
    stdv = np.round(rng.uniform(0.8, 3.5, len(kmers)), 6)
    return kmers, mean, stdv


def make_dna(rng):
    """30 chunks of 24 .. 60 bases with naive breakpoints; chunks 3, 11, 27 carry an UB already, chunk 19 has 18 bases, chunk 7
    ends with A."""
    n = N_CHUNKS
    chunks = (rng.standard_normal((n, N_SAMPLES)) * 1.2).astype(np.float16)
    targets = np.zeros((n, LT), np.uint8)
    lengths = rng.integers(24, 61, n).astype(np.uint16)
    lengths[19] = 18
    lengths[3], lengths[11], lengths[27] = 50, 33, 60
    bkps = np.zeros((n, LT), np.uint16)
    for c in range(n):
        L = int(lengths[c])
        targets[c, :L] = rng.integers(1, 3, L)
        reps = np.full(L, N_SAMPLES // L)
        reps[:N_SAMPLES % L] += 1
        bkps[c, :L] = np.cumsum(rng.permutation(reps))
    targets[3, 20], targets[11, 12], targets[27, 30], targets[27, 45] = 5, 6, 5, 6
    targets[7, int(lengths[7]) - 1], targets[8, int(lengths[8]) - 1] = 1, 2
    return chunks, targets, lengths, bkps


def main():
    ref = load_reference()
    rng = np.random.default_rng(20122)
    kmers, mean, stdv = make_model(rng)
    dna = make_dna(rng)
    poremodel = {k: [float(m), float(s)] for k, m, s in zip(kmers, mean, stdv)}
    table = sk.model_table({k: (m, s) for k, (m, s) in poremodel.items()})
    arrays = {"model_index": np.array([sk.kmer_index(k) for k in kmers], np.int32), "model_mean": mean, "model_stdv": stdv,
              "dna_chunks": dna[0], "dna_targets": dna[1], "dna_lengths": dna[2], "dna_bkps": dna[3]}
    meta = {"note": "inputs: synthetic two-letter ctc-data and a synthetic k-mer model; outputs: what ub-bonito/bonito/spike_chunks.py "
                    "computed from them with tests/spike_ref.py's draws replayed through its generator (seed %d)" % SEED,
            "seed": SEED, "cases": []}

    seen = {}
    real_med, real_sim, real_chunk = ref.compute_med_mad_squiggly, ref.sim_signals, ref.spike_chunk

    def med_mad(means, stds, rng=None, **kw):
        rng.begin(1)
        seen["med"], seen["mad"] = real_med(means, stds, rng=rng, **kw)
        return seen["med"], seen["mad"]

    def sim_signals(seq, kmer_reps, model, rng=None, **kw):
        rng.begin(2 + seen["calls"])
        seen["calls"] += 1
        return real_sim(seq, kmer_reps, model, rng=rng, **kw)

    def spike_chunk(chunk, length, target, breakpts, spiked_pos_ubs, *args, **kw):
        seen["positions"] = [int(p) for p in spiked_pos_ubs]
        seen["ubs"] = [ref.BASE_MAP.index(u) if u != "N" else 0 for u in spiked_pos_ubs.values()]
        return real_chunk(chunk, length, target, breakpts, spiked_pos_ubs, *args, **kw)

    ref.compute_med_mad_squiggly, ref.sim_signals, ref.spike_chunk = med_mad, sim_signals, spike_chunk
    chunks32 = dna[0].astype(np.float32)
    for name, ubs, prop, var, pad, std_dist, noise_std, variable in CASES:
        out = np.empty_like(chunks32)
        out_t = np.empty_like(dna[1])
        med, mad = np.zeros(N_CHUNKS), np.zeros(N_CHUNKS)
        positions, letters = [], []
        dist_rows, phi = sk.phi_table(std_dist)
        differing, worst = 0, 0
        for c in range(N_CHUNKS):
            seen.update(calls=0)
            out[c], out_t[c] = ref.spike_read(chunks32[c], int(dna[2][c]), dna[1][c], dna[3][c].astype(int), prop, list(ubs), poremodel,
                                              var_prop_ubs=var, rng=Replay(SEED, c), pad=pad, equal_kmer_reps=False, std_dist=std_dist,
                                              noise_std=noise_std, variable_noise=variable)
            med[c], mad[c] = seen["med"], seen["mad"]
            positions.append(seen["positions"])
            letters.append(seen["ubs"])
            assert seen["calls"] == len(seen["positions"])
            mine = spike_ref.spike_chunk(chunks32[c], dna[1][c], int(dna[2][c]), dna[3][c], table, c, SEED, sk.ubs_mask(ubs), prop, var,
                                         pad, dist_rows, phi, noise_std, variable)
            steps = np.abs(mine[0].view(np.int32).astype(np.int64) - out[c].view(np.int32).astype(np.int64))
            differing += int((steps > 0).sum())
            worst = max(worst, int(steps.max()))
        assert out.dtype == np.float32
        arrays["out_%s_xor" % name] = out.view(np.uint32) ^ chunks32.view(np.uint32)     # zero wherever nothing was pasted
        arrays["out_%s_targets" % name] = out_t
        arrays["out_%s_med" % name] = med
        arrays["out_%s_mad" % name] = mad
        meta["cases"].append(dict(name=name, ubs=ubs, prop_ubs=prop, var_prop_ubs=var, pad=pad, std_dist=std_dist, noise_std=noise_std,
                                  variable_noise=variable, positions=positions, position_ubs=letters,
                                  spiked=int(sum(len(p) for p in positions)), exact=std_dist == "uniform" and noise_std == 0,
                                  values_differing_from_restatement=differing, largest_difference_in_float32_steps=worst))
        print(name, "positions", meta["cases"][-1]["spiked"], "differing", differing, "worst", worst)
    ref.compute_med_mad_squiggly, ref.sim_signals, ref.spike_chunk = real_med, real_sim, real_chunk

    first = meta["cases"][0]
    assert first["spiked"] >= N_CHUNKS and not first["positions"][19], first["spiked"]
    assert all(c["largest_difference_in_float32_steps"] <= 1 for c in meta["cases"]), "more than a float32 step"
    assert all(c["values_differing_from_restatement"] == 0 for c in meta["cases"] if c["exact"])
    assert any(6 in u and 5 in u for u in first["position_ubs"])

    write_npz(os.path.join(HERE, "spike.npz"), arrays)
    with open(os.path.join(HERE, "spike.json"), "w") as fh:
        json.dump(meta, fh, indent=None, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
