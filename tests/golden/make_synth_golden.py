"""Regenerates tests/golden/synth.npz and synth.json: what the reference's fully synthetic mode -- spike_read(...,
fully_synth=True) -> sim_target -> sim_signals(append=True), ub-bonito/bonito/spike_chunks.py:217-297 -- computes on the
inputs of the spike fixture (tests/golden/spike.npz: its DNA set and its k-mer model), with the contract's draws
(tests/spike_ref.py: Sequential, Stream) replayed through its random generator, for the seven cases of make_spike_golden.py.

Run in the BUILD container only.  It imports, BY FILE PATH and as reference code, ub-bonito/bonito/spike_chunks.py (numpy,
pandas and scipy are all it needs) and runs spike_read with fully_synth=True, equal_kmer_reps=False.  Only DATA is stored: the
reference's chunks (xor against the input), labels, positions, unnatural bases, med and mad, and for the chunks where the
reference raises KeyError -- a spiked row that holds a k-mer no model has: pad 3 puts two unnatural bases into one k-mer --
which chunks they are and the k-mer it names.  The inputs are not stored again.

The generator is make_spike_golden.py's Replay: stream 0 in spike_read and choose_positions, stream 1 in
compute_med_mad_squiggly, stream 2 in the one call of sim_signals (the shift choice is draw 0, the scalar uniform of the
variable noise draw 1, the first array of uniforms draws 2 .., the second 2 + total ..).  scipy's truncnorm.rvs applies its own
ppf to those uniforms; the restatement's (AS241) may differ from it in the last bits of float64, which float32 rounding can
show as one step: the json records per case how many values differ at all.

Both files are byte-for-byte reproducible (the archive's time stamps are fixed).
"""
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import synth_ref  # noqa: E402
from make_spike_golden import CASES, N_CHUNKS, SEED, Replay, load_reference  # noqa: E402
from make_splice_golden import write_npz  # noqa: E402
from xna_basecaller_amd import spike as sk  # noqa: E402


class Recording(Replay):
    """Replay that keeps what spike_read shuffled: its list of unnatural bases."""

    shuffled = None

    def shuffle(self, x):
        super().shuffle(x)
        self.shuffled = list(x)


def main():
    ref = load_reference()
    z = np.load(os.path.join(HERE, "spike.npz"))
    kmers = [sk.index_kmer(t) for t in z["model_index"]]
    poremodel = {k: [float(m), float(s)] for k, m, s in zip(kmers, z["model_mean"], z["model_stdv"])}
    table = sk.model_table({k: (m, s) for k, (m, s) in poremodel.items()})
    chunks32 = z["dna_chunks"].astype(np.float32)
    targets, lengths, bkps = z["dna_targets"], z["dna_lengths"], z["dna_bkps"]
    assert chunks32.shape[0] == N_CHUNKS
    arrays = {}
    meta = {"note": "inputs: the DNA set and the k-mer model of tests/golden/spike.npz; outputs: what ub-bonito/bonito/spike_chunks.py "
                    "computed from them with fully_synth=True and tests/spike_ref.py's draws replayed through its generator (seed %d)" % SEED,
            "seed": SEED, "cases": []}

    seen = {}
    real_med, real_sim, real_choose = ref.compute_med_mad_squiggly, ref.sim_signals, ref.choose_positions

    def med_mad(means, stds, rng=None, **kw):
        rng.begin(1)
        seen["med"], seen["mad"] = real_med(means, stds, rng=rng, **kw)
        return seen["med"], seen["mad"]

    def sim_signals(seq, kmer_reps, model, rng=None, **kw):
        rng.begin(2 + seen["calls"])
        seen["calls"] += 1
        return real_sim(seq, kmer_reps, model, rng=rng, **kw)

    def choose_positions(*args, **kw):
        seen["positions"] = [int(p) for p in real_choose(*args, **kw)]
        return list(seen["positions"])

    ref.compute_med_mad_squiggly, ref.sim_signals, ref.choose_positions = med_mad, sim_signals, choose_positions
    for name, ubs, prop, var, pad, std_dist, noise_std, variable in CASES:
        out = chunks32.copy()
        out_t = targets.copy()
        med, mad = np.full(N_CHUNKS, np.nan), np.full(N_CHUNKS, np.nan)
        positions, letters, raised = [], [], {}
        dist_rows, phi = sk.phi_table(std_dist)
        differing, worst, synthesised = 0, 0, 0
        for c in range(N_CHUNKS):
            seen.update(calls=0, med=None, mad=None)
            rng = Recording(SEED, c)
            L = int(lengths[c])
            mine = synth_ref.synth_chunk(chunks32[c], targets[c], L, bkps[c], table, c, SEED, sk.ubs_mask(ubs), prop, var, pad,
                                         dist_rows, phi, noise_std, variable)
            try:
                got = ref.spike_read(chunks32[c], L, targets[c], bkps[c].astype(int), prop, list(ubs), poremodel, var_prop_ubs=var,
                                     fully_synth=True, rng=rng, pad=pad, equal_kmer_reps=False, std_dist=std_dist,
                                     noise_std=noise_std, variable_noise=variable)
            except KeyError as e:
                raised[str(c)] = str(e.args[0])
                got = None
            n = len(seen["positions"])
            positions.append(seen["positions"])
            if ubs == "N":
                letters.append([0] * n)
            elif len(ubs) == 1:
                letters.append([ref.BASE_MAP.index(ubs)] * n)
            else:
                letters.append([ref.BASE_MAP.index(u) for u in rng.shuffled[:n]] if n else [])
            if got is None:
                assert mine[5] == 2 and sk.index_kmer(mine[3]) == raised[str(c)], (name, c)
                continue
            assert seen["calls"] == 1 and got[0].dtype == np.float32 and len(got[0]) == int(bkps[c][L - 1]) == out.shape[1]
            out[c], out_t[c] = got
            med[c], mad[c] = seen["med"], seen["mad"]
            steps = np.abs(mine[0].view(np.int32).astype(np.int64) - out[c].view(np.int32).astype(np.int64))
            differing += int((steps > 0).sum())
            worst = max(worst, int(steps.max()))
            synthesised += len(got[0])
            assert mine[5] == 0 and mine[3] == med[c] and mine[4] == mad[c] and np.array_equal(mine[1], out_t[c]), (name, c)
        arrays["out_%s_xor" % name] = out.view(np.uint32) ^ chunks32.view(np.uint32)      # zero in the chunks that raised
        arrays["out_%s_targets" % name] = out_t
        arrays["out_%s_med" % name] = med
        arrays["out_%s_mad" % name] = mad
        meta["cases"].append(dict(name=name, ubs=ubs, prop_ubs=prop, var_prop_ubs=var, pad=pad, std_dist=std_dist, noise_std=noise_std,
                                  variable_noise=variable, positions=positions, position_ubs=letters, raised=raised,
                                  spiked=int(sum(len(p) for c, p in enumerate(positions) if str(c) not in raised)),
                                  exact=std_dist == "uniform" and noise_std == 0, values_synthesised=synthesised,
                                  values_differing_from_restatement=differing, largest_difference_in_float32_steps=worst))
        print(name, "positions", meta["cases"][-1]["spiked"], "raised", len(raised), "differing", differing, "worst", worst)
    ref.compute_med_mad_squiggly, ref.sim_signals, ref.choose_positions = real_med, real_sim, real_choose

    by = {c["name"]: c for c in meta["cases"]}
    assert all(c["largest_difference_in_float32_steps"] <= 1 for c in meta["cases"]), "more than a float32 step"
    assert all(c["values_differing_from_restatement"] == 0 for c in meta["cases"] if c["exact"])
    assert all(not c["raised"] for c in meta["cases"] if c["pad"] == 5) and len(by["one_x_pad3"]["raised"]) > 10
    assert not by["uniform_xy"]["positions"][19]                       # 18 bases: no position, synthesised all the same

    write_npz(os.path.join(HERE, "synth.npz"), arrays)
    with open(os.path.join(HERE, "synth.json"), "w") as fh:
        json.dump(meta, fh, indent=None, sort_keys=True)
        fh.write("\n")


if __name__ == "__main__":
    main()
