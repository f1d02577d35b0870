"""Inputs shared by the spike tests: the golden fixture (tests/golden/spike.npz / .json, written by
tests/golden/make_spike_golden.py from the reference's spike_chunks.py), seeded random chunks and the named edge chunks."""
import functools
import json
import os
import types

import numpy as np

import spike_ref
from conftest import GOLDEN
from xna_basecaller_amd import spike as sk

STD_DISTS = ("uniform", "truncnorm", "truncnorm_shift_1.5_0.5")


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(GOLDEN, "spike.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "spike.json")))
    return {k: z[k] for k in z.files}, meta


@functools.lru_cache(maxsize=None)
def model():
    """The fixture's k-mer model as (mean, stdv) of 7^6 k-mers."""
    z, _ = golden()
    mean, stdv = np.full(sk.MODEL_KMERS, np.nan), np.zeros(sk.MODEL_KMERS)
    mean[z["model_index"]], stdv[z["model_index"]] = z["model_mean"], z["model_stdv"]
    return mean, stdv


@functools.lru_cache(maxsize=None)
def edge_model(which):
    """'ties': every third k-mer has stdv 0 (hundreds of equal squiggle values); 'signs': the means are shifted to straddle
    0 (negative and mixed-sign keys of the selection)."""
    mean, stdv = (a.copy() for a in model())
    have = np.flatnonzero(~np.isnan(mean))
    if which == "ties":
        stdv[have[::3]] = 0.0
        mean[have] = np.round(mean[have])                # and equal means across k-mers
    else:
        mean[have] -= 90.0
    return mean, stdv


def dna():
    z, _ = golden()
    return z["dna_chunks"].astype(np.float32), z["dna_targets"], z["dna_lengths"].astype(np.int32), z["dna_bkps"]


def case_args(case):
    """A case of the fixture as the keyword arguments of Context.spike_chunks / spike_ref.spike_batch's run."""
    rows, phi = sk.phi_table(case["std_dist"])
    return dict(ubs_mask=sk.ubs_mask(case["ubs"]), prop=case["prop_ubs"], var_prop=case["var_prop_ubs"] or 0.0, pad=case["pad"],
                dist_rows=rows, phi=phi, noise_std=case["noise_std"], variable_noise=case["variable_noise"])


def dist_args(std_dist, noise_std=0.0, variable_noise=False):
    rows, phi = sk.phi_table(std_dist)
    return dict(dist_rows=rows, phi=phi, noise_std=noise_std, variable_noise=variable_noise)


def expected(case):
    """The reference's (chunks float32, targets, spiked, med, mad) of a case."""
    z, _ = golden()
    chunks = (z["dna_chunks"].astype(np.float32).view(np.uint32) ^ z["out_%s_xor" % case["name"]]).view(np.float32)
    spiked = np.array([len(p) for p in case["positions"]], np.int32)
    return chunks, z["out_%s_targets" % case["name"]], spiked, z["out_%s_med" % case["name"]], z["out_%s_mad" % case["name"]]


def random_set(seed, n, N):
    """splice_cases.random_set's chunks over the fixture model's letters: n chunks of N samples, lengths from 12 (too short for
    a position) up to N / 2, random breakpoints, a few existing unnatural bases."""
    rng = np.random.default_rng(seed)
    Lt = max(16, -(-(N // 2) // 16) * 16) if N % 3 else N // 2 + 1     # rows the 16-byte copy takes, and rows it does not
    chunks = (rng.standard_normal((n, N)) * 1.3).astype(np.float32)
    targets = np.zeros((n, Lt), np.uint8)
    lengths = np.zeros(n, np.int32)
    bkps = np.zeros((n, Lt), np.uint16)
    for c in range(n):
        L = int(rng.integers(12, max(13, min(Lt, N // 2)) + 1))
        lengths[c] = L
        targets[c, :L] = rng.integers(1, 3, L)
        if c % 7 == 3 and L > 30:
            targets[c, rng.integers(0, L)] = 5 + c % 2
        cuts = np.sort(rng.choice(np.arange(1, N), size=L - 1, replace=False))
        bkps[c, :L - 1] = cuts
        bkps[c, L - 1] = N if c % 2 else rng.integers(cuts[-1] + 1, N + 1)
    return chunks, targets, lengths, bkps


def one_chunk(seed, L, N, Lt=None, last=None):
    """One chunk of L bases (labels 1, 2) with random non-empty bases over N samples."""
    rng = np.random.default_rng(seed)
    Lt = L + 3 if Lt is None else Lt
    targets = np.zeros((1, Lt), np.uint8)
    targets[0, :L] = rng.integers(1, 3, L)
    if last is not None:
        targets[0, L - 1] = last
    bkps = np.zeros((1, Lt), np.uint16)
    bkps[0, :L - 1] = np.sort(rng.choice(np.arange(1, N), size=L - 1, replace=False))
    bkps[0, L - 1] = N
    return (rng.standard_normal((1, N)) * 1.3).astype(np.float32), targets, np.array([L], np.int32), bkps


def reference(data, mdl, first_index, seed, kw, stats=None):
    """spike_ref over a set -> the tuple Context.spike_chunks returns."""
    n = data[0].shape[0]
    out = [spike_ref.spike_chunk(data[0][c], data[1][c], data[2][c], data[3][c], mdl, first_index + c, seed, kw["ubs_mask"], kw["prop"],
                                 kw.get("var_prop", 0.0), kw.get("pad", 5), kw.get("dist_rows", 0), kw.get("phi", np.zeros((1, 2))),
                                 kw.get("noise_std", 0.0), kw.get("variable_noise", False), stats=stats) for c in range(n)]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out], np.int32),
            np.array([o[3] for o in out], np.float64), np.array([o[4] for o in out], np.float64), np.array([o[5] for o in out], np.int8))


def namespace(**kw):
    base = dict(ubs="XY", prop_ubs=0.1, var_prop_ubs=None, ub_pad=5, std_dist="uniform", noise_std=0, variable_noise=False, seed=2012,
                batchsize=4096, device="cuda", overwrite=False, fully_synth=False, equal_kmer_reps=False, legacy_pos=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def write_model(path):
    """The fixture's model as the tab-separated file the tools read."""
    z, _ = golden()
    with open(path, "w") as fh:
        fh.write("kmer\tlevel_mean\tlevel_stdv\tsd_mean\tsd_stdv\tweight\n")
        for t, m, s in zip(z["model_index"], z["model_mean"], z["model_stdv"]):
            fh.write("%s\t%r\t%r\t0.0\t0.0\t0.0\n" % (sk.index_kmer(t), float(m), float(s)))
    return path


def write_dir(tmp_path, name="dna"):
    """The fixture's DNA set as a ctc-data directory (chunks float16, as the tools write them)."""
    z, _ = golden()
    d = tmp_path / name
    d.mkdir()
    for f, key in zip(sk.FILES, ("chunks", "targets", "lengths", "bkps")):
        np.save(str(d / f), z["dna_%s" % key])
    return str(d)
