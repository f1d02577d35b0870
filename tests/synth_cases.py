"""Inputs shared by the synth tests: the golden fixture (tests/golden/synth.npz / .json, written by
tests/golden/make_synth_golden.py from the reference's spike_chunks.py with fully_synth=True on the spike fixture's inputs);
the inputs, the model, the random sets and the edge chunks are spike_cases'."""
import functools
import json
import os
import types

import numpy as np

import spike_cases
import synth_ref
from conftest import GOLDEN
from spike_cases import STD_DISTS, case_args, dist_args, dna, edge_model, model, one_chunk, random_set, write_dir, write_model  # noqa: F401

PAD3 = "one_x_pad3"                                      # the case where the reference raises: two UBs in one k-mer


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(GOLDEN, "synth.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "synth.json")))
    return {k: z[k] for k in z.files}, meta


def raised(case):
    """{chunk: the k-mer the reference's KeyError named}."""
    return {int(c): k for c, k in case["raised"].items()}


def expected(case):
    """The reference's (chunks float32, targets, spiked, med, mad, status) of a case; a chunk where it raised is the input with
    spiked 0, med and mad NaN, status 2."""
    z, _ = golden()
    inputs = spike_cases.golden()[0]["dna_chunks"].astype(np.float32)
    chunks = (inputs.view(np.uint32) ^ z["out_%s_xor" % case["name"]]).view(np.float32)
    bad = raised(case)
    spiked = np.array([0 if c in bad else len(p) for c, p in enumerate(case["positions"])], np.int32)
    status = np.array([2 if c in bad else 0 for c in range(len(spiked))], np.int8)
    return chunks, z["out_%s_targets" % case["name"]], spiked, z["out_%s_med" % case["name"]], z["out_%s_mad" % case["name"]], status


def reference(data, mdl, first_index, seed, kw, stats=None):
    """synth_ref over a set -> the tuple Context.synth_chunks returns."""
    n = data[0].shape[0]
    out = [synth_ref.synth_chunk(data[0][c], data[1][c], data[2][c], data[3][c], mdl, first_index + c, seed, kw["ubs_mask"], kw["prop"],
                                 kw.get("var_prop", 0.0), kw.get("pad", 5), kw.get("dist_rows", 0), kw.get("phi", np.zeros((1, 2))),
                                 kw.get("noise_std", 0.0), kw.get("variable_noise", False), stats=stats) for c in range(n)]
    return (np.array([o[0] for o in out]), np.array([o[1] for o in out]), np.array([o[2] for o in out], np.int32),
            np.array([o[3] for o in out], np.float64), np.array([o[4] for o in out], np.float64), np.array([o[5] for o in out], np.int8))


@functools.lru_cache(maxsize=None)
def golden_reference(index):
    """The restatement on a case of the fixture, computed once (read-only)."""
    _, meta = golden()
    stats = {}
    got = reference(dna(), model(), 0, meta["seed"], case_args(meta["cases"][index]), stats=stats)
    for a in got:
        a.setflags(write=False)
    return got, stats


def namespace(**kw):
    base = dict(ubs="XY", prop_ubs=0.1, var_prop_ubs=None, ub_pad=5, std_dist="uniform", noise_std=0, variable_noise=False, seed=2012,
                batchsize=4096, device="cuda", overwrite=False, equal_kmer_reps=False, legacy_pos=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def same(got, want, what=""):
    """Two result tuples are equal bit for bit: status, spiked, the bit patterns of med and mad (NaN equals NaN), labels, and
    the signal as uint32."""
    assert np.array_equal(got[5], want[5]), (what, "status", np.flatnonzero(got[5] != want[5])[:5])
    assert np.array_equal(got[2], want[2]), (what, "spiked", np.flatnonzero(got[2] != want[2])[:5])
    for k, name in ((3, "med"), (4, "mad")):
        a, b = np.asarray(got[k], np.float64).view(np.uint64), np.asarray(want[k], np.float64).view(np.uint64)
        nan = np.isnan(got[k]) & np.isnan(want[k])
        assert np.array_equal(a[~nan], b[~nan]) and np.array_equal(np.isnan(got[k]), np.isnan(want[k])), \
            (what, name, np.flatnonzero(a != b)[:5], got[k][:3], want[k][:3])
    bad = np.flatnonzero((got[1] != want[1]).any(axis=1))
    assert bad.size == 0, (what, "targets", bad[:5])
    bad = np.flatnonzero((np.asarray(got[0], np.float32).view(np.uint32) != np.asarray(want[0], np.float32).view(np.uint32)).any(axis=1))
    assert bad.size == 0, (what, "signal", bad[:5], [np.flatnonzero(got[0][b] != want[0][b])[:8] for b in bad[:2]])
