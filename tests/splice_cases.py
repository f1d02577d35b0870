"""Inputs shared by the splice tests: the golden fixture (tests/golden/splice.npz / .json, written by
tests/golden/make_splice_golden.py from the reference's stitch_chunks.py) and seeded random chunks."""
import functools
import json
import os
import types

import numpy as np

from conftest import GOLDEN
from xna_basecaller_amd import splice as sp


@functools.lru_cache(maxsize=None)
def golden():
    z = np.load(os.path.join(GOLDEN, "splice.npz"))
    meta = json.load(open(os.path.join(GOLDEN, "splice.json")))
    return {k: z[k] for k in z.files}, meta


def xna(which="full"):
    z, _ = golden()
    keep = np.ones(len(z["xna_lengths"]), bool) if which == "full" else z["xna_holes_keep"]
    # dropped reads lose their unnatural base instead of their row, so that read_idx stays the full set's
    targets = z["xna_targets"].copy()
    targets[~keep] = np.where(targets[~keep] > 4, 1, targets[~keep])
    return z["xna_chunks"], targets, z["xna_lengths"], z["xna_bkps"]


@functools.lru_cache(maxsize=None)
def library(which="full"):
    return sp.build_library(*xna(which))


def dna():
    z, _ = golden()
    return z["dna_chunks"].astype(np.float32), z["dna_targets"], z["dna_lengths"].astype(np.int32), z["dna_bkps"]


def case_args(case):
    """A case of the fixture as the keyword arguments of splice_ref.splice_chunk / Context.splice_chunks."""
    return dict(ubs_mask=sp.ubs_mask(case["ubs"]), prop=case["prop_ubs"], var_prop=case["var_prop_ubs"] or 0.0,
                cand_sample_size=case["cand_sample_size"], pad=case["pad"])


def expected(case):
    """The reference's (chunks float32, targets, success) of a case."""
    z, _ = golden()
    chunks = (z["dna_chunks"].astype(np.float32).view(np.uint32) ^ z["out_%s_xor" % case["name"]]).view(np.float32)
    return chunks, z["out_%s_targets" % case["name"]], z["out_%s_success" % case["name"]]


def info_rows(lib):
    """Library.info as the fixture stores the reference's frame: integers, letters as base-7 numbers."""
    def b7(s):
        t = 0
        for ch in s:
            t = t * 7 + sp.BASE_MAP.index(ch)
        return t
    return np.array([(sp.BASE_MAP.index(ub), b7(tpl), kpos, b7(kmer), read, st, en) for ub, tpl, kpos, kmer, read, st, en in lib.info],
                    dtype=np.int32).reshape(-1, 7)


def random_set(seed, n, N, four_letters=False):
    """n chunks of N samples: lengths from too short for a position up to what N carries at 2+ samples per base, random
    breakpoints, a few existing unnatural bases; two letters (every group of the full library exists) or four (most
    positions are abandoned)."""
    rng = np.random.default_rng(seed)
    Lt = max(16, -(-(N // 2) // 16) * 16) if N % 3 else N // 2 + 1     # rows the 16-byte copy takes, and rows it does not
    chunks = (rng.standard_normal((n, N)) * 1.3).astype(np.float32)
    targets = np.zeros((n, Lt), np.uint8)
    lengths = np.zeros(n, np.int32)
    bkps = np.zeros((n, Lt), np.uint16)
    for c in range(n):
        L = int(rng.integers(12, max(13, min(Lt, N // 2)) + 1))
        lengths[c] = L
        targets[c, :L] = rng.integers(1, 5 if four_letters else 3, L)
        if c % 7 == 3 and L > 30:
            targets[c, rng.integers(0, L)] = 5 + c % 2
        cuts = np.sort(rng.choice(np.arange(1, N), size=L - 1, replace=False))
        bkps[c, :L - 1] = cuts
        bkps[c, L - 1] = N if c % 2 else rng.integers(cuts[-1] + 1, N + 1)
    return chunks, targets, lengths, bkps


def namespace(**kw):
    base = dict(ubs="XY", prop_ubs=0.1, var_prop_ubs=None, stitch_mode="per_kmer", cand_sample_size=10, ub_pad=5, seed=2012,
                batchsize=4096, device="cuda", overwrite=False, weighted_pos_pick=False, stitch_noise_std=0, permute_win_size=0,
                spike=False)
    base.update(kw)
    return types.SimpleNamespace(**base)


def write_dirs(tmp_path):
    """The fixture's DNA and XNA sets as ctc-data directories (chunks float16, as the tools write them)."""
    z, _ = golden()
    for name, prefix in (("dna", "dna"), ("xna", "xna")):
        d = tmp_path / name
        d.mkdir()
        for f, key in zip(sp.FILES, ("chunks", "targets", "lengths", "bkps")):
            np.save(str(d / f), z["%s_%s" % (prefix, key)])
    return str(tmp_path / "dna"), str(tmp_path / "xna")
