"""CPU: the host side of `splice` (xna_basecaller_amd/splice.py, cli/splice.py) and the restatement of the device contract
(tests/splice_ref.py) against what the reference's ub-bonito/bonito/stitch_chunks.py computed (tests/golden/splice.npz / .json,
written by tests/golden/make_splice_golden.py): library rows and order, pasted chunks bit for bit, labels, success flags."""
import os

import numpy as np
import pytest

import splice_cases as cases
import splice_ref
from xna_basecaller_amd import splice as sp
from xna_basecaller_amd.cli import splice as cli


def test_fixture_exercises_the_paths():
    """Asserted from the stored data, as the generator asserts it: a fixture that exercises nothing cannot pass."""
    z, meta = cases.golden()
    by_name = {c["name"]: c for c in meta["cases"]}
    n = len(z["dna_lengths"])
    first = by_name["xy_cand5"]
    assert z["out_xy_cand5_success"].sum() == first["succeeded"] >= 0.9 * n
    assert first["stretch"] >= 10 and first["shrink"] >= 10
    assert by_name["holes_xy_var"]["abandoned"] >= 1
    for c in meta["cases"]:
        _, targets, ok = cases.expected(c)
        changed = targets != z["dna_targets"]
        assert changed.sum() == c["inserted"] == c["stretch"] + c["shrink"] + c["copy"]
        assert np.array_equal(changed.any(axis=1), ok)
        assert set(np.unique(targets[changed])) <= {5 + "XY".index(u) for u in c["ubs"]}
        assert c["positions"] - c["inserted"] == c["abandoned"]
    assert (z["dna_targets"] > 4).any(axis=1).sum() == 3 and (z["dna_lengths"] < 21).sum() == 1
    assert not z["out_xy_cand5_success"][z["dna_lengths"] < 21].any()
    assert {c["cand_sample_size"] for c in meta["cases"]} == {1, 5, 32}
    assert any(c["var_prop_ubs"] for c in meta["cases"]) and any(not c["var_prop_ubs"] for c in meta["cases"])
    assert int(cases.library("full").table[:, 1].max()) < 32           # 32 candidates are more than any group holds
    assert ((z["xna_targets"] > 4).sum(axis=1) == 0).sum() == 1         # a library read without an unnatural base


@pytest.mark.parametrize("which", ["full", "holes"])
def test_build_library_equals_the_reference_rows(which):
    z, _ = cases.golden()
    lib = cases.library(which)
    want = z["lib_%s_rows" % which]
    assert np.array_equal(cases.info_rows(lib), want)
    # the device arrays say the same: lengths, the pool's samples, groups keyed without the k-mer
    assert np.array_equal(lib.rows[:, 1], want[:, 6] - want[:, 5])
    chunks = z["xna_chunks"]
    for r in (0, 1, len(want) // 2, len(want) - 1):
        off, n = lib.rows[r]
        assert np.array_equal(lib.pool[off:off + n], chunks[want[r, 4], want[r, 5]:want[r, 6]])
    keys = want[:, 0].astype(np.int64) * 10 ** 7 + want[:, 1] * 10 + want[:, 2]
    groups, first, count = np.unique(keys, return_index=True, return_counts=True)
    filled = np.flatnonzero(lib.table[:, 1])
    assert len(filled) == len(groups) == (384 if which == "full" else 288)
    assert np.array_equal(lib.table[filled, 0], first) and np.array_equal(lib.table[filled, 1], count)
    for g, r in zip(filled[:50], first[:50]):
        assert g == sp.table_index(want[r, 0], [want[r, 1] // 7 ** (4 - q) % 7 for q in range(5)], want[r, 2])
    assert any(len(set(want[f:f + c, 3])) > 1 for f, c in zip(first, count))      # a group with different k-mers


def test_library_drops_what_slice_xna_drops():
    z, _ = cases.golden()
    lib = cases.library("full")
    kept = set(r[4] for r in lib.info)
    assert len(kept) == 268 and len(z["xna_lengths"]) == 272
    for read in set(range(272)) - kept:
        t, L = z["xna_targets"][read], int(z["xna_lengths"][read])
        ubs = np.flatnonzero(t[:L] > 4)
        b = z["xna_bkps"][read].astype(int)
        assert ubs.size == 0 or not 5 < ubs[0] < L - 5 or np.diff(b[ubs[0] - 6:ubs[0] + 1]).max() > 100


@pytest.mark.parametrize("index", range(4))
def test_splice_ref_equals_the_reference(index):
    _, meta = cases.golden()
    case = meta["cases"][index]
    chunks, targets, lengths, bkps = cases.dna()
    want = cases.expected(case)
    lib = cases.library(case["library"])
    args = cases.case_args(case)
    ubs = [u for u in (5, 6) if args["ubs_mask"] >> (u - 5) & 1]
    stats = {}
    for c in range(len(lengths)):
        got = splice_ref.splice_chunk(chunks[c], targets[c], lengths[c], bkps[c], lib, c, meta["seed"], ubs, args["prop"],
                                      args["var_prop"], args["cand_sample_size"], args["pad"], stats=stats)
        assert np.array_equal(got[0].view(np.uint32), want[0][c].view(np.uint32)), c
        assert np.array_equal(got[1], want[1][c]) and got[2] == want[2][c], c
        assert got[3] == (want[1][c] != targets[c]).sum()
    assert stats == {k: case[k] for k in ("positions", "stretch", "shrink", "copy", "abandoned")}


def test_prepare_equals_the_reference():
    _, meta = cases.golden()
    kinds = set()
    for p in meta["prepare"]:
        got, kind = splice_ref.prepare(p["values"], p["ins_len"], p["kmer_cnts"])
        assert got == p["out"], (p["kmer_cnts"], p["ins_len"])
        kinds.add((kind, abs(len(p["values"]) - p["ins_len"]) == 1, max(p["kmer_cnts"]) == 1))
    assert {("stretch", True, True), ("shrink", True, True), ("stretch", True, False), ("shrink", True, False),
            ("copy", False, True)} <= kinds


def test_interp_with_repeated_points_is_numpys():
    """The largest j with xp[j] <= x.  (prepare_slice_chunk itself cannot produce repeated xp while every k-mer has a
    sample -- tests/golden/make_splice_golden.py says why -- so numpy is asked directly.)"""
    rng = np.random.default_rng(4)
    for _ in range(200):
        n_out = int(rng.integers(2, 40))
        inner = np.sort(rng.integers(0, n_out, int(rng.integers(0, 30))))
        xp = np.concatenate([[0], inner, [n_out - 1]])
        fp = rng.standard_normal(len(xp)).astype(np.float16)
        want = np.interp(np.arange(n_out), xp, fp)
        got = np.array(splice_ref.interp(n_out, [int(v) for v in xp], [float(v) for v in fp]))
        assert np.array_equal(got.view(np.uint64), want.view(np.uint64)), (xp, fp)


def test_draws():
    """The contract's stream written out once more, independently of splice_ref.mix."""
    M = (1 << 64) - 1

    def fin(z):
        z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M
        z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M
        return z ^ (z >> 31)
    G = 0x9E3779B97F4A7C15
    d = splice_ref.Draws(2012, 7)
    zs = [fin((fin((2012 + G * 8) & M) + G * (k + 1)) & M) for k in range(3)]
    assert d.bounded(1000) == ((zs[0] >> 32) * 1000) >> 32
    assert d.unit() == (zs[1] >> 11) * 2.0 ** -53 and 0.0 <= (zs[1] >> 11) * 2.0 ** -53 < 1.0
    assert d.choice(["X", "Y"]) == "XY"[((zs[2] >> 32) * 2) >> 32]
    picks = splice_ref.Draws(1, 1).choice(5, size=5, replace=False)
    assert sorted(picks) == [0, 1, 2, 3, 4]
    assert splice_ref.Draws(1, 1).k == 0 and len(splice_ref.Draws(3, 0).choice(9, size=4, replace=False)) == 4
    assert fin(0) == 0 and splice_ref.mix(1) == fin(1) == 0x5692161D100B05E5


def test_batches_do_not_change_the_result():
    _, meta = cases.golden()
    lib = cases.library("full")
    chunks, targets, lengths, bkps = (a[:12] for a in cases.dna())
    kw = dict(ubs="XY", prop_ubs=0.1, var_prop_ubs=0.04, cand_sample_size=3, run=splice_ref.splice_batch(lib))
    whole = sp.splice(chunks, targets, lengths, bkps, lib, batch=4096, **kw)
    split = sp.splice(chunks, targets, lengths, bkps, lib, batch=5, **kw)
    for a, b in zip(whole, split):
        assert np.array_equal(a, b)
    assert whole[0].dtype == np.float32 and whole[1].dtype == np.uint8 and whole[2].dtype == bool and whole[3].dtype == np.int32
    assert whole[2].any() and np.array_equal(whole[3] > 0, whole[2])


def test_validation_errors_name_the_chunk():
    lib = cases.library("full")
    chunks, targets, lengths, bkps = (a[:6].copy() for a in cases.dna())
    run = splice_ref.splice_batch(lib)

    def bad(match, **kw):
        args = dict(chunks=chunks, targets=targets, lengths=lengths, bkps=bkps, ubs="XY", prop_ubs=0.1)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            sp.splice(args.pop("chunks"), args.pop("targets"), args.pop("lengths"), args.pop("bkps"), lib, run=run, **args)

    b = bkps.copy()
    b[4, 7] = b[4, 5]
    bad("chunk 4: breakpoints decrease", bkps=b)
    b = bkps.copy()
    b[2, 3] = b[2, 2]
    bad("chunk 2: a base without a sample", bkps=b)
    b = bkps.copy()
    b[5, 0] = 0
    bad("chunk 5: a base without a sample", bkps=b)
    b = bkps.copy()
    b[1, int(lengths[1]) - 1] = chunks.shape[1] + 1
    bad("chunk 1: a breakpoint beyond", bkps=b)
    ln = lengths.copy()
    ln[3] = targets.shape[1] + 1
    bad("chunk 3: reference length", lengths=ln)
    t = targets.copy()
    t[0, 2] = 7
    bad("chunk 0: a label above 6", targets=t)
    bad("cand_sample_size 33", cand_sample_size=33)
    bad("cand_sample_size 0", cand_sample_size=0)
    bad("ub_pad -1", pad=-1)
    bad("ubs must be X, Y or XY", ubs="XZ")
    bad("ubs must be X, Y or XY", ubs="")
    bad("prop_ubs", prop_ubs=0.9, var_prop_ubs=0.2)
    bad("65535", chunks=np.zeros((6, 65536), np.float32))
    bad(r"label rows of 65536", targets=np.zeros((6, 65536), np.uint8), bkps=np.zeros((6, 65536), np.uint16))
    with pytest.raises(ValueError, match="XNA chunk 0: breakpoints decrease"):
        x = [a.copy() for a in cases.xna()]
        x[3][0, 2] = 0
        sp.build_library(*x)
    assert sp.ubs_mask("X") == 1 and sp.ubs_mask("Y") == 2 and sp.ubs_mask("XY") == 3


@pytest.mark.parametrize("kw,word", [(dict(stitch_mode="per_slice"), "per_slice"), (dict(stitch_mode="mixed"), "mixed"),
                                     (dict(weighted_pos_pick=True), "kmer_count-len_6.csv"),
                                     (dict(stitch_noise_std=0.1), "--stitch-noise-std"), (dict(permute_win_size=4), "--permute-win-size"),
                                     (dict(spike=True), "--spike"), (dict(ubs="N"), "--ubs")])
def test_cli_refusals(tmp_path, kw, word):
    dna, xna = cases.write_dirs(tmp_path)
    with pytest.raises(SystemExit) as e:
        cli.main(cases.namespace(dna_ctc_dir=dna, xna_ctc_dir=xna, out_dir=str(tmp_path / "out"), **kw))
    assert word in str(e.value) and not os.path.exists(str(tmp_path / "out"))


def test_cli_parser_matches_the_reference_names():
    args = cli.argparser().parse_args(["a", "b", "c", "--ubs", "X", "--prop-ubs", "0.05"])
    assert (args.ubs, args.prop_ubs, args.var_prop_ubs, args.cand_sample_size, args.ub_pad, args.seed, args.batchsize,
            args.stitch_mode) == ("X", 0.05, None, 10, 5, 2012, 4096, "per_kmer")
    with pytest.raises(SystemExit):
        cli.argparser().parse_args(["a", "b", "c", "--stitch-mode", "per_read"])


def test_cli_files(tmp_path):
    """Shapes, dtypes and contents of OUT_DIR with the restatement in the device's place; a directory without
    breakpoints.npy and an existing output are refused."""
    _, meta = cases.golden()
    case = meta["cases"][0]
    dna, xna = cases.write_dirs(tmp_path)
    out = str(tmp_path / "out")
    args = cases.namespace(dna_ctc_dir=dna, xna_ctc_dir=xna, out_dir=out, ubs=case["ubs"], prop_ubs=case["prop_ubs"],
                           cand_sample_size=case["cand_sample_size"], ub_pad=case["pad"], seed=meta["seed"], batchsize=16)
    cli.main(args, make_run=splice_ref.splice_batch)
    want = cases.expected(case)
    z, _ = cases.golden()
    got = {f: np.load(os.path.join(out, f)) for f in sp.FILES}
    assert got["chunks.npy"].dtype == np.float16 and np.array_equal(got["chunks.npy"], want[0].astype(np.float16))
    assert got["references.npy"].dtype == np.uint8 and np.array_equal(got["references.npy"], want[1])
    assert np.array_equal(got["reference_lengths.npy"], z["dna_lengths"]) and got["reference_lengths.npy"].dtype == z["dna_lengths"].dtype
    assert np.array_equal(got["breakpoints.npy"], z["dna_bkps"]) and got["breakpoints.npy"].dtype == np.uint16
    lines = open(os.path.join(out, "splice_stats.csv")).read().split()
    assert lines[0] == "index,success,inserted" and len(lines) == 1 + len(want[2])
    rows = np.array([[int(v) for v in ln.split(",")] for ln in lines[1:]])
    assert np.array_equal(rows[:, 0], np.arange(len(want[2]))) and np.array_equal(rows[:, 1].astype(bool), want[2])
    assert np.array_equal(rows[:, 2], (want[1] != z["dna_targets"]).sum(axis=1))
    with pytest.raises(SystemExit, match="--overwrite"):
        cli.main(args, make_run=splice_ref.splice_batch)
    args.overwrite = True
    cli.main(args, make_run=splice_ref.splice_batch)
    os.remove(os.path.join(xna, "breakpoints.npy"))
    with pytest.raises(SystemExit, match="breakpoints.npy"):
        cli.main(args, make_run=splice_ref.splice_batch)
