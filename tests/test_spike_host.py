"""CPU: the contract of xb_spike_chunks (include/xna_basecaller.h) as tests/spike_ref.py restates it, against what the
reference's spike_chunks.py computed on the golden fixture (tests/golden/spike.npz / .json); its logarithm and PPND16 against
libm and CPython's statistics; the host side (xna_basecaller_amd/spike.py) and the `spike` command with the restatement in
the device's place."""
import math
import os
import statistics

import numpy as np
import pytest

import spike_cases as cases
import spike_ref
from xna_basecaller_amd import spike as sk
from xna_basecaller_amd.cli import spike as cli
from xna_basecaller_amd.segment import load_kmer_poremodel

CASE_NAMES = ("uniform_xy", "shift_variable_noise_xy", "truncnorm_fixed_noise_y", "resynthesis_n", "one_x_pad3", "var_prop_xy",
              "uniform_fixed_noise_xy")
# the bound of the issue for the restated log and PPND16: far above the < 1 ulp of such algorithms, far below float32's 2^-24
REL_BOUND = 2.0 ** -50


@pytest.mark.parametrize("index", range(len(CASE_NAMES)))
def test_restatement_equals_the_reference(index):
    """Positions, UBs, labels, med and mad bit-equal in every case; the pasted float32 values bit-equal where only uniform
    draws are involved and within one float32 step where a truncated normal is (two float64 routes to one quantile differ by
    about 1e-15 relative, which float32 rounding turns into at most one step); the fixture records how many differ at all."""
    _, meta = cases.golden()
    case = meta["cases"][index]
    assert case["name"] == CASE_NAMES[index]
    data = cases.dna()
    stats = {}
    got = cases.reference(data, cases.model(), 0, meta["seed"], cases.case_args(case), stats=stats)
    want = cases.expected(case)
    assert stats["positions"] == case["positions"]
    assert [u for u in stats["ubs"]] == case["position_ubs"]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and not got[5].any()
    assert np.array_equal(got[3].view(np.uint64), want[3].view(np.uint64)), "med"
    assert np.array_equal(got[4].view(np.uint64), want[4].view(np.uint64)), "mad"
    steps = np.abs(got[0].view(np.int32).astype(np.int64) - want[0].view(np.int32).astype(np.int64))
    print("%s: %d of %d pasted values differ, the largest by %d float32 steps" % (case["name"], (steps > 0).sum(),
                                                                                 (want[0] != data[0]).sum(), steps.max()))
    assert (steps > 0).sum() == case["values_differing_from_restatement"]
    assert steps.max() <= (0 if case["exact"] else 1)
    changed = (want[0].view(np.uint32) != data[0].view(np.uint32)).any(axis=1)
    assert np.array_equal(changed, want[2] > 0)
    if case["ubs"] == "N":
        assert np.array_equal(want[1], data[1]) and want[2].sum() > 0


def test_fixture_covers_what_it_names():
    _, meta = cases.golden()
    by = {c["name"]: c for c in meta["cases"]}
    assert tuple(c["name"] for c in meta["cases"]) == CASE_NAMES
    assert by["shift_variable_noise_xy"]["std_dist"] == "truncnorm_shift_1.5_0.5" and by["shift_variable_noise_xy"]["variable_noise"]
    # 18 bases leave no valid base; 33 bases with an unnatural base at 12 neither
    assert [i for i, p in enumerate(by["uniform_xy"]["positions"]) if not p] == [11, 19]
    data = cases.dna()
    for c in (3, 11, 27):                                 # existing UBs are kept and kept clear of
        for case in meta["cases"]:
            for ub in np.flatnonzero(data[1][c] > 4):
                assert all(abs(p - ub) > 2 * case["pad"] for p in case["positions"][c])
    assert {5, 6} <= {u for row in by["uniform_xy"]["position_ubs"] for u in row}
    assert {u for row in by["one_x_pad3"]["position_ubs"] for u in row} == {5}
    assert {u for row in by["resynthesis_n"]["position_ubs"] for u in row} == {0}


def _arguments():
    """10^5 arguments over the range the truncations reach: p from Phi(-3.5) to 1 - Phi(-3.5), and the logarithm's own
    arguments min(p, 1 - p)."""
    lo = sk.phi(-3.5)
    rng = np.random.default_rng(5)
    p = np.concatenate([np.exp(rng.uniform(math.log(lo), math.log(0.5), 40000)), rng.uniform(lo, 1.0 - lo, 59990),
                        [lo, 0.5, 1.0 - lo, 0.075, 0.925, 0.0750001, 0.9249999, 0.25, 0.75, 0.4999999]])
    assert len(p) == 100000
    return [float(v) for v in p]


def test_log_and_ppnd16_against_libm_and_statistics():
    inv = statistics.NormalDist().inv_cdf
    worst_log = worst_inv = 0.0
    for p in _arguments():
        r = min(p, 1.0 - p)
        worst_log = max(worst_log, abs(spike_ref.xb_log(r) - math.log(r)) / abs(math.log(r)))
        want = inv(p)
        got = spike_ref.ppnd16(p)
        worst_inv = max(worst_inv, abs(got - want) / abs(want) if want else abs(got))
    print("largest relative error: log %.3g (%.2f ulp of 2^-53), PPND16 %.3g" % (worst_log, worst_log * 2 ** 53, worst_inv))
    assert worst_log <= REL_BOUND and worst_inv <= REL_BOUND
    # with libm's log in place of its own the restatement IS statistics' algorithm
    for p in (0.001, 0.02, 0.3, 0.5, 0.7, 0.98, 0.9999):
        assert spike_ref.ppnd16(p, log=math.log) == inv(p)


def test_model_table_indexing(tmp_path):
    assert sk.kmer_index("NNNNNN") == 0 and sk.kmer_index("NNNNNA") == 1 and sk.kmer_index("ANNNNN") == 7 ** 5
    assert sk.kmer_index("YYYYYY") == 7 ** 6 - 1 and sk.kmer_index("ACGTXY") == spike_ref.kmer_index([1, 2, 3, 4, 5, 6])
    for t in (0, 1, 7 ** 5, 54321, 7 ** 6 - 1):
        assert sk.kmer_index(sk.index_kmer(t)) == t
    path = cases.write_model(str(tmp_path / "kmer.model"))
    mean, stdv = sk.load_model(path)
    want = cases.model()
    assert np.array_equal(np.isnan(mean), np.isnan(want[0])) and np.array_equal(stdv, want[1])
    assert np.array_equal(mean[~np.isnan(mean)], want[0][~np.isnan(mean)]) and (~np.isnan(mean)).sum() == 3 ** 6 + 12 * 3 ** 5
    assert mean[sk.kmer_index("ACTACX")] == load_kmer_poremodel(path)["ACTACX"][0] and np.isnan(mean[sk.kmer_index("ACGACT")])
    with pytest.raises(ValueError, match="AC"):
        sk.model_table({"AC": (1.0, 1.0)})
    with pytest.raises(ValueError, match="level_stdv"):
        sk.model_table({"ACTACT": (1.0, -1.0)})


def test_std_dist_parsing_and_refusals():
    assert sk.parse_std_dist("uniform") == [] and sk.parse_std_dist("truncnorm") == [(-2.0, 2.0)]
    assert sk.parse_std_dist("truncnorm_shift_1.5_0.5") == [(-2.0, 1.0), (-1.5, 1.5), (-1.0, 2.0)]
    assert len(sk.parse_std_dist("truncnorm_shift_2_1.5")) == 7 and sk.parse_std_dist("truncnorm_shift_2_0") == [(-2.0, 2.0)]
    rows, phi = sk.phi_table("truncnorm_shift_1.5_0.5")
    assert rows == 3 and phi.shape == (4, 2) and phi.dtype == np.float64
    nd = statistics.NormalDist()
    for (a, b), (pa, pw) in zip([(-2.0, 1.0), (-1.5, 1.5), (-1.0, 2.0), (-3.0, 3.0)], phi):
        assert abs(pa - nd.cdf(a)) < 1e-15 and abs(pw - (nd.cdf(b) - nd.cdf(a))) < 1e-15
    assert sk.phi_table("uniform")[0] == 0 and sk.phi_table("uniform")[1].shape == (1, 2)
    for name in ("normal", "uniform_shift_not_shared", "uniform_shift_shared", "uniform_shift_1.5_0.5", "truncnorm_prerep"):
        with pytest.raises(ValueError, match="not offered"):
            sk.parse_std_dist(name)
    for name, word in (("gauss", "not one of"), ("truncnorm_shift_1.5", "expected"), ("truncnorm_shift_a_b", "expected"),
                       ("truncnorm_shift_0_1", "positive"), ("truncnorm_shift_1.5_8", "33 shift values"),
                       ("truncnorm_shift_1_40", "shift values")):
        with pytest.raises(ValueError, match=word):
            sk.phi_table(name)
    assert [sk.ubs_mask(u) for u in ("N", "X", "Y", "XY")] == [0, 1, 2, 3]
    for bad in ("", "XZ", "NX", "YX"):
        with pytest.raises(ValueError, match="ubs must be"):
            sk.ubs_mask(bad)


def test_validation_and_missing_kmers_name_the_chunk():
    data = [a[:6].copy() for a in cases.dna()]
    run = spike_ref.spike_batch(cases.model())

    def bad(match, data=data, **kw):
        args = dict(ubs="XY", prop_ubs=0.1)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            sk.spike(*data, cases.model(), run=run, **args)

    b = data[3].copy()
    b[4, 7] = b[4, 5]
    bad("chunk 4: breakpoints decrease", data=data[:3] + [b])
    bad("ub_pad -1", pad=-1)
    bad("prop_ubs", prop_ubs=0.9, var_prop_ubs=0.2)
    bad("noise_std", noise_std=-1.0)
    bad("not offered", std_dist="normal")
    t = data[1].copy()
    t[2, 4] = 3                                          # a G: the model has no k-mer with it
    letters = "".join(sk.BASE_MAP[v] for v in t[2, :6])
    bad("DNA chunk 2: the pore model has no k-mer %s" % letters, data=[data[0], t] + data[2:])
    b = data[3].copy()
    b[1, 12] = b[1, 11]                                  # a base without a sample is allowed here
    sk.spike(data[0], data[1], data[2], b, cases.model(), run=run, ubs="XY", prop_ubs=0.1)


@pytest.mark.parametrize("kw,word", [(dict(fully_synth=True), "--fully_synth"), (dict(equal_kmer_reps=True), "--equal-kmer-reps"),
                                     (dict(legacy_pos=True), "--legacy-pos"), (dict(std_dist="normal"), "not offered"),
                                     (dict(std_dist="uniform_shift_1.5_0.5"), "not offered"),
                                     (dict(std_dist="truncnorm_prerep"), "not offered"), (dict(ubs="Z"), "--ubs")])
def test_cli_refusals(tmp_path, kw, word):
    dna = cases.write_dir(tmp_path)
    model = cases.write_model(str(tmp_path / "kmer.model"))
    with pytest.raises(SystemExit) as e:
        cli.main(cases.namespace(ctc_dir=dna, out_dir=str(tmp_path / "out"), reference=model, **kw))
    assert word in str(e.value) and not os.path.exists(str(tmp_path / "out"))


def test_cli_parser_matches_the_reference_names():
    args = cli.argparser().parse_args(["a", "b", "-r", "m", "--ubs", "X", "--prop-ubs", "0.05", "--std-dist", "truncnorm_shift_1.5_0.5",
                                       "--noise-std", "1.00", "--variable-noise"])
    assert (args.ubs, args.prop_ubs, args.var_prop_ubs, args.ub_pad, args.seed, args.batchsize, args.std_dist, args.noise_std,
            args.variable_noise, args.reference) == ("X", 0.05, None, 5, 2012, 4096, "truncnorm_shift_1.5_0.5", 1.0, True, "m")
    args = cli.argparser().parse_args(["a", "b", "-r", "m"])
    assert (args.std_dist, args.noise_std, args.variable_noise, args.fully_synth) == ("uniform", 0, False, False)


def test_cli_files_and_batch_independence(tmp_path):
    """Shapes, dtypes and contents of OUT_DIR with the restatement in the device's place, for the recipe's default
    distribution; the same output whatever --batchsize; an existing output and a missing breakpoints.npy are refused."""
    z, meta = cases.golden()
    case = meta["cases"][1]
    dna = cases.write_dir(tmp_path)
    model = cases.write_model(str(tmp_path / "kmer.model"))
    want = cases.expected(case)
    outs = []
    for batch in (4096, 7, 1):
        out = str(tmp_path / ("out%d" % batch))
        args = cases.namespace(ctc_dir=dna, out_dir=out, reference=model, ubs=case["ubs"], prop_ubs=case["prop_ubs"],
                               ub_pad=case["pad"], std_dist=case["std_dist"], noise_std=case["noise_std"],
                               variable_noise=case["variable_noise"], seed=meta["seed"], batchsize=batch)
        cli.main(args, make_run=spike_ref.spike_batch)
        outs.append({f: np.load(os.path.join(out, f)) for f in sk.FILES})
        outs[-1]["csv"] = open(os.path.join(out, "spike_stats.csv")).read()
    got = outs[0]
    for other in outs[1:]:
        assert all(np.array_equal(got[f], other[f]) for f in sk.FILES) and got["csv"] == other["csv"]
    steps = np.abs(got["chunks.npy"].astype(np.float32) - want[0].astype(np.float16).astype(np.float32))
    assert got["chunks.npy"].dtype == np.float16 and np.array_equal(got["chunks.npy"], want[0].astype(np.float16)), steps.max()
    assert got["references.npy"].dtype == np.uint8 and np.array_equal(got["references.npy"], want[1])
    assert np.array_equal(got["reference_lengths.npy"], z["dna_lengths"]) and got["reference_lengths.npy"].dtype == z["dna_lengths"].dtype
    assert np.array_equal(got["breakpoints.npy"], z["dna_bkps"]) and got["breakpoints.npy"].dtype == np.uint16
    lines = got["csv"].split()
    assert lines[0] == "index,spiked,med,mad" and len(lines) == 1 + len(want[2])
    rows = [ln.split(",") for ln in lines[1:]]
    assert [int(r[0]) for r in rows] == list(range(len(want[2]))) and [int(r[1]) for r in rows] == [int(v) for v in want[2]]
    assert [float(r[2]) for r in rows] == [float(v) for v in want[3]] and [float(r[3]) for r in rows] == [float(v) for v in want[4]]
    with pytest.raises(SystemExit, match="--overwrite"):
        cli.main(args, make_run=spike_ref.spike_batch)
    args.overwrite = True
    cli.main(args, make_run=spike_ref.spike_batch)
    os.remove(os.path.join(dna, "breakpoints.npy"))
    with pytest.raises(SystemExit, match="breakpoints.npy"):
        cli.main(args, make_run=spike_ref.spike_batch)
