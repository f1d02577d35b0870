"""CPU: the contract of xb_synth_chunks (include/xna_basecaller.h) as tests/synth_ref.py restates it, against what the
reference's spike_chunks.py computed with fully_synth=True on the spike fixture's inputs (tests/golden/synth.npz / .json); the
host side (xna_basecaller_amd/spike.py: synth) and the `synth` command with the restatement in the device's place."""
import os

import numpy as np
import pytest

import spike_cases
import synth_cases as cases
import synth_ref
from xna_basecaller_amd import spike as sk
from xna_basecaller_amd.cli import spike as spike_cli
from xna_basecaller_amd.cli import synth as cli

CASE_NAMES = ("uniform_xy", "shift_variable_noise_xy", "truncnorm_fixed_noise_y", "resynthesis_n", "one_x_pad3", "var_prop_xy",
              "uniform_fixed_noise_xy")


@pytest.mark.parametrize("index", range(len(CASE_NAMES)))
def test_restatement_equals_the_reference(index):
    """Positions, UBs, labels, med and mad bit-equal in every case; every float32 value of every synthesised chunk bit-equal
    where only uniform draws are involved and within one float32 step where a truncated normal is (two float64 routes to one
    quantile; tests/test_spike_host.py); the fixture records how many values differ at all (none does).  Where the reference
    raises KeyError the restatement's status is 2 and names the same k-mer."""
    _, meta = cases.golden()
    case = meta["cases"][index]
    assert case["name"] == CASE_NAMES[index]
    data = cases.dna()
    got, stats = cases.golden_reference(index)
    want = cases.expected(case)
    bad = cases.raised(case)
    ok = np.array([c not in bad for c in range(len(data[2]))])
    assert stats["positions"] == case["positions"]
    assert stats["ubs"] == case["position_ubs"]
    assert np.array_equal(got[1], want[1]) and np.array_equal(got[2], want[2]) and np.array_equal(got[5], want[5])
    assert np.array_equal(got[3][ok].view(np.uint64), want[3][ok].view(np.uint64)), "med"
    assert np.array_equal(got[4][ok].view(np.uint64), want[4][ok].view(np.uint64)), "mad"
    steps = np.abs(got[0].view(np.int32).astype(np.int64) - want[0].view(np.int32).astype(np.int64))
    print("%s: %d of %d synthesised values differ, the largest by %d float32 steps; %d went through a truncated normal"
          % (case["name"], (steps > 0).sum(), case["values_synthesised"], steps.max(), stats["ppnd"]))
    assert (steps > 0).sum() == case["values_differing_from_restatement"]
    assert steps.max() <= (0 if case["exact"] else 1)
    assert case["values_synthesised"] == stats["total"] == int(ok.sum()) * data[0].shape[1]
    # every chunk is synthesised, a position or not; a chunk that raised is the input
    changed = (want[0].view(np.uint32) != data[0].view(np.uint32)).mean(axis=1)
    assert (changed[ok] > 0.99).all() and not changed[~ok].any()
    assert np.array_equal(want[1][~ok], data[1][~ok]) and np.isnan(got[4][~ok]).all()
    assert {c: sk.index_kmer(got[3][c]) for c in bad} == bad
    if case["ubs"] == "N":
        assert np.array_equal(want[1], data[1]) and want[2].sum() > 0


def test_fixture_covers_what_it_names():
    _, meta = cases.golden()
    by = {c["name"]: c for c in meta["cases"]}
    assert tuple(c["name"] for c in meta["cases"]) == CASE_NAMES
    spike_by = {c["name"]: c for c in spike_cases.golden()[1]["cases"]}
    for name, case in by.items():                        # the inputs, draws and so the positions are the spike fixture's
        assert case["positions"] == spike_by[name]["positions"] and case["position_ubs"] == spike_by[name]["position_ubs"]
        assert all(case[k] == spike_by[name][k] for k in ("ubs", "prop_ubs", "var_prop_ubs", "pad", "std_dist", "noise_std"))
    assert [n for n, c in by.items() if c["raised"]] == [cases.PAD3] and len(by[cases.PAD3]["raised"]) == 26
    for c, kmer in cases.raised(by[cases.PAD3]).items():  # positions four bases apart: two X in one k-mer
        assert kmer.count("X") == 2 and min(np.diff(by[cases.PAD3]["positions"][c])) < 6
    # chunks 11 and 19 have no free base: synthesised all the same, no UB written
    got, _ = cases.golden_reference(0)
    data = cases.dna()
    for c in (11, 19):
        assert by["uniform_xy"]["positions"][c] == [] and got[2][c] == 0 and np.array_equal(got[1][c], data[1][c])
        assert (got[0][c] != data[0][c]).all()
    # med comes from the spiked labels: where an UB was written it is another than spike's (the original labels) -- in most
    # chunks, since swapping six k-mers of a chunk can leave the two middle values in place; where none was, it is the same
    spike_med = spike_cases.expected(spike_by["uniform_xy"])[3]
    assert (got[3][got[2] > 0] != spike_med[got[2] > 0]).sum() > 20 and np.array_equal(got[3][[11, 19]], spike_med[[11, 19]])


def test_one_shift_and_one_noise_std_per_chunk():
    """With stdv 0 in the model and fixed noise off, a chunk's value is (mean - med) / mad of its base's k-mer: the samples of
    one base are equal, bases without a sample draw nothing, and the samples past the last breakpoint keep the input."""
    mean, stdv = cases.model()
    flat = (mean, np.zeros_like(stdv))
    data = cases.one_chunk(3, 30, 200)
    bk = data[3].copy()
    bk[0, :30] = 6 * np.arange(1, 31) + 10               # ends at 190, short of the chunk
    bk[0, 0] = 0                                         # an empty first base
    bk[0, 10:16] = bk[0, 9]                              # a run of six empty bases
    stats = {}
    out, out_t, n, med, mad, status = synth_ref.synth_chunk(data[0][0], data[1][0], 30, bk[0], flat, 0, 1, 3, 0.1, 0.0, 5, 0, np.zeros((1, 2)),
                                                            0.0, False, stats=stats)
    assert status == 0 and n >= 1 and stats["empty"] == 7 and stats["total"] == 190
    assert np.array_equal(out[190:], data[0][0][190:]) and (out[:190] != data[0][0][:190]).all()
    start = 0
    full = synth_ref.letters_with_tail([int(v) for v in out_t[:30]])
    for base in range(30):
        end = int(bk[0, base])
        want = np.float32((mean[synth_ref.kmer_index(full[base:base + 6])] - med) / mad)
        assert (out[start:end] == want).all(), base
        start = end


def test_validation_and_missing_kmers_name_the_chunk():
    data = [a[:6].copy() for a in cases.dna()]
    run = synth_ref.synth_batch(cases.model())

    def bad(match, data=data, **kw):
        args = dict(ubs="XY", prop_ubs=0.1)
        args.update(kw)
        with pytest.raises(ValueError, match=match):
            sk.synth(*data, cases.model(), run=run, **args)

    b = data[3].copy()
    b[3, int(data[2][3]) - 1] -= 1
    bad("DNA chunk 3: its last breakpoint is 479, the chunk has 480 samples", data=data[:3] + [b])
    b = data[3].copy()
    b[4, 7] = b[4, 5]
    bad("chunk 4: breakpoints decrease", data=data[:3] + [b])
    bad("ub_pad -1", pad=-1)
    bad("prop_ubs", prop_ubs=0.9, var_prop_ubs=0.2)
    bad("noise_std", noise_std=-1.0)
    for name in sk.REFUSED_DISTS + ("uniform_shift_1.5_0.5",):
        bad("not offered", std_dist=name)
    t = data[1].copy()
    t[2, 4] = 3                                          # a G: the model has no k-mer with it
    letters = "".join(sk.BASE_MAP[v] for v in t[2, :6])
    bad("DNA chunk 2: the pore model has no k-mer %s" % letters, data=[data[0], t] + data[2:])
    bad("DNA chunk [0-5]: the pore model has no k-mer [ACT]*X[ACT]*X", pad=3, ubs="X", prop_ubs=0.12)     # two UBs in one k-mer
    b = data[3].copy()
    b[1, 12] = b[1, 11]                                  # a base without a sample is allowed
    got = sk.synth(data[0], data[1], data[2], b, cases.model(), run=run, ubs="XY", prop_ubs=0.1)
    assert len(got) == 5 and got[0].dtype == np.float32 and got[1].dtype == np.uint8 and got[2].dtype == np.int32
    # what spike() returns for the same arguments is another thing: it keeps the signal outside the windows
    import spike_ref
    pasted = sk.spike(data[0], data[1], data[2], b, cases.model(), run=spike_ref.spike_batch(cases.model()), ubs="XY", prop_ubs=0.1)
    assert np.array_equal(pasted[1], got[1]) and (pasted[0] == data[0]).mean() > 0.3 and (got[0] == data[0]).mean() < 0.01


@pytest.mark.parametrize("kw,word", [(dict(equal_kmer_reps=True), "--equal-kmer-reps"), (dict(legacy_pos=True), "--legacy-pos"),
                                     (dict(std_dist="normal"), "not offered"), (dict(std_dist="uniform_shift_1.5_0.5"), "not offered"),
                                     (dict(std_dist="truncnorm_prerep"), "not offered"), (dict(ubs="Z"), "--ubs")])
def test_cli_refusals(tmp_path, kw, word):
    dna = cases.write_dir(tmp_path)
    model = cases.write_model(str(tmp_path / "kmer.model"))
    with pytest.raises(SystemExit) as e:
        cli.main(cases.namespace(ctc_dir=dna, out_dir=str(tmp_path / "out"), reference=model, **kw))
    assert word in str(e.value) and not os.path.exists(str(tmp_path / "out"))


def test_spike_fully_synth_is_still_refused_and_points_here(tmp_path):
    dna = cases.write_dir(tmp_path)
    model = cases.write_model(str(tmp_path / "kmer.model"))
    with pytest.raises(SystemExit) as e:
        spike_cli.main(spike_cases.namespace(ctc_dir=dna, out_dir=str(tmp_path / "out"), reference=model, fully_synth=True))
    assert "--fully_synth" in str(e.value) and "`synth`" in str(e.value) and not os.path.exists(str(tmp_path / "out"))


def test_cli_parser_defaults_and_registration():
    args = cli.argparser().parse_args(["a", "b", "-r", "m", "--ubs", "X", "--prop-ubs", "0.05", "--std-dist", "truncnorm_shift_1.5_0.5",
                                       "--noise-std", "1.00", "--variable-noise"])
    assert (args.ubs, args.prop_ubs, args.var_prop_ubs, args.ub_pad, args.seed, args.batchsize, args.std_dist, args.noise_std,
            args.variable_noise, args.reference) == ("X", 0.05, None, 5, 2012, 4096, "truncnorm_shift_1.5_0.5", 1.0, True, "m")
    args = cli.argparser().parse_args(["a", "b", "-r", "m"])
    assert (args.ubs, args.prop_ubs, args.std_dist, args.noise_std, args.variable_noise, args.overwrite, args.equal_kmer_reps,
            args.legacy_pos, args.device) == ("XY", 0, "uniform", 0, False, False, False, False, "cuda")
    assert not hasattr(args, "fully_synth")
    import xna_basecaller_amd.__main__ as entry
    assert entry.synth is cli


def test_cli_files_and_batch_independence(tmp_path):
    """Shapes, dtypes and contents of OUT_DIR with the restatement in the device's place, for the recipe's distribution; the
    same output whatever --batchsize; an existing output and a missing breakpoints.npy are refused."""
    z = spike_cases.golden()[0]
    _, meta = cases.golden()
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
        cli.main(args, make_run=synth_ref.synth_batch)
        assert sorted(os.listdir(out)) == sorted(sk.FILES + ("synth_stats.csv",))
        outs.append({f: np.load(os.path.join(out, f)) for f in sk.FILES})
        outs[-1]["csv"] = open(os.path.join(out, "synth_stats.csv")).read()
    got = outs[0]
    for other in outs[1:]:
        assert all(np.array_equal(got[f], other[f]) for f in sk.FILES) and got["csv"] == other["csv"]
    assert got["chunks.npy"].dtype == np.float16 and np.array_equal(got["chunks.npy"], want[0].astype(np.float16))
    assert got["references.npy"].dtype == np.uint8 and np.array_equal(got["references.npy"], want[1])
    assert np.array_equal(got["reference_lengths.npy"], z["dna_lengths"]) and got["reference_lengths.npy"].dtype == z["dna_lengths"].dtype
    assert np.array_equal(got["breakpoints.npy"], z["dna_bkps"]) and got["breakpoints.npy"].dtype == np.uint16
    lines = got["csv"].split()
    assert lines[0] == "index,spiked,med,mad" and len(lines) == 1 + len(want[2])
    rows = [ln.split(",") for ln in lines[1:]]
    assert [int(r[0]) for r in rows] == list(range(len(want[2]))) and [int(r[1]) for r in rows] == [int(v) for v in want[2]]
    assert [float(r[2]) for r in rows] == [float(v) for v in want[3]] and [float(r[3]) for r in rows] == [float(v) for v in want[4]]
    with pytest.raises(SystemExit, match="--overwrite"):
        cli.main(args, make_run=synth_ref.synth_batch)
    args.overwrite = True
    cli.main(args, make_run=synth_ref.synth_batch)
    os.remove(os.path.join(dna, "breakpoints.npy"))
    with pytest.raises(SystemExit, match="breakpoints.npy"):
        cli.main(args, make_run=synth_ref.synth_batch)
