"""Regenerates tests/golden/splice.npz and splice.json: what the reference's XNA augmentation computes on small synthetic
ctc-data, with the contract's draws (tests/splice_ref.py: Draws) as its random generator.

Run in the BUILD container only.  It imports, BY FILE PATH and as reference code, ub-bonito/bonito/stitch_chunks.py (numpy,
pandas and tqdm are all it needs) and runs slice_xna(.., 'per_kmer', include_chunks=True), stitch_read_per_kmer(rng=Draws) and
prepare_slice_chunk.  Only DATA is stored: the inputs, the reference's library rows in its order, its chunks, labels and
success flags, prepare_slice_chunk's inputs and outputs for hand-picked cases, and counts of what the cases exercise.

The alphabet has two letters (labels 1, 2), so that 256 XNA reads built template-UB-template over all 32 five-mers give all
2 * 32 * 6 groups and random positions find candidates.  The second library lacks the templates that start with 1 1: some
positions are abandoned.  Both files are byte-for-byte reproducible (the archive's time stamps are fixed).
"""
import importlib.util
import io
import json
import os
import sys
import tempfile
import zipfile

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import splice_ref  # noqa: E402

REFTREE = "/root/reference"
SEED = 2012
N_DNA, N_XNA, LT = 600, 200, 80
CASES = [   # name, library, ubs, prop_ubs, var_prop_ubs, cand_sample_size, pad
    ("xy_cand5", "full", "XY", 0.08, None, 5, 5),
    ("x_var_cand1", "full", "X", 0.10, 0.05, 1, 5),
    ("y_cand32_pad3", "full", "Y", 0.10, 0.0, 32, 3),
    ("holes_xy_var", "holes", "XY", 0.10, 0.05, 5, 5),
]
PREPARE = [  # k-mer sample counts, ins_len
    ([1, 1, 1, 1, 1, 1], 7), ([1, 1, 1, 1, 1, 1], 20), ([1, 1, 1, 1, 1, 1], 5), ([1, 1, 1, 1, 1, 1], 6),
    ([3, 1, 4, 2, 1, 5], 17), ([3, 1, 4, 2, 1, 5], 40), ([3, 1, 4, 2, 1, 5], 15), ([3, 1, 4, 2, 1, 5], 10),
    ([4, 4, 4, 4, 4, 4], 25), ([4, 4, 4, 4, 4, 4], 26), ([4, 4, 4, 4, 4, 4], 27), ([9, 2, 30, 1, 7, 12], 200),
    ([100, 100, 100, 100, 100, 100], 601), ([100, 1, 100, 1, 100, 1], 64),
]


def load_reference():
    spec = importlib.util.spec_from_file_location("ref_stitch_chunks", os.path.join(REFTREE, "ub-bonito", "bonito", "stitch_chunks.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def random_breakpoints(rng, n_samples, length):
    cuts = np.sort(rng.choice(np.arange(1, n_samples), size=length - 1, replace=False))
    return np.concatenate([cuts, [n_samples]])


def make_xna(rng):
    """256 reads template-UB-template, four per (UB, template), with 1 .. 3 letters in front and 0 .. 3 behind; 12 reads whose
    letters behind the UB are not the template's (the reference groups without the k-mer); then the reads that slice_xna (or
    build_library) drops: no UB, UB too close to either edge, a k-mer of more than 100 samples."""
    reads = []
    for ub in (5, 6):
        for t in range(32):
            tpl = [1 + (t >> (4 - q) & 1) for q in range(5)]
            for _ in range(4):
                pre = [int(v) for v in rng.integers(1, 3, rng.integers(1, 4))]
                post = [int(v) for v in rng.integers(1, 3, rng.integers(0, 4))]
                reads.append((pre + tpl + [ub] + tpl + post, None))
    for k in range(12):                                                  # other letters behind the UB: groups of mixed k-mers
        tpl = [1 + (5 * k >> (4 - q) & 1) for q in range(5)]
        other = [3 - v for v in tpl[:2]] + [int(v) for v in rng.integers(1, 3, 3)]
        reads.append(([2] + tpl + [5 + k % 2] + other + [1], None))
    reads.append(([1, 2] * 7, None))                                     # no UB
    reads.append(([1, 2, 1, 2, 1, 5, 1, 2, 1, 2, 1, 2, 2], None))          # ub_pos = 5
    reads.append(([1, 2, 1, 2, 1, 2, 1, 2, 6, 1, 2, 1, 2], None))          # ub_pos = length - 5
    reads.append(([2, 1, 1, 1, 1, 1, 5, 1, 1, 1, 1, 1, 2], "long"))        # a k-mer of 101 samples
    order = rng.permutation(len(reads))
    n = len(reads)
    chunks = (rng.standard_normal((n, N_XNA)) * 1.5).astype(np.float16)
    targets = np.zeros((n, 20), np.uint8)
    lengths = np.zeros(n, np.uint16)
    bkps = np.zeros((n, 20), np.uint16)
    for row, src in enumerate(order):
        labels, kind = reads[src]
        L = len(labels)
        targets[row, :L] = labels
        lengths[row] = L
        if kind == "long":
            b = np.concatenate([np.arange(1, 5), [105], 105 + np.arange(1, L - 4) * 5])
            b[-1] = N_XNA
        else:
            b = random_breakpoints(rng, N_XNA, L)
        bkps[row, :L] = b
    return chunks, targets, lengths, bkps


def make_dna(rng):
    """40 chunks of 25 .. 75 bases with naive breakpoints; chunks 3, 11, 27 carry an UB already, chunk 19 has 18 bases."""
    n = 40
    chunks = (rng.standard_normal((n, N_DNA)) * 1.2).astype(np.float16)
    targets = np.zeros((n, LT), np.uint8)
    lengths = rng.integers(25, 76, n).astype(np.uint16)
    lengths[19] = 18
    lengths[3], lengths[11], lengths[27] = 50, 33, 60
    bkps = np.zeros((n, LT), np.uint16)
    for c in range(n):
        L = int(lengths[c])
        targets[c, :L] = rng.integers(1, 3, L)
        reps = np.full(L, N_DNA // L)
        reps[:N_DNA % L] += 1
        bkps[c, :L] = np.cumsum(reps)
    targets[3, 20], targets[11, 12], targets[27, 30], targets[27, 31] = 5, 6, 5, 6
    return chunks, targets, lengths, bkps


def keep_in_holes(labels):
    """The second library drops the reads whose template starts with 1 1."""
    ubs = np.flatnonzero(labels > 4)
    return not (ubs.size and ubs[0] >= 5 and tuple(labels[ubs[0] - 5:ubs[0] - 3]) == (1, 1))


def write_dir(path, chunks, targets, lengths, bkps):
    os.makedirs(path)
    for name, a in zip(("chunks", "references", "reference_lengths", "breakpoints"), (chunks, targets, lengths, bkps)):
        np.save(os.path.join(path, name + ".npy"), a)


def base7(letters, ref):
    t = 0
    for ch in letters:
        t = t * 7 + ref.BASE_MAP.index(ch)
    return t


def library_rows(ref, grouped):
    """The reference's sorted frame as integers: ub label, template and k-mer as base-7 numbers, kmer_ub_pos, read_idx,
    slice_st, slice_en."""
    df = grouped.obj
    rows = [(ref.BASE_MAP.index(ub), base7(tpl, ref), int(kpos), base7(kmer, ref), int(read), int(st), int(en))
            for (ub, tpl, kpos, kmer, read), st, en in zip(df.index, df.slice_st, df.slice_en)]
    return np.array(rows, dtype=np.int32)


def write_npz(path, arrays):
    with zipfile.ZipFile(path, "w") as z:
        for name in sorted(arrays):
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.ascontiguousarray(arrays[name]), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type = zipfile.ZIP_DEFLATED
            info.external_attr = 0o644 << 16
            z.writestr(info, buf.getvalue(), compresslevel=9)


def main():
    ref = load_reference()
    rng = np.random.default_rng(20121)
    xna = make_xna(rng)
    dna = make_dna(rng)
    holes = np.array([keep_in_holes(t[:int(L)]) for t, L in zip(xna[1], xna[2])])
    # slice_xna raises on a read without an UB (build_library skips it): the reference gets the library without that read,
    # as rows that keep their read_idx
    has_ub = np.array([(t[:int(L)] > 4).any() for t, L in zip(xna[1], xna[2])])
    arrays = {"xna_chunks": xna[0], "xna_targets": xna[1], "xna_lengths": xna[2], "xna_bkps": xna[3], "xna_holes_keep": holes,
              "dna_chunks": dna[0], "dna_targets": dna[1], "dna_lengths": dna[2], "dna_bkps": dna[3]}
    meta = {"note": "inputs: synthetic two-letter ctc-data; outputs: what ub-bonito/bonito/stitch_chunks.py computed from them with "
                    "tests/splice_ref.py's Draws as rng (seed %d, one generator per chunk index)" % SEED,
            "seed": SEED, "cases": [], "prepare": []}
    libs = {}
    with tempfile.TemporaryDirectory() as tmp:
        for name, keep in (("full", np.ones(len(holes), bool)), ("holes", holes)):
            keep = keep & has_ub
            index = np.flatnonzero(keep)
            path = os.path.join(tmp, name)
            write_dir(path, *(a[keep] for a in xna))
            grouped = ref.slice_xna(path, "per_kmer", include_chunks=True)
            rows = library_rows(ref, grouped)
            rows[:, 4] = index[rows[:, 4]]                               # read_idx in the full set
            arrays["lib_%s_rows" % name] = rows
            libs[name] = grouped

    counts = {}
    real_prepare, real_choose = ref.prepare_slice_chunk, ref.choose_positions

    def prepare(slice_chunk, ins_len, kmer_cnts, verbose=False):
        kind = "stretch" if len(slice_chunk) < ins_len else ("shrink" if len(slice_chunk) > ins_len else "copy")
        counts[kind] += 1
        return real_prepare(slice_chunk, ins_len, kmer_cnts, verbose=verbose)

    def choose(*args, **kwargs):
        got = real_choose(*args, **kwargs)
        counts["positions"] += len(got)
        return got

    ref.prepare_slice_chunk, ref.choose_positions = prepare, choose
    chunks32 = dna[0].astype(np.float32)
    for name, lib, ubs, prop, var, cand, pad in CASES:
        counts.update(stretch=0, shrink=0, copy=0, positions=0)
        out = np.empty_like(chunks32)
        out_t = np.empty_like(dna[1])
        ok = np.zeros(len(chunks32), bool)
        for c in range(len(chunks32)):
            data = (chunks32[c], dna[1][c], int(dna[2][c]), dna[3][c].astype(int))
            out[c], out_t[c], ok[c] = ref.stitch_read_per_kmer(data, libs[lib], list(ubs), prop, var_prop_ubs=var,
                                                                 cand_sample_size=cand, rng=splice_ref.Draws(SEED, c), pad=pad)
        assert out.dtype == np.float32
        inserted = int((out_t != dna[1]).sum())
        arrays["out_%s_xor" % name] = out.view(np.uint32) ^ chunks32.view(np.uint32)     # zero wherever nothing was pasted
        arrays["out_%s_targets" % name] = out_t
        arrays["out_%s_success" % name] = ok
        meta["cases"].append(dict(name=name, library=lib, ubs=ubs, prop_ubs=prop, var_prop_ubs=var, cand_sample_size=cand, pad=pad,
                                  succeeded=int(ok.sum()), inserted=inserted, abandoned=counts["positions"] - inserted,
                                  **counts))
    ref.prepare_slice_chunk, ref.choose_positions = real_prepare, real_choose

    first = meta["cases"][0]
    assert first["succeeded"] >= 0.9 * len(chunks32), first
    assert first["stretch"] >= 10 and first["shrink"] >= 10, first
    assert meta["cases"][3]["abandoned"] >= 1, meta["cases"][3]
    assert all(c["abandoned"] == 0 for c in meta["cases"][:3]), meta["cases"]
    assert not arrays["out_xy_cand5_success"][19]

    repeated = 0
    for cnts, ins_len in PREPARE:
        values = (rng.standard_normal(sum(cnts)) * 1.5).astype(np.float16)
        got = ref.prepare_slice_chunk(values, ins_len, list(cnts))
        assert len(got) == ins_len
        if sum(cnts) < ins_len:
            xp = splice_ref.stretch_points(sum(cnts), ins_len, list(cnts))
            repeated += len(set(xp)) < len(xp)
        meta["prepare"].append(dict(kmer_cnts=cnts, ins_len=ins_len, values=[float(v) for v in values],
                                    out=[float(v) for v in np.asarray(got, dtype=np.float64)]))
    # Repeated xp cannot come out of prepare_slice_chunk while every k-mer has a sample: a stretch has step > 1, so the first
    # linspace is strictly increasing, a k-mer of n points gets the span left .. right with right - left >= n - 1, and points a
    # step >= 1 apart round to different integers.  (numpy.interp's rule for repeated xp, the largest j with xp[j] <= x, is
    # checked against numpy itself in tests/test_splice_host.py.)
    assert repeated == 0, repeated
    meta["prepare_repeated_xp"] = repeated

    write_npz(os.path.join(HERE, "splice.npz"), arrays)
    with open(os.path.join(HERE, "splice.json"), "w") as fh:
        json.dump(meta, fh, indent=1, sort_keys=True)
        fh.write("\n")
    print(json.dumps(meta["cases"], indent=1))
    print("rows:", {k: v.shape for k, v in arrays.items() if k.startswith("lib_")}, "repeated xp cases:", repeated)


if __name__ == "__main__":
    main()
