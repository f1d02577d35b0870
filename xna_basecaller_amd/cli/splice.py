"""
`python -m xna_basecaller_amd splice DNA_CTC_DIR XNA_CTC_DIR OUT_DIR --ubs XY --prop-ubs 0.1`: the reference's XNA spliced
augmentation (`bonito train -m per_kmer --xna_ctc_dir ...`, ub-bonito/bonito/stitch_chunks.py) as a tool of its own.  The
signal of the six k-mers around an unnatural base is cut out of the XNA chunks and pasted into the DNA chunks on the device
(xb_splice_chunks); OUT_DIR is a ctc-data directory that `evaluate`, `segment` and `bonito train --directory` read.  The
argument names and defaults are `bonito train`'s (cli/train.py:218-273).
"""
import os
import sys
import time
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

import numpy as np

from .. import splice as sp

REFUSED = (   # attribute, its neutral value, why not
    ("weighted_pos_pick", False, "--weighted-pos-pick needs a kmer_count-len_6.csv that no tool of the reference writes, and "
                                 "numpy's pairwise sums"),
    ("stitch_noise_std", 0, "--stitch-noise-std draws from a host random stream"),
    ("permute_win_size", 0, "--permute-win-size draws from a host random stream"),
    ("spike", False, "--spike (synthetic signal) is the `spike` command"),
)


def load_ctc(path, what):
    if not os.path.isdir(path):
        raise SystemExit("> error: %s is not a directory" % path)
    missing = [f for f in sp.FILES if not os.path.exists(os.path.join(path, f))]
    if missing:
        hint = " (`segment` writes breakpoints.npy)" if "breakpoints.npy" in missing else ""
        raise SystemExit("> error: the %s directory %s lacks %s%s" % (what, path, ", ".join(missing), hint))
    return tuple(np.load(os.path.join(path, f), mmap_mode="r" if f == "chunks.npy" else None) for f in sp.FILES)


def main(args, make_run=None):
    """make_run(library) -> the batch call that stands in for the device (tests); default: the device."""
    if args.stitch_mode != "per_kmer":
        raise SystemExit("> error: --stitch-mode %s is not offered: only per_kmer runs on the device" % args.stitch_mode)
    for name, neutral, why in REFUSED:
        if getattr(args, name) != neutral:
            raise SystemExit("> error: %s" % why)
    if args.ubs not in ("X", "Y", "XY"):
        raise SystemExit("> error: --ubs takes X, Y or XY")
    outputs = [os.path.join(args.out_dir, f) for f in sp.FILES + ("splice_stats.csv",)]
    if any(os.path.exists(f) for f in outputs) and not args.overwrite:
        raise SystemExit("> error: %s already holds output files; pass --overwrite to replace them" % args.out_dir)
    dna = load_ctc(args.dna_ctc_dir, "DNA")
    xna = load_ctc(args.xna_ctc_dir, "XNA")
    t0 = time.perf_counter()
    try:
        library = sp.build_library(*xna)
        if not len(library.info):
            raise ValueError("XNA: no read gives a candidate (an unnatural base more than five bases from either end, k-mers of "
                             "at most %d samples)" % sp.MAX_KMER_CNT)
        t1 = time.perf_counter()
        timings = {}
        chunks, targets, ok, inserted = sp.splice(*dna, library, ubs=args.ubs, prop_ubs=args.prop_ubs, var_prop_ubs=args.var_prop_ubs,
                                                  cand_sample_size=args.cand_sample_size, pad=args.ub_pad, seed=args.seed,
                                                  batch=args.batchsize, device=args.device,
                                                  run=None if make_run is None else make_run(library), timings=timings)
    except ValueError as e:
        raise SystemExit("> error: %s" % e)
    os.makedirs(args.out_dir, exist_ok=True)
    np.save(outputs[0], chunks.astype(np.float16))
    np.save(outputs[1], targets)
    np.save(outputs[2], np.asarray(dna[2]))
    np.save(outputs[3], np.asarray(dna[3]))
    with open(outputs[4], "w") as fh:
        fh.write("index,success,inserted\n")
        for c in range(len(ok)):
            fh.write("%d,%d,%d\n" % (c, int(ok[c]), int(inserted[c])))
    sys.stderr.write("> library: %d rows of %d reads, %d samples, built in %.2f s\n"
                     % (len(library.info), len(set(r[4] for r in library.info)), library.pool.size, t1 - t0))
    sys.stderr.write("> %d chunks in %.2f s (device calls %.2f s): %d unnatural bases inserted; %d chunks kept unchanged because "
                     "nothing could be inserted\n" % (len(ok), time.perf_counter() - t1, timings["device"], int(inserted.sum()),
                                                      int((~ok).sum())))
    return chunks, targets, ok, inserted


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("dna_ctc_dir", help="ctc-data directory of the chunks that receive unnatural bases (with breakpoints.npy)")
    parser.add_argument("xna_ctc_dir", help="ctc-data directory of the XNA chunks the signal is cut from (with breakpoints.npy)")
    parser.add_argument("out_dir", help="ctc-data directory to write")
    parser.add_argument("--ubs", default="XY", type=str, help="unnatural bases to insert: X, Y or XY")
    parser.add_argument("--prop-ubs", default=0, type=float, help="proportion of bases to become unnatural (0.01 = 1%%)")
    parser.add_argument("--var-prop-ubs", default=None, type=float, help="draw the proportion per chunk from prop-ubs +- this")
    parser.add_argument("--stitch-mode", default="per_kmer", choices=["per_kmer", "per_slice", "mixed"], type=str)
    parser.add_argument("--cand-sample-size", default=10, type=int,
                        help="candidates sampled per k-mer before the one of the closest length is taken")
    parser.add_argument("--ub-pad", default=5, type=int, help="bases kept free around an inserted unnatural base")
    parser.add_argument("--seed", default=2012, type=int, help="seed of the draws")
    parser.add_argument("--batchsize", default=4096, type=int, help="chunks per device call")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--overwrite", action="store_true", help="replace existing output files")
    parser.add_argument("--weighted-pos-pick", dest="weighted_pos_pick", action="store_true", help="refused")
    parser.add_argument("--stitch-noise-std", default=0, type=float, help="refused unless 0")
    parser.add_argument("--permute-win-size", default=0, type=int, help="refused unless 0")
    parser.add_argument("--spike", action="store_true", help="refused")
    return parser
