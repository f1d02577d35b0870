"""
`python -m xna_basecaller_amd segment CTC_DIR` == the reference's `src/tools/dtw_segmentation.py CTC_DIR`: DTW signal
segmentation of a ctc-data directory (chunks.npy, references.npy, reference_lengths.npy) into breakpoints.npy -- per
reference base the sample index where its signal ends.  The alignment runs on the device (xb_dtw_segment); `-n` (the naive
split) needs none.  The reference's --parallel / --n_proc / --pool_chunksize spread its host DTW over processes and have no
counterpart here.
"""
import os
import sys
import time
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

import numpy as np

from .. import segment as seg

DEFAULT_MODEL = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "data",
                             "r9.4_450bps.nucleotide.6mer.XNA-Px_Ds.template.model")


def output_name(naive, suffix):
    name = "breakpoints-naive" if naive else "breakpoints"
    return name + (".npy" if suffix is None else "-%s.npy" % suffix)


def main(args):
    if args.ref_rep < 1:
        raise SystemExit("> error: --ref_rep must be at least 1")
    if args.window_size is not None and args.window_size < 0:
        raise SystemExit("> error: --window_size must not be negative")
    if args.ubs_map is not None and (len(args.ubs_map) != 2 or any(c not in "ACGT" for c in args.ubs_map)):
        raise SystemExit("> error: --ubs_map takes two natural bases, the first for X and the second for Y (e.g. AT)")
    if not os.path.isdir(args.ctc_dir):
        raise SystemExit("> error: %s is not a directory" % args.ctc_dir)
    path = os.path.join(args.ctc_dir, output_name(args.naive, args.suffix))
    sys.stderr.write("> output file: %s\n" % path)
    if os.path.exists(path) and not args.overwrite:
        sys.stderr.write("[WARNING] Skipping because output file already exist:\n%s\n" % path)
        return None
    chunks = np.load(os.path.join(args.ctc_dir, "chunks.npy"), mmap_mode="r")
    targets = np.load(os.path.join(args.ctc_dir, "references.npy"))
    lengths = np.load(os.path.join(args.ctc_dir, "reference_lengths.npy"))
    if args.naive:
        bkps, ok = seg.naive_segment(chunks.shape[-1], targets, lengths)
    else:
        model = args.ref_filepath if args.ref_filepath is not None else DEFAULT_MODEL
        if not os.path.exists(model):
            raise SystemExit("> error: no k-mer pore model at %s: pass one with -r (the reference's "
                             "r9.4_450bps.nucleotide.6mer.XNA-Px_Ds.template.model is not shipped)" % model)
        poremodel = seg.load_kmer_poremodel(model)
        timings = {}
        t0 = time.perf_counter()
        try:
            bkps, ok = seg.segment(chunks, targets, lengths, poremodel, ref_rep=args.ref_rep, window_size=args.window_size,
                                   ubs_map=args.ubs_map, seed=args.seed, batch=args.batchsize, workers=args.workers,
                                   device=args.device, timings=timings)
        except ValueError as e:
            raise SystemExit("> error: %s" % e)
        sys.stderr.write("> %d chunks in %.2f s: device calls %.2f s, reference levels %.2f s on %d threads (waited %.2f s for them); "
                         "%d chunks failed and got the naive split\n" % (len(ok), time.perf_counter() - t0, timings["device"],
                                                                         timings["levels"], args.workers, timings["levels_wait"],
                                                                         int((~ok).sum())))
    sys.stderr.write("Saving file: %s\n" % path)
    np.save(path, bkps)
    return bkps, ok


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("ctc_dir", help="ctc-data directory for which breakpoints.npy is generated")
    parser.add_argument("-r", "--ref_filepath", default=None, help="k-mer pore model (kmer, level_mean, level_stdv); required "
                        "unless one is installed at %s" % DEFAULT_MODEL)
    parser.add_argument("-R", "--ref_rep", default=3, type=int, help="repeat of every level (the least samples per base)")
    parser.add_argument("-u", "--ubs_map", default=None, type=str, help="natural bases to read X and Y as, e.g. AT: X=A Y=T")
    parser.add_argument("-S", "--suffix", default=None, type=str, help="suffix of the breakpoints file")
    parser.add_argument("-n", "--naive", action="store_true", help="naive segmentation: chunksize / length samples for every base")
    parser.add_argument("-w", "--window_size", default=None, type=int, help="slanted-band half-width, in mean samples per base")
    parser.add_argument("--seed", default=25, type=int, help="seed of the noise in the level normalisation")
    parser.add_argument("--overwrite", action="store_true", help="replace an existing output file")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--batchsize", default=1024, type=int, help="chunks per device call")
    parser.add_argument("--workers", default=4, type=int, help="host threads that build the reference levels ahead of the device")
    return parser
