"""
`python -m xna_basecaller_amd synth CTC_DIR OUT_DIR -r KMER.model --ubs XY --prop-ubs 0.1`: the reference's fully synthetic XNA
chunks (`bonito train --spike --fully_synth`, ub-bonito/bonito/spike_chunks.py: sim_target; the -Z runs of its training recipe)
as a tool of its own.  The positions and unnatural bases are chosen as `spike` chooses them; then every chunk's signal is
re-synthesised on the device (xb_synth_chunks) from its spiked labels and its breakpoints -- one k-mer per base, held for the
samples the base had, normalised by the med / mad of the spiked labels' squiggle -- and nothing of the measured signal is
kept.  OUT_DIR is a ctc-data directory that `evaluate`, `segment` and `bonito train --directory` read.  The arguments are
`spike`'s, which are `bonito train`'s (cli/train.py:218-273).
"""
import os
import sys
import time
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

import numpy as np

from .. import spike as sk
from .splice import load_ctc

REFUSED = (   # attribute, its neutral value, why not
    ("equal_kmer_reps", False, "--equal-kmer-reps is not offered: a base is held for the samples its breakpoints give it"),
    ("legacy_pos", False, "--legacy-pos (the count of positions of the first experiments) is not offered"),
)


def main(args, make_run=None):
    """make_run(model) -> the batch call that stands in for the device (tests); default: the device."""
    for name, neutral, why in REFUSED:
        if getattr(args, name) != neutral:
            raise SystemExit("> error: %s" % why)
    if args.ubs not in ("X", "Y", "XY", "N"):
        raise SystemExit("> error: --ubs takes X, Y, XY or N")
    outputs = [os.path.join(args.out_dir, f) for f in sk.FILES + ("synth_stats.csv",)]
    if any(os.path.exists(f) for f in outputs) and not args.overwrite:
        raise SystemExit("> error: %s already holds output files; pass --overwrite to replace them" % args.out_dir)
    if not os.path.isfile(args.reference):
        raise SystemExit("> error: the k-mer model %s is not a file" % args.reference)
    dna = load_ctc(args.ctc_dir, "ctc-data")
    t0 = time.perf_counter()
    try:
        sk.parse_std_dist(args.std_dist)
        model = sk.load_model(args.reference)
        t1 = time.perf_counter()
        timings = {}
        chunks, targets, spiked, med, mad = sk.synth(*dna, model, ubs=args.ubs, prop_ubs=args.prop_ubs, var_prop_ubs=args.var_prop_ubs,
                                                     pad=args.ub_pad, std_dist=args.std_dist, noise_std=args.noise_std,
                                                     variable_noise=args.variable_noise, seed=args.seed, batch=args.batchsize,
                                                     device=args.device, run=None if make_run is None else make_run(model),
                                                     timings=timings)
    except ValueError as e:
        raise SystemExit("> error: %s" % e)
    os.makedirs(args.out_dir, exist_ok=True)
    np.save(outputs[0], chunks.astype(np.float16))
    np.save(outputs[1], targets)
    np.save(outputs[2], np.asarray(dna[2]))
    np.save(outputs[3], np.asarray(dna[3]))            # exact: a base keeps its samples
    with open(outputs[4], "w") as fh:
        fh.write("index,spiked,med,mad\n")
        for c in range(len(spiked)):
            fh.write("%d,%d,%r,%r\n" % (c, int(spiked[c]), float(med[c]), float(mad[c])))
    sys.stderr.write("> model: %d k-mers, read in %.2f s\n" % (int(np.isfinite(model[0]).sum()), t1 - t0))
    sys.stderr.write("> %d chunks in %.2f s (device calls %.2f s): every chunk synthesised, %d positions spiked; %d chunks without "
                     "an unnatural base because no base was free\n" % (len(spiked), time.perf_counter() - t1, timings["device"],
                                                                       int(spiked.sum()), int((spiked == 0).sum())))
    return chunks, targets, spiked, med, mad


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("ctc_dir", help="ctc-data directory of the chunks to synthesise (with breakpoints.npy)")
    parser.add_argument("out_dir", help="ctc-data directory to write")
    parser.add_argument("-r", "--reference", required=True, help="k-mer pore model (tab-separated: kmer, level_mean, level_stdv)")
    parser.add_argument("--ubs", default="XY", type=str, help="unnatural bases to insert: X, Y, XY, or N to synthesise the DNA as it is")
    parser.add_argument("--prop-ubs", default=0, type=float, help="proportion of bases to become unnatural (0.01 = 1%%)")
    parser.add_argument("--var-prop-ubs", default=None, type=float, help="draw the proportion per chunk from prop-ubs +- this")
    parser.add_argument("--ub-pad", default=5, type=int, help="bases kept free around a spiked base")
    parser.add_argument("--std-dist", default="uniform", type=str,
                        help="level noise: uniform, truncnorm or truncnorm_shift_<len>_<range>")
    parser.add_argument("--noise-std", default=0, type=float, help="std of the truncated normal noise added to the squiggle")
    parser.add_argument("--variable-noise", action="store_true", help="draw the noise std per chunk from 0 .. noise-std")
    parser.add_argument("--seed", default=2012, type=int, help="seed of the draws")
    parser.add_argument("--batchsize", default=4096, type=int, help="chunks per device call")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--overwrite", action="store_true", help="replace existing output files")
    parser.add_argument("--equal-kmer-reps", dest="equal_kmer_reps", action="store_true", help="refused")
    parser.add_argument("--legacy-pos", dest="legacy_pos", action="store_true", help="refused")
    return parser
