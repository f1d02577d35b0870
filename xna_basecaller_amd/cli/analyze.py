"""
`python -m xna_basecaller_amd analyze LIB.fasta CALLS.paf -R CALLS.fastq` == the reference's `src/tools/analyze_paf.py -p`
for calls made earlier: per-position UB accuracy of the mappings of a PAF file (with cs:Z: tags, as `basecaller --paf` writes
them) against the template library.  Every cs string is turned back into the mapper's alignment columns on the host; the
per-read walk, the UB polish and the tallies run on the device (xb_ub_tally), the figures are ubreport's.  -d N keeps an
alignment only when the barcode of its template lies within N edits of the read where the alignment puts it, and of a read's
alignments those at its smallest distance (xb_barcode_dist on the device, the reference's two-step filter on the host); the
summary then carries demux and align.  The library FASTA stands in for the reference's XNA_refs table, so the barcode's place
comes from --barcode-start / --barcode-len (the reference's left_primer_len and barcode length: 25 / 24 for POC, 23 / 30 for
CPLX); -q has no counterpart here.
"""
import os
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser

from .. import ubreport


def output_prefix(paf, reads):
    """results_summ-<reads name> beside the PAF (analyze_paf.py:597-603)."""
    name = os.path.splitext(os.path.basename(reads))[0]
    if name.startswith("reads-"):
        name = name[6:]
    return os.path.join(os.path.dirname(paf), "results_summ-" + name)


def select(alignments, only_strand=None, ubs="XY"):
    """analyze_paf.py:652-658: -u X keeps strand F, -u Y strand R; -S names the strand itself."""
    if ubs != "XY":
        only_strand = {"X": "F", "Y": "R"}[ubs]
    if only_strand is None:
        return alignments
    want = -1 if only_strand.replace("+", "F").replace("-", "R") == "R" else 1
    return [a for a in alignments if a["strand"] == want]


def demux_setting(args):
    """(max_dist, bc_pos, bc_len, relax) of -d and its companions, None without -d."""
    if args.max_bc_dist is None:
        return None
    return (args.max_bc_dist, args.barcode_start, args.barcode_len, args.barcode_relax)


def main(args):
    for path in (args.library, args.paf, args.reads_filepath):
        if not os.path.isfile(path):
            raise SystemExit("> error: no file %s" % path)
    from ..aligner import read_fasta
    records = read_fasta(args.library)
    if not records or any(not s for _, s in records):
        raise SystemExit("> error: %s holds no template" % args.library)
    try:
        alignments = ubreport.read_paf(args.paf)
        sequences = ubreport.read_sequences(args.reads_filepath)
    except ValueError as e:
        raise SystemExit("> error: %s" % e)
    sys.stderr.write("> paf contains %d reads (%d alignments)\n" % (len({a["read_id"] for a in alignments}), len(alignments)))
    sys.stderr.write("> number of reads on file: %d\n" % len(sequences))
    demux = demux_setting(args)
    if demux is None:
        alignments = select(alignments, args.only_strand, args.ubs)
    if not alignments:
        sys.stderr.write("> no read left to analyze performance, exiting\n")
        return None
    from .. import _lib
    _lib.require_gpu()
    report = ubreport.Report([n for n, _ in records], [s for _, s in records], demux=demux)
    ctx = _lib.mapper_context(args.device)
    try:
        if demux is not None:           # the barcode filter comes before -S / -u, as in the reference
            alignments = ubreport.demux_paf(report, ctx, alignments, sequences, batch=args.batchsize)
            sys.stderr.write("> filtering by barcode distance, max: %d\n" % demux[0])
            sys.stderr.write("> remaining number of unique read ids: %d\n" % len(report.demuxed))
            alignments = select(alignments, args.only_strand, args.ubs)
        if alignments:
            ubreport.tally_paf(report, ctx, alignments, sequences, batch=args.batchsize)
    except (ValueError, _lib.XbError) as e:
        raise SystemExit("> error: %s" % e)
    finally:
        ctx.close()
    if not alignments:
        sys.stderr.write("> no read left to analyze performance, exiting\n")
        return None
    prefix = output_prefix(args.paf, args.reads_filepath)
    for path in report.write(prefix, by_tar=args.save_detailed_perf, by_read=args.save_perf_per_read,
                             confusion=args.save_confusion_matrix):
        sys.stderr.write("> saving file: %s\n" % path)
    row = report.summary()
    sys.stdout.write(",".join(row) + "\n" + ",".join(ubreport._fmt(v, "%.1f") for v in row.values()) + "\n")
    return report


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("library", help="FASTA of the template library the calls were mapped to")
    parser.add_argument("paf", help="PAF with cs:Z: tags (short form, or long form with '=')")
    parser.add_argument("-R", "--reads_filepath", required=True, help="the calls: FASTA or FASTQ, plain text")
    parser.add_argument("-S", "--only_strand", choices=["F", "R", "+", "-"], default=None)
    parser.add_argument("-u", "--ubs", choices=["X", "Y", "XY"], default="XY", help="X keeps strand F, Y keeps strand R")
    parser.add_argument("-d", "--max_bc_dist", type=int, default=None,
                        help="keep an alignment only when its template's barcode is within this many edits of the read "
                             "(the reference uses 5 for POC, 8 for CPLX)")
    parser.add_argument("--barcode-start", type=int, default=25, help="with -d: where the barcode starts in every template")
    parser.add_argument("--barcode-len", type=int, default=24, help="with -d: letters of the barcode (1 .. 64)")
    parser.add_argument("--barcode-relax", type=int, default=3, help="with -d: windows tried to either side (0 .. 8)")
    parser.add_argument("--save_confusion_matrix", action="store_true", default=False)
    parser.add_argument("--save_perf_per_read", action="store_true", default=False)
    parser.add_argument("-D", "--save_detailed_perf", action="store_true", default=False)
    parser.add_argument("--device", default=0, type=int)
    parser.add_argument("--batchsize", default=512, type=int, help="alignments per device call")
    return parser
