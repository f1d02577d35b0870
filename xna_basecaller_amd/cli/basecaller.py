"""
`bonito basecaller`-compatible command line (ub-bonito/bonito/cli/basecaller.py:24-196): same positional
arguments, flags, defaults and stderr lines; FASTQ (or, redirected to `*.sam`, unaligned SAM text) on stdout,
`<stdout-stem>_summary.tsv` beside it.

Differences, all outside the hot path: reads come from `*.xsig.npz` signal bundles (no HDF5/VBZ reader in
this image, see reads.py); --modified-bases is rejected (remora is not on the north-star path); --save-ctc (with
--reference) cuts every read into chunks, basecalls, maps and labels them on the device (xb_ctc_chunks) and writes a
ctc-data directory beside stdout (io.CTCWriter) -- it refuses --revcomp, --qscores, --ub-probs, --paf, more than one rank,
and a library with unnatural positions under a model that cannot call them; --reference FASTA maps every call to a
TEMPLATE LIBRARY on the device (aligner.py: exhaustive alignment, this package's own contract, not minimap2) and, as in
the reference, makes SAM the default output;
--paf PATH (an extension) writes the mappings as PAF beside it; --ub-report PREFIX (an extension) tallies the mapped calls'
per-position UB accuracy on the device (xb_ub_tally) and writes the reference's analyze_paf.py figures, with --max-bc-dist N
only of the calls that carry their template's barcode within N edits (xb_barcode_dist, analyze_paf.py -d); under torchrun (WORLD_SIZE > 1) reads are sharded over the
ranks and gathered to rank 0 over RCCL before writing.  Extension: --qscores writes the Viterbi decode's device
qualities (xb_decode_q) in place of the reference's placeholder 'O'; --ub-probs adds per-base probabilities of every
letter outside A, C, G, T as `u<letter>:B:C` tags (xb_decode_ub); without them the output is unchanged.
"""
import os
import sys
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from datetime import timedelta
from time import perf_counter

import numpy as np

from .. import dist as xdist
from ..io import Writer, biofmt
from ..reads import get_read_groups, get_reads
from ..util import column_to_set, init, load_model, load_symbol


READ_FIELDS = ("read_id", "run_id", "filename", "channel", "mux", "start", "duration", "template_start",
               "template_duration")


class _CalledRead:
    """What the writer needs of a read that was basecalled on another rank: its metadata and length, not its signal."""

    def __init__(self, fields, tags, n_samples):
        for k, v in zip(READ_FIELDS, fields):
            setattr(self, k, v)
        self._tags = tags
        self.signal = np.broadcast_to(np.float32(0), (n_samples,))     # len() only; no memory behind it

    def tagdata(self):
        return self._tags


def _gathered_results(results, loader, rank, world, window=256):
    """
    Multi-GPU: every rank basecalls its shard (reads i % world == rank); rank 0 receives (index, metadata, sequence)
    of all ranks in windows of `window` reads per rank and yields them in global read order, so nothing but metadata
    and called strings is kept, output starts while later windows are still being basecalled, and the collective is
    entered the same number of times by every rank.  A rank that fails keeps entering the remaining collectives with
    an error marker (its peers are never left blocked), then re-raises; rank 0 raises once it has seen the marker.
    """
    import torch.distributed as tdist
    n_windows = (loader.total + window * world - 1) // (window * world) if loader.total else 0
    it = iter(results)
    failure = None
    held = None
    for w in range(n_windows):
        hi = (w + 1) * window * world                   # global indices below `hi` belong to this window
        batch = []
        while failure is None:
            try:
                item = held if held is not None else next(it)
                held = None
            except StopIteration:
                break
            except BaseException as e:                   # noqa: BLE001 -- carried to rank 0, re-raised below
                failure = e
                break
            read, res = item
            if read.index >= hi:
                held = item
                break
            batch.append((read.index, tuple(getattr(read, k) for k in READ_FIELDS), read.tagdata(), len(read.signal),
                          res["sequence"], res["qstring"], res.get("mods", []), res.get("mapping", False)))
        payload = ("error", repr(failure)) if failure is not None else ("ok", batch)
        gathered = [None] * world if rank == 0 else None
        tdist.gather_object(payload, gathered, dst=0)
        if rank == 0 and failure is None:
            bad = [p[1] for p in gathered if p[0] == "error"]
            if bad:
                # keep entering the remaining collectives (the other ranks do), raise at the end
                failure = RuntimeError("a rank failed while basecalling: %s" % "; ".join(bad))
                continue
            merged = sorted((rec for p in gathered for rec in p[1]), key=lambda rec: rec[0])
            for _, fields, tags, n_samples, seq, qstring, mods, mapping in merged:
                res = {"sequence": seq, "qstring": qstring}
                if mods:
                    res["mods"] = mods
                if mapping is not False:                 # --reference: every rank mapped its own reads
                    res["mapping"] = mapping
                yield _CalledRead(fields, tags, n_samples), res
    if failure is not None:
        raise failure


def ub_probs_refusal(model):
    """Why `--ub-probs` cannot run on `model` (a message), or None: the letter probabilities come from the Viterbi decode,
    and they are reported for the letters outside A, C, G, T only."""
    from ..crf.basecall import ub_letters
    if not model.encoder[-1].expand_blanks:
        return "--ub-probs needs the Viterbi decode; this model takes the beam search"
    if not ub_letters(model):
        return "--ub-probs reports letters outside A, C, G, T; the alphabet %s has none" % "".join(model.alphabet[1:])
    return None


UB_PLUS, UB_MINUS = 5, 6        # the labels `--save-ctc` gives a template's unnatural position: the reference's X and Y


def save_ctc_refusal(args, world=1, labels=None, library=None):
    """Why `--save-ctc` cannot run with these arguments (the message, without the "> " prefix), or None.  labels: the
    model's alphabet when it could be read; library: the template letters (bytes) when the FASTA could be read."""
    if not args.reference:
        return "a reference is needed to output ctc training data"
    for flag, name in ((args.revcomp, "--revcomp"), (args.qscores, "--qscores"), (args.ub_probs, "--ub-probs"),
                       (args.paf, "--paf")):
        if flag:
            return "error: --save-ctc writes training chunks as they were called; %s does not apply to it" % name
    if world > 1:
        return "error: --save-ctc runs on one GPU (WORLD_SIZE is %d): the chunks' signals are not gathered across ranks" % world
    if labels is not None and library is not None and len(labels) <= UB_MINUS and \
            any(c not in b"ACGTacgt" for c in library):
        return ("error: %s has letters outside A, C, G, T, which --save-ctc labels %d and %d; the model's alphabet %s has "
                "only %d symbols" % (args.reference, UB_PLUS, UB_MINUS, "".join(labels), len(labels)))
    return None


def _save_ctc_early_refusal(args, world):
    """save_ctc_refusal before anything touches the GPU, with whatever of the model's config and the FASTA can be read
    (a missing model or reference is reported further down, where it always was)."""
    labels = library = None
    try:
        from .. import toml_lite
        from ..util import _model_dir
        labels = toml_lite.load(os.path.join(_model_dir(args.model_directory), "config.toml"))["labels"]["labels"]
    except (OSError, KeyError, ValueError):
        pass
    try:
        from ..aligner import read_fasta
        library = "".join(s for _, s in read_fasta(args.reference)).encode("ascii", "replace") if args.reference else None
    except OSError:
        pass
    return save_ctc_refusal(args, world, labels, library)


def ub_report_refusal(args, world=1):
    """Why `--ub-report` cannot run with these arguments (the message, without the "> " prefix), or None."""
    if not args.ub_report:
        return None
    if not args.reference:
        return "error: --ub-report tallies the mappings of --reference"
    if world > 1:
        return "error: --ub-report runs on one GPU (WORLD_SIZE is %d): the tallies are not gathered across ranks" % world
    if args.save_ctc:
        return "error: --ub-report reports on whole reads; --save-ctc maps chunks"
    return None


def max_bc_dist_refusal(args):
    """Why `--max-bc-dist` cannot run with these arguments (the message, without the "> " prefix), or None."""
    if args.max_bc_dist is None:
        return None
    if not args.ub_report:
        return "error: --max-bc-dist filters the reads of --ub-report by barcode distance; there is no report to filter"
    if args.max_bc_dist < 0 or args.barcode_start < 0 or not 1 <= args.barcode_len <= 64 or not 0 <= args.barcode_relax <= 8:
        return ("error: --max-bc-dist %d --barcode-start %d --barcode-len %d --barcode-relax %d: distance and start must not be "
                "negative, the barcode has 1 .. 64 letters, 0 .. 8 windows to either side"
                % (args.max_bc_dist, args.barcode_start, args.barcode_len, args.barcode_relax))
    return None


def reader_procs(world=1):
    """Reader workers of this rank: the reference's 8 (cli/basecaller.py:107-111) when the host has them to give -- the cores
    this process may run on, divided by the ranks that share the node (LOCAL_WORLD_SIZE under torchrun, else the world size),
    one core per rank left for its own pipeline threads; XB_READER_PROCS overrides.  8 ranks x 8 workers on a 64-core node
    would otherwise put 72 busy processes on 64 cores and slow every rank's reader (host budget)."""
    env = os.environ.get("XB_READER_PROCS", "")
    if env:
        return max(1, int(env))
    cores = len(os.sched_getaffinity(0)) if hasattr(os, "sched_getaffinity") else (os.cpu_count() or 1)
    local = max(1, int(os.environ.get("LOCAL_WORLD_SIZE", world) or 1))
    return max(1, min(8, cores // local - 1))


def main(args):
    if args.read_ids is not None and not os.path.isfile(args.read_ids):
        raise FileNotFoundError(args.read_ids)
    # the reader pool (8 worker processes, cli/basecaller.py:107-111) is forked BEFORE anything touches the GPU: the shard
    # comes from torchrun's environment alone, and the process group (whose nccl backend selects the device, i.e.
    # initialises HIP and starts runtime threads) is only joined once the pool exists.  Under torchrun every rank only
    # ever loads its own shard of the reads.
    rank, world = xdist.env_rank_world()
    why = ub_report_refusal(args, world) or max_bc_dist_refusal(args)
    if why is not None:
        sys.stderr.write("> %s\n" % why)
        exit(1)
    if args.save_ctc:
        why = _save_ctc_early_refusal(args, world)
        if why is not None:
            sys.stderr.write("> %s\n" % why)
            exit(1)
    n_proc = reader_procs(world)
    reads = get_reads(args.reads_directory, n_proc=n_proc, recursive=args.recursive,
                      read_ids=column_to_set(args.read_ids), skip=args.skip, limit=args.max_reads,
                      shard=(rank, world) if world > 1 else None)
    rank, world = xdist.init_from_env()

    init(args.seed, args.device)
    device = args.device
    if world > 1 and device == "cuda":
        device = "cuda:%d" % int(os.environ.get("LOCAL_RANK", rank))

    sys.stderr.write(f"> loading model {args.model_directory}\n")
    try:
        model = load_model(args.model_directory, device, weights=int(args.weights), chunksize=args.chunksize,
                           overlap=args.overlap, batchsize=args.batchsize, quantize=args.quantize,
                           use_koi=args.use_koi)
    except FileNotFoundError:
        sys.stderr.write(f"> error: failed to load {args.model_directory}\n")
        exit(1)

    if args.verbose:
        sys.stderr.write(f"> model basecaller params: {model.config['basecaller']}\n")
        sys.stderr.write("> decode algorithm: %s\n" % ("Viterbi" if model.encoder[-1].expand_blanks else "Beam Search"))
        sys.stderr.write(f"> read_ids: {args.read_ids}\n")

    basecall = load_symbol(args.model_directory, "basecall")

    if args.modified_bases or args.modified_base_model:
        sys.stderr.write("> error: --modified-bases is not part of the MI355X path\n")
        exit(1)
    if args.paf and not args.reference:
        sys.stderr.write("> error: --paf writes the mappings of --reference\n")
        exit(1)
    aligner = None
    if args.reference:
        # a template library, mapped exhaustively on the device (aligner.py) -- on the model's own context, so that the
        # mapper's launches queue on the basecaller's stream instead of competing with its persistent kernels
        from ..aligner import TemplateAligner
        sys.stderr.write("> loading reference\n")
        try:
            aligner = TemplateAligner.from_config(args.reference, model.config, device=getattr(model, "_device", 0),
                                                  context=lambda: getattr(model, "_ctx", None))
        except (OSError, ValueError) as e:
            sys.stderr.write("> failed to load/build index: %s\n" % e)
            exit(1)
    if args.ub_probs:
        why = ub_probs_refusal(model)
        if why is not None:
            sys.stderr.write("> error: %s\n" % why)
            exit(1)
    fmt = biofmt(aligned=aligner is not None)
    sys.stderr.write(f"> outputting {fmt.aligned} {fmt.name}\n")
    if fmt.name not in ("fastq", "sam"):
        sys.stderr.write("> error: FASTQ and SAM text output are implemented (redirect stdout to *.fastq or *.sam); "
                         "BAM / CRAM need htslib\n")
        exit(1)
    # SAM: the header carries one @RG line per (run, model) of the selected reads -- metadata only (cli/basecaller.py:100-106)
    groups = []
    if fmt.name != "fastq" and rank == 0:
        groups = get_read_groups(args.reads_directory, args.model_directory, recursive=args.recursive,
                                 read_ids=column_to_set(args.read_ids), skip=args.skip, n_proc=n_proc)

    if args.save_ctc:
        return _save_ctc(args, model, aligner, reads, fmt, groups, n_proc)

    # --qscores (an extension): the Viterbi decode's device qualities instead of the reference's 'O' placeholders
    extra = {"qscores": True} if args.qscores else {}
    if args.ub_probs:                   # --ub-probs (an extension): per-base letter probabilities as u<letter>:B:C tags
        extra["ub_probs"] = True
    results = basecall(model, reads, reverse=args.revcomp,
                       batchsize=model.config["basecaller"]["batchsize"],
                       chunksize=model.config["basecaller"]["chunksize"],
                       overlap=model.config["basecaller"]["overlap"], **extra)

    if args.ub_report:                  # --ub-report (an extension): every mapper call's rows also go through xb_ub_tally
        from ..ubreport import Report
        demux = None                    # --max-bc-dist: a mapped call counts only when it carries its template's barcode
        if args.max_bc_dist is not None:
            demux = (args.max_bc_dist, args.barcode_start, args.barcode_len, args.barcode_relax)
        aligner.ub_report = Report(aligner.names, aligner.templates, demux=demux)
    if aligner is not None:             # every rank maps its own reads, before the gather
        from ..aligner import align_map
        results = align_map(aligner, results)

    t0 = perf_counter()
    if world > 1:
        results = _gathered_results(results, reads, rank, world)
        if rank != 0:
            for _ in results:                           # drives the local pipeline and the collectives
                pass
            return

    paf = open(args.paf, "w") if args.paf else None
    writer = Writer(fmt.mode, results, aligner=aligner, group_key=args.model_directory, groups=groups, paf=paf)
    writer.start()
    writer.join()
    if paf is not None:
        paf.close()
    if aligner is not None:
        aligner.close()
    if writer.error is not None:
        raise writer.error
    if args.ub_report:
        for path in aligner.ub_report.write(args.ub_report):
            sys.stderr.write("> ub report: %s\n" % path)
    duration = perf_counter() - t0
    num_samples = sum(num_samples for read_id, num_samples in writer.log)

    sys.stderr.write(f"> completed reads: {len(writer.log):0,d}\n")
    sys.stderr.write("> duration: %s\n" % timedelta(seconds=np.round(duration)))
    sys.stderr.write("> samples per second %.1E\n" % (num_samples / duration))
    if args.verbose:
        # beyond the reference's lines: what the device stage did -- chunks of chunksize samples, overlaps and stub chunks included
        # (the reference's metric above counts READ samples); tools/cli_e2e.py compares this rate with bench.py's
        chunks = getattr(model, "chunks_submitted", 0)
        sys.stderr.write("> duration (s): %.2f\n" % duration)
        sys.stderr.write("> reads per second: %.0f (reader workers: %d)\n" % (len(writer.log) / duration, n_proc))
        sys.stderr.write("> chunks basecalled: %d x %d samples = %.3E chunk samples per second\n"
                         % (chunks, model.config["basecaller"]["chunksize"], chunks * model.config["basecaller"]["chunksize"] / duration))
    sys.stderr.write("> done\n")


def _save_ctc(args, model, aligner, reads, fmt, groups, n_proc):
    """`--save-ctc` (cli/basecaller.py:116-129): every read cut into chunks of the model's chunksize, each chunk basecalled,
    mapped and labelled on the device (crf.basecall.basecall_ctc), the kept ones written as ctc-data (io.CTCWriter)."""
    from ..crf.basecall import basecall_ctc
    from ..io import CTCWriter
    from ..reads import read_chunks
    why = save_ctc_refusal(args, 1, model.alphabet, aligner.library)
    if why is not None:
        sys.stderr.write("> %s\n" % why)
        exit(1)
    run = model.config["basecaller"]
    chunks = (c for read in reads for c in read_chunks(read, chunksize=run["chunksize"], overlap=run["overlap"]))
    writer_kwargs = dict(min_coverage=args.min_coverage, min_accuracy=args.min_accuracy, ub_only=args.ub_only)
    sys.stderr.write(f"> writer_kwargs: {writer_kwargs}\n")
    results = basecall_ctc(model, aligner, chunks, batchsize=run["batchsize"], ub_plus=UB_PLUS, ub_minus=UB_MINUS, **writer_kwargs)
    t0 = perf_counter()
    writer = CTCWriter(fmt.mode, results, aligner=aligner, group_key=args.model_directory, ref_fn=args.reference, groups=groups,
                       ub_plus=UB_PLUS, ub_minus=UB_MINUS, **writer_kwargs)
    writer.start()
    writer.join()
    aligner.close()
    if writer.error is not None:
        raise writer.error
    duration = perf_counter() - t0
    num_samples = sum(num_samples for read_id, num_samples in writer.log)
    sys.stderr.write(f"> completed reads: {len(writer.log):0,d}\n")
    sys.stderr.write("> duration: %s\n" % timedelta(seconds=np.round(duration)))
    sys.stderr.write("> samples per second %.1E\n" % (num_samples / duration))
    sys.stderr.write("> done\n")


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("model_directory")
    parser.add_argument("reads_directory")
    parser.add_argument("--reference", help="FASTA of a template library: every call is mapped to it on the device (exhaustive "
                        "local alignment, both strands; libraries up to 2^20 letters, templates up to 4096)")
    parser.add_argument("--paf", help="with --reference: also write the mappings as PAF to this file; not in the reference CLI")
    parser.add_argument("--ub-report", metavar="PREFIX",
                        help="with --reference: per-position UB accuracy of the mapped calls, tallied on the device, as "
                             "PREFIX.csv, PREFIX-by_tar.csv, PREFIX-by_read.csv.gz and PREFIX-confusion_matrix.npy (the figures of "
                             "the reference's analyze_paf.py -p); not in the reference CLI")
    parser.add_argument("--max-bc-dist", type=int, default=None,
                        help="with --ub-report: count a mapped call only when its template's barcode lies within this many edits "
                             "of the call (the reference's analyze_paf.py -d: 5 for POC, 8 for CPLX); the summary gains demux and align")
    parser.add_argument("--barcode-start", type=int, default=25, help="with --max-bc-dist: where the barcode starts in every template")
    parser.add_argument("--barcode-len", type=int, default=24, help="with --max-bc-dist: letters of the barcode (1 .. 64)")
    parser.add_argument("--barcode-relax", type=int, default=3, help="with --max-bc-dist: windows tried to either side (0 .. 8)")
    parser.add_argument("--modified-bases", nargs="+")
    parser.add_argument("--modified-base-model")
    parser.add_argument("--read-ids")
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--seed", default=25, type=int)
    parser.add_argument("--weights", default="0", type=str)
    parser.add_argument("--skip", action="store_true", default=False)
    parser.add_argument("--save-ctc", action="store_true", default=False)
    parser.add_argument("--revcomp", action="store_true", default=False)
    parser.add_argument("--qscores", action="store_true", default=False,
                        help="Viterbi decode: per-base qualities computed on the device (path posteriors, calibrated by the "
                             "model's [qscore] scale / bias) instead of the placeholder 'O'; not in the reference CLI")
    parser.add_argument("--ub-probs", action="store_true", default=False,
                        help="Viterbi decode: per-base probability of every alphabet letter outside A, C, G, T, computed on "
                             "the device from the decode's posteriors, as u<letter>:B:C tags (1/256 bins); not in the "
                             "reference CLI")
    parser.add_argument("--recursive", action="store_true", default=False)
    quant_parser = parser.add_mutually_exclusive_group(required=False)
    quant_parser.add_argument("--quantize", dest="quantize", action="store_true")
    quant_parser.add_argument("--no-quantize", dest="quantize", action="store_false")
    quant_parser.add_argument("--no-use-koi", dest="use_koi", action="store_false")
    parser.set_defaults(quantize=None)
    parser.add_argument("--overlap", default=None, type=int)
    parser.add_argument("--chunksize", default=None, type=int)
    parser.add_argument("--batchsize", default=None, type=int,
                        help="chunks per device call; 512 and 1024 are the efficient sizes on MI355X (a recurrence launch serves "
                             "64-chunk groups, 8 or 16 at a time with a group on one XCD, up to 10 or 20 dealt over all XCDs: 513..640 "
                             "and 1025..1280 chunks cost up to 11 %% more per chunk, 641 chunks 25 %% more)")
    parser.add_argument("--max-reads", default=0, type=int)
    parser.add_argument("--min-accuracy", default=0.95, type=float)
    parser.add_argument("--min-coverage", default=0.90, type=float)
    parser.add_argument("--ub-only", action="store_true", default=False)
    parser.add_argument("-v", "--verbose", action="count", default=0)
    return parser
