"""
Output side of the basecaller: FASTQ records on stdout and one summary row per read.

Written from the OUTPUT FORMAT the reference produces (ub-bonito/bonito/io.py), not from its code:

  * stdout format is chosen from the name stdout is redirected to (io.py:30-49): `*.fq` / `*.fastq` / a tty / a pipe
    mean FASTQ; `.sam` means SAM text: the header (io.py:87-112: @HD VN:1.5 SO:unknown ob:0.0.1, @PG basecaller with version
    and command line, the reads' @RG lines) and one UNALIGNED record per read (io.py:115-145 with mapping = False: flag 4,
    `*` reference / CIGAR, NM:i:0, then the same tags as the FASTQ header) -- the reference hands both to pysam
    (`AlignmentFile(fd, 'w', text=header)` / `AlignedSegment.fromstring`, io.py:391-401,432-437), whose SAM text mode prints the
    header text as it is and each record as its own line; pysam is in no image, so the text is written directly.  The
    reference's header also carries `@PG ID:aligner PN:minimap2 VN:<mappy version>` whether or not anything is aligned; here
    that line is written only when an aligner version is given (none exists: mappy is in no image), so an unaligned file does
    not claim an aligner; with `--reference` the line names this package's own mapper (PN:xnacall-map, aligner.py), never
    minimap2, and the records are aligned ones.  `.bam` / `.cram` need htslib: refused;
  * a FASTQ record is  "@<read_id> <tag>\\t<tag>...\\n<sequence>\\n+\\n<qstring>\\n"  (io.py:76-84) with the tags
    RG:Z:<run_id>_<model>  qs:i:<rounded mean q>  mx:i  ch:i  st:Z  rn:i  f5:Z  (io.py:412-419, fast5.py:118-128);
  * the summary is `<stdout stem>_summary.tsv` (`summary.tsv` on a tty or a pipe; io.py:148-155), tab separated with the
    CSV dialect of Python's csv.writer (CRLF line ends, minimal quoting), header
    filename read_id run_id channel mux start_time duration template_start template_duration
    sequence_length_template mean_qscore_template (io.py:158-170, 190-206); appended to if it already exists;
  * reads whose called sequence is empty are skipped with a warning (io.py:444-445); the writer keeps a
    (read_id, samples) log from which the CLI prints samples per second (cli/basecaller.py:153-161).
"""
import os
import sys
from collections import namedtuple
from logging import getLogger
from threading import Thread

import numpy as np

from .util import mean_qscore_from_qstring

logger = getLogger("bonito")
Format = namedtuple("Format", "aligned name mode")

SUMMARY_COLUMNS = ("filename", "read_id", "run_id", "channel", "mux", "start_time", "duration", "template_start",
                   "template_duration", "sequence_length_template", "mean_qscore_template")
# the columns an aligner adds (io.py:170-187)
ALIGNMENT_COLUMNS = ("alignment_genome", "alignment_genome_start", "alignment_genome_end", "alignment_strand_start",
                     "alignment_strand_end", "alignment_direction", "alignment_length", "alignment_num_aligned",
                     "alignment_num_correct", "alignment_num_insertions", "alignment_num_deletions",
                     "alignment_num_substitutions", "alignment_mapq", "alignment_strand_coverage", "alignment_identity",
                     "alignment_accuracy")
_MODES = {"fq": ("fastq", "wfq"), "fastq": ("fastq", "wfq"), "sam": ("sam", "w"), "bam": ("bam", "wb"),
          "cram": ("cram", "wc")}


def _stdout_target():
    """Path stdout points at, or None for a terminal / pipe / socket."""
    if sys.stdout.isatty():
        return None
    target = os.path.realpath("/dev/fd/1")
    return None if target.startswith("/proc") else target


def biofmt(aligned=False):
    """Output format implied by stdout's file name: Format(aligned|unaligned, fastq|sam|bam|cram, open mode)."""
    kind = "aligned" if aligned else "unaligned"
    fallback = ("sam", "w") if aligned else ("fastq", "wfq")
    target = _stdout_target()
    ext = target.rsplit(os.extsep, 1)[-1] if target else ""
    name, mode = _MODES.get(ext, fallback)
    return Format(kind, name, mode)


def summary_file():
    target = _stdout_target()
    return "summary.tsv" if target is None else os.path.splitext(target)[0] + "_summary.tsv"


def write_fastq(header, sequence, qstring, fd=sys.stdout, tags=None, sep="\t"):
    title = header if tags is None else "%s %s" % (header, sep.join(tags))
    fd.write("@%s\n%s\n+\n%s\n" % (title, sequence, qstring))


def write_fasta(header, sequence, fd=sys.stdout):
    fd.write(">%s\n%s\n" % (header, sequence))


SAM_SPEC = "0.0.1"          # the reference's __ont_bam_spec__ (io.py:27)


ALIGNER_NAME = "xnacall-map"    # the @PG PN of this package's template mapper (aligner.py); it is not minimap2


def sam_header(groups, sep="\t", version=None, argv=None, aligner_version=None, aligner_name="minimap2", aligner_ds="mappy"):
    """The SAM header text (io.py:87-112): @HD, @PG of the basecaller (PN:bonito -- the drop-in's program name -- with `version`
    and the command line `argv`), optionally the aligner's @PG (the reference's names by default; the Writer passes this
    package's mapper), then the read-group lines; lines joined by os.linesep, one trailing newline."""
    from . import __version__
    lines = [sep.join(["@HD", "VN:1.5", "SO:unknown", "ob:%s" % SAM_SPEC]),
             sep.join(["@PG", "ID:basecaller", "PN:bonito", "VN:%s" % (__version__ if version is None else version),
                       "CL:bonito %s" % " ".join(sys.argv[1:] if argv is None else argv)])]
    if aligner_version is not None:
        lines.append(sep.join(["@PG", "ID:aligner", "PN:%s" % aligner_name, "VN:%s" % aligner_version, "DS:%s" % aligner_ds]))
    return "%s\n" % os.linesep.join(lines + list(groups))


# minimap2's complement table (sketch.c `seq_comp_table`, what `mappy.revcomp` applies): the IUPAC codes in both cases, every
# other byte unchanged.  On the XNA alphabets that means X stays X and Y -- an IUPAC code -- becomes R; the reference calls
# mappy.revcomp on the called sequence as it is (io.py:133), so this is what its aligned records carry.  mappy is in no
# image: the table is restated, and the generator of tests/golden/sam.json uses the same restatement as its stand-in.
_COMP = {a: b for a, b in zip("ACGTUMRWSYKVHDBN", "TGCAAKYWSRMBDHVN")}
_COMP.update({a.lower(): b.lower() for a, b in list(_COMP.items())})
_COMP_TABLE = str.maketrans(_COMP)


def revcomp(sequence):
    """mappy.revcomp: reverse, then complement through minimap2's table."""
    return sequence[::-1].translate(_COMP_TABLE)


def sam_record(read_id, sequence, qstring, mapping=None, tags=None, sep="\t"):
    """One SAM record as text (io.py:115-145).  Unaligned (mapping false): flag 4, no reference, NM:i:0.  Aligned: `mapping` is
    a mappy.Alignment-shaped object (ctg, r_st, q_st, q_en, strand, mapq, cigar_str, NM, MD): flag 0 / 16, 1-based position,
    the CIGAR wrapped in the soft clips of the unaligned query ends (swapped on the reverse strand), the sequence reverse
    complemented on the reverse strand -- and the quality string left as it is, as the reference does.  The formatting is pinned
    by tests/golden/sam.json; `--reference` produces the mapping with this package's template mapper (aligner.Mapping)."""
    if mapping:
        tail = len(sequence) - mapping.q_en
        softclip = ["%sS" % mapping.q_st if mapping.q_st else "", mapping.cigar_str, "%sS" % tail if tail else ""]
        forward = mapping.strand == +1
        record = [read_id, 0 if forward else 16, mapping.ctg, mapping.r_st + 1, mapping.mapq,
                  "".join(softclip if forward else softclip[::-1]), "*", 0, 0,
                  sequence if forward else revcomp(sequence), qstring, "NM:i:%s" % mapping.NM, "MD:Z:%s" % mapping.MD]
    else:
        record = [read_id, 4, "*", 0, 0, "*", "*", 0, 0, sequence, qstring, "NM:i:0"]
    if tags is not None:
        record.extend(tags)
    return sep.join(map(str, record))


def _tsv_field(value):
    """One field in csv.writer's default dialect with a tab delimiter (quote only when needed, double the quotes)."""
    text = "" if value is None else str(value)
    if any(c in text for c in '\t"\r\n'):
        text = '"%s"' % text.replace('"', '""')
    return text


class SummaryTable:
    """Append-only TSV: the header is written when the file is new, otherwise the existing header's columns are kept."""

    def __init__(self, path, columns=SUMMARY_COLUMNS):
        self.path = str(path)
        self.columns = list(columns)
        fresh = not os.path.exists(self.path) or os.path.getsize(self.path) == 0
        if not fresh:
            with open(self.path, newline="") as fh:
                first = fh.readline().rstrip("\r\n")
            if first:
                self.columns = first.split("\t")
        self._fh = open(self.path, "a", newline="")
        self._pending = 0
        if fresh:
            self._line(self.columns)

    def _line(self, fields):
        self._fh.write("\t".join(_tsv_field(f) for f in fields) + "\r\n")

    def append(self, row):
        self._line([row.get(c, "-") for c in self.columns])
        self._pending += 1
        if self._pending > 100:
            self._fh.flush()
            self._pending = 0

    def close(self):
        self._fh.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def summary_row(read, seqlen, qscore, alignment=False):
    """One summary row (io.py:190-237).  alignment False: the eleven read columns.  A mapping: the reference's sixteen
    alignment columns with its arithmetic; None (an aligner ran, nothing aligned): its empty alignment row."""
    values = [read.filename, read.read_id, read.run_id, read.channel, read.mux, read.start, read.duration,
              read.template_start, read.template_duration, seqlen, qscore]
    if alignment:
        ins = sum(count for count, op in alignment.cigar if op == 1)
        dels = sum(count for count, op in alignment.cigar if op == 2)
        subs = alignment.NM - ins - dels
        length = alignment.blen
        matches = length - ins - dels
        correct = alignment.mlen
        forward = alignment.strand == +1
        values += [alignment.ctg, alignment.r_st, alignment.r_en,
                   alignment.q_st if forward else seqlen - alignment.q_en,
                   alignment.q_en if forward else seqlen - alignment.q_st,
                   "+" if forward else "-", length, matches, correct, ins, dels, subs, alignment.mapq,
                   (alignment.q_en - alignment.q_st) / seqlen, correct / matches, correct / length]
    elif alignment is None:
        values += ["*", -1, -1, -1, -1, "*", 0, 0, 0, 0, 0, 0, 0, 0.0, 0.0, 0.0]
    return dict(zip(SUMMARY_COLUMNS + ALIGNMENT_COLUMNS, values))


def write_paf(fd, read_id, seqlen, mapping):
    """One PAF line of a mapping: the twelve columns (query coordinates on the call as it was made) and the tags tp:A:P,
    s1:i:<score>, s2:i:<best other template's score>, cs:Z:<short cs>.  Nothing for an unmapped read, as minimap2."""
    if not mapping:
        return
    fields = [read_id, seqlen, mapping.q_st, mapping.q_en, "+" if mapping.strand == +1 else "-", mapping.ctg, mapping.ctg_len,
              mapping.r_st, mapping.r_en, mapping.mlen, mapping.blen, mapping.mapq, "tp:A:P", "s1:i:%d" % mapping.score,
              "s2:i:%d" % mapping.second, "cs:Z:%s" % mapping.cs]
    fd.write("\t".join(map(str, fields)) + "\n")


class Writer(Thread):
    """Drains the (read, result) iterator on its own thread: FASTQ (mode 'wfq') or SAM text (mode 'w', header first) to `fd`, a
    summary row and a log entry per read.  With an `aligner` (aligner.TemplateAligner; the results then carry 'mapping') the
    SAM records are aligned ones, the header names this package's mapper, the summary gains the alignment columns and `paf`
    (a text file object) receives a PAF line per mapped read.  Without one nothing changes."""

    def __init__(self, mode, iterator, aligner=None, fd=sys.stdout, duplex=False, ref_fn=None, groups=None,
                 group_key=None, summary=None, paf=None):
        super().__init__()
        if mode not in ("wfq", "w") or duplex:
            raise NotImplementedError("FASTQ (mode 'wfq') and SAM text (mode 'w') are on the MI355X path; BAM / CRAM need htslib")
        self.mode, self.fd, self.iterator = mode, fd, iterator
        self.aligner, self.paf = aligner, paf
        self.group_key = group_key
        self.groups = sorted(groups) if groups else []
        self.summary = summary
        self.log = []
        self.error = None

    def _emit(self, table, read, res):
        seq = res["sequence"]
        if not len(seq):
            logger.warning("> skipping empty sequence %s", read.read_id)
            return
        qstring = res.get("qstring", "*")
        mean_q = res.get("mean_qscore")
        if mean_q is None:
            mean_q = mean_qscore_from_qstring(qstring)
        tags = ["RG:Z:%s_%s" % (read.run_id, self.group_key), "qs:i:%d" % round(mean_q)]
        tags += list(read.tagdata()) + list(res.get("mods", []))
        if self.mode == "wfq":
            write_fastq(read.read_id, seq, qstring, fd=self.fd, tags=tags)
        else:
            self.fd.write(sam_record(read.read_id, seq, qstring, res.get("mapping", False), tags=tags) + "\n")
        if self.aligner is None:
            table.append(summary_row(read, len(seq), mean_q))
        else:
            table.append(summary_row(read, len(seq), mean_q, alignment=res.get("mapping")))
            if self.paf is not None:
                write_paf(self.paf, read.read_id, len(seq), res.get("mapping"))
        self.log.append((read.read_id, len(read.signal)))

    def run(self):
        try:
            columns = SUMMARY_COLUMNS if self.aligner is None else SUMMARY_COLUMNS + ALIGNMENT_COLUMNS
            with SummaryTable(self.summary or summary_file(), columns) as table:
                if self.mode == "w" and self.aligner is None:
                    self.fd.write(sam_header(self.groups))
                elif self.mode == "w":
                    from . import __version__
                    self.fd.write(sam_header(self.groups, aligner_version=__version__, aligner_name=ALIGNER_NAME,
                                             aligner_ds="exhaustive template alignment on the device"))
                for read, res in self.iterator:
                    self._emit(table, read, res)
        except BaseException as e:  # surfaced by the CLI after join()
            self.error = e
            raise


# ---- `--save-ctc`: ctc-data from filtered, labelled chunks (io.py:448-585) ---------------------------------------------
FAILED_SEQ, FAILED_MAP, SKIPPED_NON_UB, FAILED_ACC, FAILED_COV = 1, 2, 4, 8, 16      # the verdict bits of xb_ctc_targets
FILTER_COUNTERS = ("count_failed_seq", "count_failed_map", "count_failed_acc", "count_failed_cov", "count_failed_both",
                   "non_ubs_skipped")
_STRAND_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def ctc_verdict(sequence, mapping, refseq, min_accuracy=0.95, min_coverage=0.90, ub_only=False, ub_plus=5, ub_minus=6):
    """The reference's per-chunk decision (io.py:495-540) on the host, for results that carry no device verdict: ->
    (verdict byte as xb_ctc_targets writes it, label list or None).  refseq(ctg, r_st, r_en) returns the template letters;
    every letter outside A, C, G, T counts as the reference's 'N'."""
    verdict = (FAILED_SEQ if len(sequence) == 0 else 0) | (FAILED_MAP if mapping is None else 0)
    if verdict:
        return verdict, None
    cov = (mapping.q_en - mapping.q_st) / len(sequence)
    acc = mapping.mlen / mapping.blen
    letters = refseq(mapping.ctg, mapping.r_st, mapping.r_en)
    if ub_only and all(c in "ACGTacgt" for c in letters):
        return SKIPPED_NON_UB, None
    verdict = (FAILED_ACC if acc < min_accuracy else 0) | (FAILED_COV if cov < min_coverage else 0)
    if verdict:
        return verdict, None
    if mapping.strand == -1:
        letters = letters[::-1].translate(_STRAND_COMP)
    ub = ub_minus if mapping.strand == -1 else ub_plus
    return 0, ["ACGT".find(c.upper()) + 1 or ub for c in letters]


def typical_indices(x, n=2.5):
    """cli/convert.py:80-83: the indices whose value lies STRICTLY inside mean +- n standard deviations.  Quirk kept: when all
    values are equal the deviation is 0, both bounds are the mean itself, and nothing is kept."""
    x = np.asarray(x)
    mu, sd = np.mean(x), np.std(x)
    idx, = np.where((mu - n * sd < x) & (x < mu + n * sd))
    return idx


def filter_stats_text(counts):
    """`pandas.Series(counts).to_csv()` without pandas: the header `,0`, then one `name,value` line per counter."""
    return ",0\n" + "".join("%s,%d\n" % (k, counts[k]) for k in FILTER_COUNTERS)


class CTCWriter(Thread):
    """`basecaller --save-ctc` (io.py:448-585): drains (chunk, result) on its own thread, keeps the chunks that pass, and
    writes ctc-data beside the stdout target -- chunks.npy float16 (k, chunksize), references.npy uint8 (k, longest label
    row), reference_lengths.npy uint16 -- plus filter_stats.csv, one SAM record on `fd` and one summary row per kept chunk.
    A result carries 'sequence', 'qstring', 'mapping' and, from the device stage (crf.basecall.basecall_ctc), 'verdict' and
    'target' (xb_ctc_targets' byte and label row); without them the decision is made here (ctc_verdict) from the mapping and
    aligner.seq.  Every chunk is logged.  Kept chunks go through typical_indices on their label lengths -- with its quirk:
    equal lengths keep NOTHING -- and through np.random.permutation from numpy's global state (util.init seeds it); the
    summary file is then rewritten with this run's rows in that order (the rows as first written, CRLF: the reference's
    pandas round trip is not reproduced).  Records are SAM text (mode 'w': header first; 'wfq': no header, as the
    reference opens pysam then); BAM / CRAM need htslib."""

    def __init__(self, mode, iterator, aligner, fd=sys.stdout, min_coverage=0.90, min_accuracy=0.95, ref_fn=None, groups=None,
                 group_key=None, ub_only=False, summary=None, directory=None, ub_plus=5, ub_minus=6):
        super().__init__()
        if mode not in ("wfq", "w"):
            raise NotImplementedError("SAM text is on the MI355X path; BAM / CRAM need htslib")
        self.mode, self.fd, self.iterator, self.aligner = mode, fd, iterator, aligner
        self.group_key = group_key
        self.groups = sorted(groups) if groups else []
        self.min_coverage, self.min_accuracy, self.ub_only = min_coverage, min_accuracy, ub_only
        self.ub_plus, self.ub_minus = ub_plus, ub_minus
        self.summary, self.directory = summary, directory
        self.log = []
        self.counts = dict.fromkeys(FILTER_COUNTERS, 0)
        self.error = None

    def _verdict(self, res):
        if "verdict" in res:
            return int(res["verdict"]), res.get("target")
        return ctc_verdict(res["sequence"], res.get("mapping"), self.aligner.seq, self.min_accuracy, self.min_coverage,
                           self.ub_only, self.ub_plus, self.ub_minus)

    def _count(self, verdict):
        c = self.counts
        c["count_failed_seq"] += bool(verdict & FAILED_SEQ)
        c["count_failed_map"] += bool(verdict & FAILED_MAP)
        c["non_ubs_skipped"] += bool(verdict & SKIPPED_NON_UB)
        c["count_failed_acc"] += bool(verdict & FAILED_ACC)
        c["count_failed_cov"] += bool(verdict & FAILED_COV)
        c["count_failed_both"] += verdict & (FAILED_ACC | FAILED_COV) == FAILED_ACC | FAILED_COV

    def run(self):
        try:
            self._run()
        except BaseException as e:  # surfaced by the CLI after join()
            self.error = e
            raise

    def _run(self):
        chunks, targets, rows = [], [], []
        path = self.summary or summary_file()
        columns = SUMMARY_COLUMNS + ALIGNMENT_COLUMNS
        with SummaryTable(path, columns) as table:
            if self.mode == "w":
                from . import __version__
                self.fd.write(sam_header(self.groups, aligner_version=__version__, aligner_name=ALIGNER_NAME,
                                         aligner_ds="exhaustive template alignment on the device"))
            for read, res in self.iterator:
                self.log.append((read.read_id, len(read.signal)))
                verdict, target = self._verdict(res)
                self._count(verdict)
                if verdict:
                    continue
                seq, qstring, mapping = res["sequence"], res["qstring"], res["mapping"]
                mean_q = res.get("mean_qscore")
                if mean_q is None:
                    mean_q = mean_qscore_from_qstring(qstring)
                self.fd.write(sam_record(read.read_id, seq, qstring, mapping) + "\n")
                row = summary_row(read, len(seq), mean_q, alignment=mapping)
                table.append(row)
                rows.append(row)
                targets.append(np.asarray(target, dtype=np.uint8))
                chunks.append(read.signal)
            columns = table.columns
        if self.ub_only:
            sys.stderr.write("Non-UB chunks skipped: {:0,d}\n".format(self.counts["non_ubs_skipped"]))
        sys.stderr.write("Filtered reads (failed): {:0,d} seq, {:0,d} map\n".format(
            self.counts["count_failed_seq"], self.counts["count_failed_map"]))
        sys.stderr.write("Filtered reads (failed): {:0,d} acc, {:0,d} cov, {:0,d} both\n".format(
            self.counts["count_failed_acc"], self.counts["count_failed_cov"], self.counts["count_failed_both"]))
        if len(chunks) == 0:
            sys.stderr.write("> no suitable ctc data to write\n")
            return
        chunks = np.array(chunks, dtype=np.float16)
        lengths = np.array([len(t) for t in targets], dtype=np.uint16)
        references = np.zeros((chunks.shape[0], int(lengths.max())), dtype=np.uint8)
        for idx, target in enumerate(targets):
            references[idx, :len(target)] = target
        indices = np.random.permutation(typical_indices(lengths))
        chunks, references, lengths = chunks[indices], references[indices], lengths[indices]
        with open(path, "w", newline="") as fh:
            for fields in [columns] + [[rows[i].get(c, "-") for c in columns] for i in indices]:
                fh.write("\t".join(_tsv_field(f) for f in fields) + "\r\n")
        directory = self.directory
        if directory is None:
            target = _stdout_target()
            directory = "." if target is None else os.path.dirname(target)
        with open(os.path.join(directory, "filter_stats.csv"), "w", newline="") as fh:
            fh.write(filter_stats_text(self.counts))
        np.save(os.path.join(directory, "chunks.npy"), chunks)
        np.save(os.path.join(directory, "references.npy"), references)
        np.save(os.path.join(directory, "reference_lengths.npy"), lengths)
        sys.stderr.write("> written ctc training data\n")
        sys.stderr.write("  - output_directory: {}\n".format(directory))
        sys.stderr.write("  - chunks.npy with shape (%s)\n" % ",".join(map(str, chunks.shape)))
        sys.stderr.write("  - references.npy with shape (%s)\n" % ",".join(map(str, references.shape)))
        sys.stderr.write("  - reference_lengths.npy shape (%s)\n" % ",".join(map(str, lengths.shape)))

    def stop(self):
        self.join()
