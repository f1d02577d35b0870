"""
`--reference`: map called sequences to a template library on the device (the reference's stage is bonito/aligner.py:12-16,
mappy over minimap2 -- a genome aligner no image here has, and more than a library of a few hundred short templates needs).

xb_map_templates (include/xna_basecaller.h) aligns every call against every template on both strands exhaustively and hands
back, per call, the winning template, strand, score, the best other template's score, the coordinates and one byte per
alignment column; everything a `mappy.Alignment` carries that the reference reads (io.py:118-135, 208-230) -- CIGAR, NM, MD,
blen, mlen -- and the `cs` string are put together from those columns here, on the host.

The contract is this package's own (minimap2 parity is unpinned): scoring defaults to minimap2's map-ont first piece, every
letter outside A, C, G, T is ambiguous on both sides, and `mapq` is clamp(int(60 * (1 - second / score)), 0, 60) -- NOT
minimap2's formula, which needs chain scores.
"""
from collections import namedtuple

import numpy as np

from . import _lib

Scoring = namedtuple("Scoring", "match mismatch gap_open gap_extend ambiguous")
MAP_ONT = Scoring(2, 4, 4, 2, 1)           # minimap2 -x map-ont, first gap piece; sc_ambi 1
MAX_ROW = 4096                             # widest row xb_map_templates takes
CELL_BUDGET = 1.2e11                       # its cell budget per call: 2 n W sum(L)
CIGAR_OPS = {"M": 0, "I": 1, "D": 2}       # mappy's numbers (BAM's)
_COMP = str.maketrans("ACGTacgt", "TGCAtgca")


def read_fasta(path):
    """[(name, sequence)]: names up to the first whitespace, records over several lines."""
    records, name, parts = [], None, []
    with open(path) as fh:
        for line in fh:
            line = line.strip()
            if line.startswith(">"):
                if name is not None:
                    records.append((name, "".join(parts)))
                fields = line[1:].split()
                name, parts = (fields[0] if fields else ""), []
            elif line and name is not None:
                parts.append(line)
    if name is not None:
        records.append((name, "".join(parts)))
    return records


def _cs_letter(c):
    return c.lower() if c in "ACGTacgt" else "n"


def aligned_strand(sequence, strand):
    """The letters the aligner saw: the call itself, or on the reverse strand its reverse with A, C, G, T complemented (any
    other letter is ambiguous either way and stays what it is)."""
    return sequence if strand == +1 else sequence[::-1].translate(_COMP)


def mapq(score, second):
    return min(60, max(0, int(60 * (1 - second / score)))) if score > 0 else 0


class Mapping:
    """What the reference reads from a mappy.Alignment, plus cs, score and second.  q_st / q_en are mappy's: on the call as it
    was made (the original strand); r_st / r_en on the template; the CIGAR runs along the template."""

    __slots__ = ("ctg", "ctg_len", "r_st", "r_en", "q_st", "q_en", "strand", "mapq", "cigar", "cigar_str", "NM", "MD", "blen",
                 "mlen", "cs", "score", "second")

    def __init__(self, ctg, template, sequence, strand, r_st, q_st_aligned, ops, score=0, second=0):
        """From the alignment columns `ops` ('=' 'X' 'I' 'D' in template order), the template start r_st and the start on the
        ALIGNED strand q_st_aligned (xb_map_templates' q_st)."""
        ops = ops.decode("ascii") if isinstance(ops, (bytes, bytearray)) else "".join(map(chr, ops)) if not isinstance(ops, str) else ops
        query = aligned_strand(sequence, strand)
        runs, md, cs = [], [], []
        match_run = 0                      # '=' columns since the last MD event
        qi, ri, k = q_st_aligned, r_st, 0
        while k < len(ops):
            op = ops[k]
            e = k
            while e < len(ops) and ops[e] == op:
                e += 1
            n = e - k
            kind = "M" if op in "=X" else op
            if runs and runs[-1][1] == kind:
                runs[-1][0] += n
            else:
                runs.append([n, kind])
            if op == "=":
                match_run += n
                cs.append(":%d" % n)
                qi, ri = qi + n, ri + n
            elif op == "X":
                for _ in range(n):
                    md.append("%d%s" % (match_run, template[ri]))
                    match_run = 0
                    cs.append("*%s%s" % (_cs_letter(template[ri]), _cs_letter(query[qi])))
                    qi, ri = qi + 1, ri + 1
            elif op == "D":
                md.append("%d^%s" % (match_run, template[ri:ri + n]))
                match_run = 0
                cs.append("-" + "".join(_cs_letter(c) for c in template[ri:ri + n]))
                ri += n
            elif op == "I":
                cs.append("+" + "".join(_cs_letter(c) for c in query[qi:qi + n]))
                qi += n
            else:
                raise ValueError("alignment column %r" % op)
            k = e
        md.append("%d" % match_run)
        self.ctg, self.ctg_len, self.strand = ctg, len(template), strand
        self.r_st, self.r_en = r_st, ri
        if strand == +1:
            self.q_st, self.q_en = q_st_aligned, qi
        else:
            self.q_st, self.q_en = len(sequence) - qi, len(sequence) - q_st_aligned
        self.cigar = [(n, CIGAR_OPS[kind]) for n, kind in runs]
        self.cigar_str = "".join("%d%s" % (n, kind) for n, kind in runs)
        self.mlen = ops.count("=")
        self.blen = len(ops)
        self.NM = self.blen - self.mlen
        self.MD = "".join(md)
        self.cs = "".join(cs)
        self.score, self.second = int(score), int(second)
        self.mapq = mapq(score, second) if score else 0

    def __repr__(self):
        return "Mapping(%s %s %d-%d q %d-%d %s mapq %d cs %s)" % (self.ctg, "+" if self.strand == 1 else "-", self.r_st, self.r_en,
                                                                   self.q_st, self.q_en, self.cigar_str, self.mapq, self.cs)


class TemplateAligner:
    """A template library (FASTA) and the device mapper over it.  `.map(sequences)` -> [Mapping | None] in order, through
    xb_map_templates, in as many device calls as the cell budget asks for.  `context` is a callable that returns the
    _lib.Context to run on (the CLI passes the model's, so that mapping queues on the basecaller's own stream); without one
    the aligner opens a small context of its own on `device`."""

    def __init__(self, path, scoring=None, device=0, context=None, batch=512):
        self.path = str(path)
        self.records = read_fasta(path)
        if not self.records:
            raise ValueError("%s holds no FASTA record" % path)
        self.names = [n for n, _ in self.records]
        self.templates = [s for _, s in self.records]
        if any(not t for t in self.templates):
            raise ValueError("%s: empty template" % path)
        self.scoring = Scoring(*(MAP_ONT if scoring is None else scoring))
        self.library = "".join(self.templates).encode("ascii")
        self.offsets = np.zeros(len(self.templates) + 1, np.int32)
        self.offsets[1:] = np.cumsum([len(t) for t in self.templates])
        self.batch = int(batch)
        self._device, self._context, self._own = device, context, None
        self.ub_report = None                      # `--ub-report`: a ubreport.Report that map() feeds after every mapper call

    @classmethod
    def from_config(cls, path, config, **kwargs):
        """Scoring from the optional [aligner] keys of a model's config.toml (match, mismatch, gap_open, gap_extend,
        ambiguous); map-ont's where a key is missing."""
        keys = (config or {}).get("aligner", {}) or {}
        return cls(path, scoring=Scoring(*[int(keys.get(f, d)) for f, d in zip(Scoring._fields, MAP_ONT)]), **kwargs)

    def context(self):
        ctx = self._context() if self._context is not None else None
        if ctx is not None and getattr(ctx, "h", None):
            return ctx
        if self._own is None:
            _lib.require_gpu()
            self._own = _lib.mapper_context(self._device)
        return self._own

    def close(self):
        if self._own is not None:
            self._own.close()
            self._own = None

    def seq(self, name, start=0, end=None):
        """mappy's Aligner.seq: letters [start, end) of the template called `name`."""
        return self.templates[self.names.index(name)][start:end]

    def mapping(self, got, k, sequence):
        """Row k of map_templates' outputs `got` as a Mapping of `sequence`, None when the row is unmapped."""
        t = int(got["tmpl"][k])
        if t < 0:
            return None
        return Mapping(self.names[t], self.templates[t], sequence, int(got["strand"][k]), int(got["r_st"][k]), int(got["q_st"][k]),
                       got["ops"][k, :int(got["n_ops"][k])].tobytes(), got["score"][k], got["second"][k])

    def ctc_rows(self, sequences, **rule):
        """Host-form mapping and labelling of called strings (the beam branch of `--save-ctc`): per device call of the mapper
        (its cell budget) a call of xb_ctc_targets over the same rows; yields (index, mapper outputs, label outputs, row) for
        every sequence, in order.  rule: ctc_targets' thresholds and labels."""
        sequences = list(sequences)
        if any(len(s) > MAX_ROW for s in sequences):
            raise ValueError("a call longer than the mapper's %d letters" % MAX_ROW)
        at = 0
        while at < len(sequences):
            take = sequences[at:at + self.batch]
            width = max(16, -(-max(len(s) for s in take) // 16) * 16)
            fit = int(CELL_BUDGET // (2.0 * width * len(self.library)))
            if 0 < fit < len(take):
                take = take[:fit]
            got = self._call(take)
            lens = np.array([len(s) for s in take], np.int32)
            lab = self.context().ctc_targets(lens, got["ops"].shape[1] - int(np.diff(self.offsets).max()), got, self.library,
                                             self.offsets, **rule)
            for k in range(len(take)):
                yield at + k, got, lab, k
            at += len(take)

    @staticmethod
    def _pack(seqs):
        """Called strings as the mapper's rows: (n, W) int8 left-packed, W a multiple of 16, and their lengths."""
        width = max(16, -(-max(len(s) for s in seqs) // 16) * 16)
        rows = np.zeros((len(seqs), width), np.int8)
        for r, s in enumerate(seqs):
            rows[r, :len(s)] = np.frombuffer(s.encode("ascii"), np.int8)
        return rows, np.array([len(s) for s in seqs], np.int32)

    def _call(self, seqs):
        rows, lens = self._pack(seqs)
        return self.context().map_templates(rows, lens, self.library, self.offsets, self.scoring)

    def map(self, sequences, read_ids=None):
        """[Mapping | None] per sequence.  With a ub_report set, the rows of every mapper call also go through xb_ub_tally
        (read_ids name them in the report)."""
        sequences = list(sequences)
        out = [None] * len(sequences)
        todo = [i for i, s in enumerate(sequences) if 0 < len(s) <= MAX_ROW]
        if self.ub_report is not None:              # every read counts in the report's denominators, mapped or not
            self.ub_report.shown.update(read_ids if read_ids is not None else [str(i) for i in range(len(sequences))])
        if len(todo) < sum(1 for s in sequences if s):
            from logging import getLogger
            getLogger("bonito").warning("> %d calls longer than the mapper's %d letters are left unmapped",
                                        sum(1 for s in sequences if len(s) > MAX_ROW), MAX_ROW)
        at = 0
        while at < len(todo):
            take = todo[at:at + self.batch]
            width = -(-max(len(sequences[i]) for i in take) // 16) * 16
            fit = int(CELL_BUDGET // (2.0 * max(16, width) * len(self.library)))
            if 0 < fit < len(take):                 # fit == 0: one row is over the budget -- the library's refusal says so
                take = take[:fit]
            rows, lens = self._pack([sequences[i] for i in take])
            got = self.context().map_templates(rows, lens, self.library, self.offsets, self.scoring)
            if self.ub_report is not None:
                self.ub_report.add(self.context(), rows, lens, got, [read_ids[i] if read_ids is not None else str(i) for i in take])
            for k, i in enumerate(take):
                out[i] = self.mapping(got, k, sequences[i])
            at += len(take)
        return out


def align_map(aligner, results, batch=256):
    """The reference's stage (bonito/aligner.py:12-16): adds 'mapping' to every (read, result), order kept; `batch` reads go
    to the device together.  None where nothing aligns."""
    held = []

    def flush():
        ids = [read.read_id for read, _ in held] if getattr(aligner, "ub_report", None) is not None else None
        seqs = [res["sequence"] for _, res in held]
        for (read, res), m in zip(held, aligner.map(seqs) if ids is None else aligner.map(seqs, ids)):
            yield read, dict(res, mapping=m)
        held.clear()

    for item in results:
        held.append(item)
        if len(held) >= batch:
            yield from flush()
    yield from flush()
