"""
The UB report: the figures of the reference's `src/tools/analyze_paf.py -p`, from what xb_ub_tally leaves (per-read counts and
the accumulators reads / err / cm).  Pure host code; the per-read walk, the polish and every tally ran on the device.

  per read       utils.py:850-916 and :1000-1001: read_acc, target_acc, ub_acc, ub_area_acc, ub_area_acc_plus, non_ub_area_acc,
                 fdr, fpr and the four outcomes -- quotients of the device's integer counts
  per position   100 * err / reads per (template, strand), labelled by distance to the UB (analyze_paf.py:111-190)
  summary        analyze_paf.py:904-1022: means over reads and over labelled positions, specificity, precision, F1, F2
  demux          analyze_paf.py:623-643 and :977-983 (`-d`): rows whose barcode distance (xb_barcode_dist, on the device) is over
                 the limit are dropped before anything is tallied; the summary gains demux and align
Departures from the reference are listed in INTEGRATION.md: the library FASTA stands in for XNA_refs, a template without a UB
site is of type PC, and the barcode's place in a template comes from the caller, not from XNA_refs.
"""
import gzip
import io

import numpy as np

from .aligner import MAX_ROW

COUNTS = ("n_match", "ub_matches", "ub_len", "ub_area_matches", "ub_area_len", "non_ub_area_matches", "non_ub_area_len",
          "ubs_detected")
METRICS = ("read_acc", "target_acc", "ub_acc", "ub_area_acc", "ub_area_acc_plus", "non_ub_area_acc", "fdr", "fpr", "true_pos",
           "false_neg", "false_pos", "true_neg")
KMER_LEN = 6                   # a UB's area reaches KMER_LEN - 1 positions to either side
MAX_DIST = 10                  # dist_ub_d-1 .. d-10, then d-11+
SUMMARY_DIST = 4               # err_ub_d_1 .. 4 in the summary row
BY_TAR_COLUMNS = ("percent_match", "target_acc", "read_acc", "ub_acc", "ub_area_acc", "non_ub_area_acc", "fpr", "ub_area_acc_plus")
STRAND_NAMES = ("F", "R")
BARCODE_COLUMNS = ("barcode_distance", "barcode_start", "barcode_end")


def ub_positions(template):
    """Positions of the UB sites of a template: every letter outside A, C, G, T (either case)."""
    return [j for j, c in enumerate(template) if c.upper() not in ("A", "C", "G", "T")]


def _div(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.asarray(a, np.float64) / np.asarray(b, np.float64)


def per_read_metrics(counts, read_alignment_length, target_length):
    """counts (n, 8) in the order COUNTS, the aligned length on the read and the template's length per read -> dict of (n,)
    arrays named in METRICS, computed as utils.py:850-916 computes them (nan where the reference gives nan)."""
    c = np.asarray(counts, np.int64).reshape(-1, len(COUNTS))
    n_match, ub_m, ub_len, ar_m, ar_len, non_m, non_len, det = c.T
    tl = np.asarray(target_length, np.int64)
    false = det - ub_m
    has_ub = ub_len > 0
    nan = np.full(len(c), np.nan)
    out = {
        "read_acc": _div(n_match, read_alignment_length),
        "target_acc": _div(n_match, tl),
        "ub_acc": np.where(has_ub, _div(ub_m, ub_len), nan),
        "ub_area_acc": np.where(has_ub, _div(ar_m, ar_len), nan),
        "ub_area_acc_plus": np.where(has_ub, _div(ar_m + ub_m, ar_len + ub_len), nan),
        "non_ub_area_acc": _div(non_m, non_len),
        "fdr": np.where(det > 0, _div(false, det), nan),
        "fpr": _div(false, tl - ub_len),
        "true_pos": ub_m,
        "false_neg": ub_len - ub_m,
        "false_pos": false,
        "true_neg": tl - ub_len - false,
    }
    return out


def error_rate(acc, offsets, t, s):
    """100 * err / reads of template t on strand index s (0 +, 1 -): the reference's error-rate vector, reversed on -."""
    a, b = int(offsets[t]), int(offsets[t + 1])
    return 100.0 * _div(acc.err[s, a:b], acc.reads[t, s])


def position_labels(length, x_positions, max_dist=MAX_DIST):
    """analyze_paf.py:111-190: label -> indices into an error-rate vector of `length` positions whose UB sites sit at
    x_positions (already mirrored for the reverse strand).  Without a UB site every position is no_ub / outside_ub_area."""
    pos = np.arange(length)
    no_ub = np.ones(length, bool)
    infl = np.zeros(length, bool)
    for x in x_positions:
        infl[max(0, x + 1 - KMER_LEN):x + KMER_LEN] = True
    for x in x_positions:
        no_ub[x] = False
        infl[x] = True
    cuts = {"only_ub": pos[~no_ub], "no_ub": pos[no_ub], "outside_ub_area": pos[~infl], "inside_ub_area": pos[infl & no_ub],
            "ub_and_ub_area": pos[infl]}
    if len(x_positions):
        dist = np.abs(pos[:, None] - np.asarray(x_positions)[None, :]).min(axis=1)
    else:
        dist = np.full(length, -1)
    for d in range(1, max_dist + 1):
        cuts["dist_ub_d-%d" % d] = pos[dist == d]
    cuts["dist_ub_d-%d+" % (max_dist + 1)] = pos[dist >= max_dist + 1]
    return cuts


def labelled_error_rates(acc, templates, offsets):
    """[(template index, strand index, type, label, error rates array)] for every (template, strand) with reads."""
    out = []
    for s in (0, 1):
        for t, tpl in enumerate(templates):
            if acc.reads[t, s] <= 0:
                continue
            xs = ub_positions(tpl)
            kind = "XNA" if xs else "PC"
            if s:
                xs = [len(tpl) - 1 - x for x in xs[::-1]]
            rate = error_rate(acc, offsets, t, s)
            for label, idx in position_labels(len(tpl), xs).items():
                out.append((t, s, kind, label, rate[idx]))
    return out


def _mean(values):
    values = np.asarray(values, np.float64)
    values = values[~np.isnan(values)]
    return float(values.mean()) if values.size else float("nan")


class Report:
    """Collects the reads of a run: per mapped read its identity and counts, and the accumulators.  demux: None, or
    (max_dist, bc_pos, bc_len, relax) -- the reference's `-d`: a row counts only when the barcode of its template lies within
    max_dist edits of the read where the mapping puts it (xb_barcode_dist)."""

    def __init__(self, names, templates, demux=None):
        from ._lib import UbAccumulators
        self.names, self.templates = list(names), list(templates)
        self.offsets = np.zeros(len(self.templates) + 1, np.int32)
        self.offsets[1:] = np.cumsum([len(t) for t in self.templates])
        self.library = "".join(self.templates).encode("ascii")
        self.acc = UbAccumulators(self.offsets)
        self.kind = ["XNA" if ub_positions(t) else "PC" for t in self.templates]
        self.read_ids, self.tmpl, self.strand, self.counts = [], [], [], []
        self.ral, self.mlen, self.blen = [], [], []
        self.demux = None if demux is None else tuple(int(v) for v in demux)
        self.barcode = []                         # per recorded row (distance, start, end), with demux only
        # the denominators of demux / align: every read id shown (n_reads overrides their number: the reads on file),
        # those that were mapped at all, those left after the barcode filter
        self.shown, self.aligned, self.demuxed, self.n_reads = set(), set(), set(), None

    def barcodes(self, ctx, rows, lens, got):
        """xb_barcode_dist on ctx over the rows of one mapper call with this report's demux setting."""
        _, bc_pos, bc_len, relax = self.demux
        return ctx.barcode_dist(rows, lens, got, self.library, self.offsets, bc_pos, bc_len, relax)

    def add(self, ctx, rows, lens, got, read_ids, barcodes=None):
        """The rows of one mapper call through xb_ub_tally on ctx; records every mapped row.  With demux the rows go through
        xb_barcode_dist first (or `barcodes`, what it returned for them earlier) and a row over the limit is passed on as
        unmapped: it adds nothing."""
        self.shown.update(read_ids)
        if self.demux is not None:
            bc = self.barcodes(ctx, rows, lens, got) if barcodes is None else barcodes
            dist = np.asarray(bc["bc_dist"])
            fail = (dist < 0) | (dist > self.demux[0])
            self.aligned.update(rid for rid, t in zip(read_ids, got["tmpl"]) if int(t) >= 0)
            self.demuxed.update(rid for rid, f in zip(read_ids, fail) if not f)
            got = dict(got, tmpl=np.where(fail, -1, got["tmpl"]).astype(np.int32))
        counts, self.acc = ctx.ub_tally(rows, lens, got, self.library, self.offsets, self.acc)
        for k, rid in enumerate(read_ids):
            t = int(got["tmpl"][k])
            if t < 0:
                continue
            n_ops = int(got["n_ops"][k])
            ops = got["ops"][k, :n_ops]
            self.read_ids.append(rid)
            self.tmpl.append(t)
            self.strand.append(1 if int(got["strand"][k]) < 0 else 0)
            self.counts.append(counts[k])
            self.ral.append(int(got["q_en"][k]) - int(got["q_st"][k]))
            self.mlen.append(int((ops == ord("=")).sum()))
            self.blen.append(n_ops)
            if self.demux is not None:
                self.barcode.append((int(bc["bc_dist"][k]), int(bc["bc_start"][k]), int(bc["bc_end"][k])))

    # ---- the figures ----
    def table(self):
        """Per-read columns: dict name -> array (tmpl, strand index, type, percent_match, the counts, the metrics)."""
        n = len(self.read_ids)
        tmpl = np.asarray(self.tmpl, np.int64).reshape(n)
        counts = np.asarray(self.counts, np.int64).reshape(n, len(COUNTS))
        tl = np.asarray([len(self.templates[t]) for t in tmpl], np.int64)
        out = {"tmpl": tmpl, "strand": np.asarray(self.strand, np.int64).reshape(n),
               "type": np.asarray([self.kind[t] for t in tmpl], object),
               "percent_match": _div(np.asarray(self.mlen, np.int64), np.asarray(self.blen, np.int64)).reshape(n)}
        out.update({k: counts[:, i] for i, k in enumerate(COUNTS)})
        out.update(per_read_metrics(counts, np.asarray(self.ral, np.int64).reshape(n), tl))
        if self.demux is not None:
            bc = np.asarray(self.barcode, np.int64).reshape(n, len(BARCODE_COLUMNS))
            out.update({k: bc[:, i] for i, k in enumerate(BARCODE_COLUMNS)})
        return out

    def summary(self):
        """analyze_paf.py:904-1022: the summary row as an ordered dict."""
        tab = self.table()
        xna, pc = tab["type"] == "XNA", tab["type"] == "PC"
        rates = labelled_error_rates(self.acc, self.templates, self.offsets)

        def err(label):
            vals = [r for _, _, kind, lab, r in rates if kind == "XNA" and lab == label]
            return _mean(np.concatenate(vals)) if vals else float("nan")

        row = {"num_aligned_reads": len(set(self.read_ids)),
               "target_acc": 100 * _mean(tab["target_acc"][xna]), "read_acc": 100 * _mean(tab["read_acc"][xna]),
               "err_far_ub": err("outside_ub_area"), "err_close_ub": err("inside_ub_area"), "err_only_ub": err("only_ub")}
        for d in range(1, SUMMARY_DIST + 1):
            row["err_ub_d_%d" % d] = err("dist_ub_d-%d" % d)
        row["acc_xna"] = 100 * _mean(tab["percent_match"][xna])
        row["acc_pc"] = 100 * _mean(tab["percent_match"][pc]) if pc.any() else float("nan")
        if self.demux is not None:
            total = len(self.shown) if self.n_reads is None else self.n_reads
            row["demux"] = float(100 * _div(len(self.demuxed), total))
            row["align"] = float(100 * _div(len(self.aligned), total))
        row["specificity"] = 100 * (1 - _mean(tab["fpr"]))
        row["precision"] = 100 * (1 - _mean(tab["fdr"]))
        tp, fn, fp, tn = (int(tab[k].sum()) for k in ("true_pos", "false_neg", "false_pos", "true_neg"))
        row.update(f_scores(tp, fn, fp))
        row.update({"true_pos": tp, "false_neg": fn, "false_pos": fp, "true_neg": tn})
        return row

    def by_target(self):
        """Rows (template name, strand F / R, type, the means * 100 of BY_TAR_COLUMNS, read count), sorted as pandas sorts its
        group keys: by name, strand, type."""
        tab = self.table()
        rows = []
        for t, s in sorted(set(zip(tab["tmpl"].tolist(), tab["strand"].tolist())), key=lambda k: (self.names[k[0]], k[1])):
            pick = (tab["tmpl"] == t) & (tab["strand"] == s)
            rows.append((self.names[t], STRAND_NAMES[s], self.kind[t], [100 * _mean(tab[c][pick]) for c in BY_TAR_COLUMNS],
                         int(pick.sum())))
        return rows

    # ---- the files ----
    def write(self, prefix, by_tar=True, by_read=True, confusion=True):
        """PREFIX.csv and, as asked for, PREFIX-by_tar.csv, PREFIX-by_read.csv.gz, PREFIX-confusion_matrix.npy; returns the paths."""
        paths = [prefix + ".csv"]
        row = self.summary()
        with open(paths[0], "w") as fh:
            fh.write(",".join(row) + "\n")
            fh.write(",".join(_fmt(v) for v in row.values()) + "\n")
        if by_tar:
            paths.append(prefix + "-by_tar.csv")
            with open(paths[-1], "w") as fh:
                fh.write("target_id,strand,type," + ",".join(BY_TAR_COLUMNS) + ",read_id\n")
                for name, strand, kind, means, count in self.by_target():
                    fh.write("%s,%s,%s,%s,%d\n" % (name, strand, kind, ",".join(_fmt(v) for v in means), count))
        if by_read:
            paths.append(prefix + "-by_read.csv.gz")
            tab = self.table()
            cols = ("percent_match",) + COUNTS + METRICS + (BARCODE_COLUMNS if self.demux is not None else ())
            text = io.StringIO()
            text.write("read_id,target_id,strand,type," + ",".join(cols) + "\n")
            for k, rid in enumerate(self.read_ids):
                vals = [_fmt(tab[c][k], "%.6f") for c in cols]
                text.write("%s,%s,%s,%s,%s\n" % (rid, self.names[tab["tmpl"][k]], STRAND_NAMES[tab["strand"][k]], tab["type"][k],
                                                 ",".join(vals)))
            with open(paths[-1], "wb") as fh:                    # no name, no time stamp: equal figures give equal bytes
                with gzip.GzipFile(filename="", mode="wb", fileobj=fh, mtime=0) as gz:
                    gz.write(text.getvalue().encode())
        if confusion:
            paths.append(prefix + "-confusion_matrix.npy")
            np.save(paths[-1], np.asarray(self.acc.cm, np.int64))
        return paths


def f_scores(tp, fn, fp):
    """analyze_paf.py:1003-1018: F1 and F2 (in percent) of the summed outcomes."""
    recall = tp / (tp + fn) if tp + fn > 0 else 0
    precision = tp / (tp + fp) if tp + fp > 0 else 0
    f1 = 2 * tp / (2 * tp + fp + fn) if tp + fp + fn > 0 else 0
    beta = 2
    f2 = (1 + beta ** 2) * precision * recall / (beta ** 2 * precision + recall) if precision + recall > 0 else 0
    return {"f1_score": 100 * f1, "f2_score": 100 * f2}


def _fmt(v, float_format="%.3f"):
    if isinstance(v, (int, np.integer)):
        return "%d" % v
    return "nan" if np.isnan(v) else float_format % v


# ---- from files: PAF + reads -> the mapper's columns (`analyze`) ------------------------------------------------------------
def cs_to_ops(cs):
    """A cs string (short form, or long form with '=' runs) -> the mapper's column bytes '=' 'X' 'I' 'D'."""
    ops, k, n = [], 0, len(cs)
    while k < n:
        sym = cs[k]
        e = k + 1
        if sym == ":":
            while e < n and cs[e].isdigit():
                e += 1
            if e == k + 1:
                raise ValueError("cs: ':' without a length in %r" % cs)
            ops.append("=" * int(cs[k + 1:e]))
        elif sym == "*":
            e = k + 3
            if e > n or not cs[k + 1:e].isalpha():
                raise ValueError("cs: '*' needs two letters in %r" % cs)
            ops.append("X")
        elif sym in "=+-":
            while e < n and cs[e].isalpha():
                e += 1
            if e == k + 1:
                raise ValueError("cs: %r without letters in %r" % (sym, cs))
            ops.append({"=": "=", "+": "I", "-": "D"}[sym] * (e - k - 1))
        elif sym == "~":
            raise ValueError("cs: introns ('~') are not supported")
        else:
            raise ValueError("cs: unexpected %r in %r" % (sym, cs))
        k = e
    return "".join(ops)


def read_paf(path):
    """[dict] per PAF line that carries a cs:Z: tag: read_id, read_length, q_st, q_en (on the read as it was made), strand
    (+1 / -1), target_id, r_st, r_en, ops."""
    out = []
    with open(path) as fh:
        for number, line in enumerate(fh, 1):
            if not line.strip():
                continue
            f = line.rstrip("\n").split("\t")
            if len(f) < 12:
                raise ValueError("%s: line %d has %d fields, a PAF line has at least 12" % (path, number, len(f)))
            cs = [x[5:] for x in f[12:] if x.startswith("cs:Z:")]
            if not cs:
                raise ValueError("%s: a PAF line without a cs:Z: tag (read %s)" % (path, f[0]))
            out.append(dict(read_id=f[0], read_length=int(f[1]), q_st=int(f[2]), q_en=int(f[3]), strand=-1 if f[4] == "-" else 1,
                            target_id=f[5], r_st=int(f[7]), r_en=int(f[8]), ops=cs_to_ops(cs[0])))
    return out


def read_sequences(path):
    """read id -> sequence of a FASTA or FASTQ text file (the first character decides)."""
    seqs = {}
    with open(path) as fh:
        lines = [l.rstrip("\n") for l in fh]
    k = 0
    while k < len(lines):
        line = lines[k]
        if line.startswith("@"):
            if k + 3 >= len(lines):
                raise ValueError("%s: truncated FASTQ record" % path)
            seqs[line[1:].split()[0] if line[1:].split() else ""] = lines[k + 1]
            k += 4
        elif line.startswith(">"):
            name = line[1:].split()[0] if line[1:].split() else ""
            parts = []
            k += 1
            while k < len(lines) and not lines[k].startswith(">"):
                parts.append(lines[k].strip())
                k += 1
            seqs[name] = "".join(parts)
        elif not line.strip():
            k += 1
        else:
            raise ValueError("%s: line %d is neither a FASTA nor a FASTQ record" % (path, k + 1))
    return seqs


def _paf_batches(report, alignments, sequences, batch):
    """The PAF rows `alignments` with the reads `sequences` as the mapper would have left them, `batch` at a time: (rows, lens,
    got, read ids)."""
    index = {n: t for t, n in enumerate(report.names)}
    lmax = int(np.diff(report.offsets).max())
    for at in range(0, len(alignments), batch):
        take = alignments[at:at + batch]
        seqs = []
        for a in take:
            if a["read_id"] not in sequences:
                raise ValueError("read %s of the PAF is not in the reads file" % a["read_id"])
            if a["target_id"] not in index:
                raise ValueError("target %s of the PAF is not in the library" % a["target_id"])
            s = sequences[a["read_id"]]
            if len(s) != a["read_length"]:
                raise ValueError("read %s has %d letters, the PAF says %d" % (a["read_id"], len(s), a["read_length"]))
            if len(s) > MAX_ROW:
                raise ValueError("read %s is longer than the %d letters a row takes" % (a["read_id"], MAX_ROW))
            seqs.append(s)
        n = len(take)
        width = max(16, -(-max(len(s) for s in seqs) // 16) * 16)
        rows = np.zeros((n, width), np.int8)
        got = {"ops": np.zeros((n, width + lmax), np.uint8)}
        for k in ("tmpl", "q_st", "q_en", "r_st", "r_en", "n_ops"):
            got[k] = np.zeros(n, np.int32)
        got["strand"] = np.zeros(n, np.int8)
        for k, (a, s) in enumerate(zip(take, seqs)):
            rows[k, :len(s)] = np.frombuffer(s.encode("ascii"), np.int8)
            if len(a["ops"]) > width + lmax:
                raise ValueError("read %s: %d alignment columns for a read of %d letters" % (a["read_id"], len(a["ops"]), len(s)))
            got["ops"][k, :len(a["ops"])] = np.frombuffer(a["ops"].encode("ascii"), np.uint8)
            got["n_ops"][k] = len(a["ops"])
            got["tmpl"][k], got["strand"][k] = index[a["target_id"]], a["strand"]
            got["r_st"][k], got["r_en"][k] = a["r_st"], a["r_en"]
            # the mapper's coordinates on the aligned strand
            got["q_st"][k] = a["q_st"] if a["strand"] > 0 else len(s) - a["q_en"]
            got["q_en"][k] = a["q_en"] if a["strand"] > 0 else len(s) - a["q_st"]
        yield rows, np.array([len(s) for s in seqs], np.int32), got, take


BARCODE_KEYS = ("bc_dist", "bc_start", "bc_end", "bc_obs_len")


def tally_paf(report, ctx, alignments, sequences, batch=512):
    """The PAF rows `alignments` (read_paf) with the reads `sequences` through xb_ub_tally on ctx into `report`.  For a report
    with demux the rows are those demux_paf kept, each with its "barcode"; rows without one get the first step of the filter
    alone (the limit), not the second (the read's smallest distance)."""
    for rows, lens, got, take in _paf_batches(report, alignments, sequences, batch):
        bc = None
        if report.demux is not None and all("barcode" in a for a in take):
            bc = {k: np.array([a["barcode"][i] for a in take], np.int32) for i, k in enumerate(BARCODE_KEYS)}
        report.add(ctx, rows, lens, got, [a["read_id"] for a in take], barcodes=bc)


def paf_barcodes(report, ctx, alignments, sequences, batch=512):
    """xb_barcode_dist over every PAF row: per alignment the tuple (bc_dist, bc_start, bc_end, bc_obs_len)."""
    out = []
    for rows, lens, got, _ in _paf_batches(report, alignments, sequences, batch):
        bc = report.barcodes(ctx, rows, lens, got)
        out.extend(zip(*[bc[k].tolist() for k in BARCODE_KEYS]))
    return out


def demux_filter(dist, read_ids, max_dist):
    """analyze_paf.py:628-632 over alignment rows: those with 0 <= dist <= max_dist, and of those, per read id, the rows whose
    distance equals that read's smallest; ties stay, all of them.  Returns the indices kept, ascending."""
    ok = [k for k, d in enumerate(dist) if 0 <= int(d) <= max_dist]
    low = {}
    for k in ok:
        low[read_ids[k]] = min(low.get(read_ids[k], int(dist[k])), int(dist[k]))
    return [k for k in ok if int(dist[k]) == low[read_ids[k]]]


def demux_paf(report, ctx, alignments, sequences, batch=512):
    """The first pass of `analyze -d`: distances for all alignments, the two-step filter, and the report's denominators (the
    reads on file, the read ids of the PAF, those left).  Returns the alignments kept, each with its "barcode", for tally_paf."""
    report.n_reads = len(sequences)
    report.aligned = {a["read_id"] for a in alignments}
    bc = paf_barcodes(report, ctx, alignments, sequences, batch)
    keep = demux_filter([b[0] for b in bc], [a["read_id"] for a in alignments], report.demux[0])
    report.demuxed = {alignments[k]["read_id"] for k in keep}
    return [dict(alignments[k], barcode=bc[k]) for k in keep]
