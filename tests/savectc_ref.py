"""
Test infrastructure (like tests/map_ref.py): the CPU restatement of xb_ctc_targets' contract (include/xna_basecaller.h,
"ctc-data labels of mapped rows") in plain numpy / Python, written from the reference's CTCWriter.run (bonito/io.py).
Nothing in the product imports this module, and it imports nothing of the product.

  io.py:495-501   an empty sequence counts as failed_seq, a missing mapping as failed_map, either one ends the chunk
  io.py:503-504   cov = (q_en - q_st) / len(seq), acc = mlen / blen -- Python floats: one float64 division each
  io.py:505-510   refseq = template[r_st:r_en]; ub_only and no 'N' in it: skipped, before the thresholds
  io.py:512-522   acc < min_accuracy, cov < min_coverage, counted one by one and together; either one drops the chunk
  io.py:532-540   strand -1: the reverse complement; A C G T -> 1 2 3 4, N -> 5 on strand +1, 6 on strand -1
Stated beyond the reference: every byte outside ACGTacgt is what 'N' is there (the mapper's letter contract); the labels 5 / 6
are the arguments ub_plus / ub_minus; mlen counts the '=' columns; a mapped row without columns fails the accuracy test.
"""
import numpy as np

FAILED_SEQ, FAILED_MAP, SKIPPED_NON_UB, FAILED_ACC, FAILED_COV = 1, 2, 4, 8, 16
NATURAL = "ACGTacgt"
_COMP = {"A": "T", "C": "G", "G": "C", "T": "A", "a": "t", "c": "g", "g": "c", "t": "a"}


def quotients(seq_len, q_st, q_en, mlen, blen):
    """(cov, acc) as the reference computes them: Python's true division of ints."""
    return (q_en - q_st) / seq_len, mlen / blen


def row(seq_len, tmpl, strand, q_st, q_en, r_st, r_en, ops, templates, min_accuracy=0.95, min_coverage=0.90, ub_only=False,
        ub_plus=5, ub_minus=6):
    """One row -> (mlen, blen, verdict, labels list).  ops: the row's alignment columns (bytes, n_ops of them)."""
    ops = bytes(ops)
    mlen, blen = ops.count(b"="), len(ops)
    verdict = (FAILED_SEQ if seq_len == 0 else 0) | (FAILED_MAP if tmpl < 0 or tmpl >= len(templates) else 0)
    if verdict:
        return mlen, blen, verdict, []
    template = templates[tmpl]
    r_st = min(max(r_st, 0), len(template))
    r_en = min(max(r_en, r_st), len(template))
    refseq = template[r_st:r_en]
    if ub_only and not any(c not in NATURAL for c in refseq):
        return mlen, blen, SKIPPED_NON_UB, []
    if blen == 0:
        verdict |= FAILED_ACC
        cov = (q_en - q_st) / seq_len
    else:
        cov, acc = quotients(seq_len, q_st, q_en, mlen, blen)
        if acc < min_accuracy:
            verdict |= FAILED_ACC
    if cov < min_coverage:
        verdict |= FAILED_COV
    if verdict:
        return mlen, blen, verdict, []
    if strand == -1:
        refseq = "".join(_COMP.get(c, c) for c in reversed(refseq))
    ub = ub_minus if strand == -1 else ub_plus
    return mlen, blen, 0, [{"A": 1, "C": 2, "G": 3, "T": 4}.get(c.upper(), ub) if c in NATURAL else ub for c in refseq]


def target_width(templates):
    return -(-max(len(t) for t in templates) // 16) * 16


def targets(seq_len, width, mapped, templates, **rule):
    """The arrays xb_ctc_targets writes for seq_len (n), rows of `width` and the mapper's outputs `mapped` (name -> array):
    name -> array, target (n, longest template rounded up to 16) zero-filled."""
    n = len(seq_len)
    cap = width + max(len(t) for t in templates)
    out = {"mlen": np.zeros(n, np.int32), "blen": np.zeros(n, np.int32), "verdict": np.zeros(n, np.uint8),
           "target": np.zeros((n, target_width(templates)), np.uint8), "target_len": np.zeros(n, np.int32)}
    for r in range(n):
        sl = min(max(int(seq_len[r]), 0), width)
        nops = min(max(int(mapped["n_ops"][r]), 0), cap)
        mlen, blen, verdict, labels = row(sl, int(mapped["tmpl"][r]), int(mapped["strand"][r]), int(mapped["q_st"][r]),
                                          int(mapped["q_en"][r]), int(mapped["r_st"][r]), int(mapped["r_en"][r]),
                                          np.asarray(mapped["ops"][r, :nops], np.uint8).tobytes(), templates, **rule)
        out["mlen"][r], out["blen"][r], out["verdict"][r], out["target_len"][r] = mlen, blen, verdict, len(labels)
        out["target"][r, :len(labels)] = labels
    return out


def typical_indices(x, n=2.5):
    """cli/convert.py:80-83"""
    mu, sd = np.mean(x), np.std(x)
    idx, = np.where((mu - n * sd < x) & (x < mu + n * sd))
    return idx


def predict(items, seed, chunksize):
    """What `basecaller --save-ctc` leaves for `items` = [(signal, summary key, verdict, labels)] in stream order under
    util.init(seed): the counters, and chunks / references / reference_lengths / the summary keys in written order (None for
    the arrays when nothing is kept)."""
    counts = dict.fromkeys(("count_failed_seq", "count_failed_map", "count_failed_acc", "count_failed_cov", "count_failed_both",
                            "non_ubs_skipped"), 0)
    kept = []
    for signal, key, verdict, labels in items:
        counts["count_failed_seq"] += bool(verdict & FAILED_SEQ)
        counts["count_failed_map"] += bool(verdict & FAILED_MAP)
        counts["non_ubs_skipped"] += bool(verdict & SKIPPED_NON_UB)
        counts["count_failed_acc"] += bool(verdict & FAILED_ACC)
        counts["count_failed_cov"] += bool(verdict & FAILED_COV)
        counts["count_failed_both"] += bool(verdict & FAILED_ACC) and bool(verdict & FAILED_COV)
        if verdict == 0:
            kept.append((signal, key, labels))
    if not kept:
        return counts, None, None, None, []
    chunks = np.array([s for s, _, _ in kept], dtype=np.float16)
    lengths = np.array([len(l) for _, _, l in kept], dtype=np.uint16)
    refs = np.zeros((len(kept), int(lengths.max())), np.uint8)
    for i, (_, _, l) in enumerate(kept):
        refs[i, :len(l)] = l
    state = np.random.get_state()
    np.random.seed(seed)
    idx = np.random.permutation(typical_indices(lengths))
    np.random.set_state(state)
    return counts, chunks[idx], refs[idx], lengths[idx], [kept[i][1] for i in idx]


def filter_stats_text(counts):
    """pandas.Series(dict(...)).to_csv(): an empty index label, the column name 0, then name,value lines."""
    lines = [",0"] + ["%s,%d" % (k, counts[k]) for k in ("count_failed_seq", "count_failed_map", "count_failed_acc",
                                                         "count_failed_cov", "count_failed_both", "non_ubs_skipped")]
    return "\n".join(lines) + "\n"
