"""
CRF basecalling pipeline (ub-bonito/bonito/crf/basecall.py): chunk -> batch -> compute_scores ->
unbatch -> stitch -> strings, as five generator stages on background threads with bounded queues
(bonito/multiprocessing.py:20-24,92-122), strict FIFO order.
"""
import queue
from collections import deque
from threading import Thread

import numpy as np

from .._lib import output_level
from ..util import chunk, stitch, batchify, unbatchify, mean_qscore_from_qstring


class _ThreadIterator(Thread):
    """Run an iterator on a background thread behind a bounded queue (exceptions are re-raised)."""

    def __init__(self, iterator, maxsize=1):
        super().__init__(daemon=True)
        self.iterator = iterator
        self.queue = queue.Queue(maxsize)

    def __iter__(self):
        self.start()
        while True:
            item = self.queue.get()
            if item is StopIteration:
                break
            if isinstance(item, BaseException):
                raise item
            yield item

    def run(self):
        try:
            for item in self.iterator:
                self.queue.put(item)
            self.queue.put(StopIteration)
        except BaseException as e:  # propagate to the consumer instead of hanging it
            self.queue.put(e)


def thread_iter(iterator, maxsize=1):
    return iter(_ThreadIterator(iterator, maxsize=maxsize))


def stitch_results(results, length, size, overlap, stride, reverse=False):
    """crf/basecall.py:15-24"""
    if isinstance(results, dict):
        return {k: stitch_results(v, length, size, overlap, stride, reverse=reverse) for k, v in results.items()}
    return stitch(results, size, overlap, length, stride, reverse=reverse)


def compute_scores(model, batch, beam_width=32, beam_cut=100.0, scale=1.0, offset=0.0, blank_score=2.0,
                   reverse=False, qscores=False, ub_probs=False):
    """
    crf/basecall.py:27-82: (n,1,L) batch -> {'sequence': int8 (n,T), 'qstring': int8 (n,T), 'moves': bool (n,T)}.
    Viterbi branch (expand_blanks, the only one the reference reaches for XNA alphabets): left-packed ASCII rows, 'O'
    placeholders, no moves -- one fused device call; the per-character Python loops of the reference are gone.  With
    qscores (an extension, parity unpinned): the device's per-base qualities, left-packed beside the bases, and the
    per-step moves (xb_basecall_chunks_q; xb_decode_q on the host-reversed scores with reverse), qscale / qoffset from
    the config's [qscore] section.
    Beam branch (expand_blanks = False, `koi.decode.beam_search`): bases and quality characters at the blocks that emit,
    real moves -- xb_basecall_chunks_beam, for any alphabet the CRF supports.  `qscores` changes nothing there.
    With ub_probs (an extension, parity unpinned, Viterbi branch only): also 'probs' (n, nb, T) uint8, per base the
    probability byte of every letter alphabet[1 + b], left-packed beside the bases (xb_basecall_chunks_ub; xb_decode_ub with
    reverse); the qualities and moves are the device's with qscores, else the placeholders.
    """
    if not model.encoder[-1].expand_blanks:
        if ub_probs:
            raise ValueError("letter probabilities come from the Viterbi decode; this model takes the beam search")
        own = model.encoder[-1].blank_score
        if own is None or float(own) != float(blank_score):
            raise ValueError("beam search uses the model's fixed blank score (%r); blank_score=%r was asked for"
                             % (own, blank_score))
        if 0.0 < beam_cut < 1.0:
            raise ValueError("beam_cut %g inside (0, 1): no candidate can reach it" % beam_cut)
        if reverse:
            scores = model.seqdist.reverse_complement(model(batch))
            res = model.beam_search(scores, beam_width, beam_cut, scale, offset)
        else:
            res = model.basecall_chunks_beam(batch, beam_width, beam_cut, scale, offset)
        return {"qstring": res["qstring"], "sequence": res["sequence"], "moves": res["moves"].astype(bool)}
    level = output_level(qscores, ub_probs)
    if reverse:
        scores = model.seqdist.reverse_complement(model(batch))
        ctx = model.context(np.asarray(batch).shape[-1], scores.shape[1])
        rows = getattr(ctx, _DECODE[level])(scores, model.alphabet, *(model.qscore_params() if level else ()))
    else:
        rows = model.basecall_chunks(batch, **_LEVEL_FLAGS[level])
    return _result_dict(rows, qscores)


_DECODE = ("decode", "decode_q", "decode_ub")                         # the Context decode of each output level
_LEVEL_FLAGS = ({}, {"qscores": True}, {"ub_probs": True})            # ... and the Model keywords that ask for it


def _result_dict(rows, qscores):
    """compute_scores' dict of a decode's rows (seq, lens[, qstring, moves[, probs]]): the device qualities and moves with
    qscores, else the reference's layout around the left-packed ASCII rows -- dummy quality 'O', no moves (the bytes of a run
    without qualities, with letter probabilities too) -- and the letter-probability planes where the rows carry them."""
    sequence = rows[0]
    if qscores:
        out = {"qstring": rows[2], "sequence": sequence, "moves": rows[3].astype(bool)}
    else:
        out = {"qstring": np.where(sequence != 0, np.int8(ord("O")), np.int8(0)).astype(np.int8), "sequence": sequence,
               "moves": np.zeros(sequence.shape, dtype=bool)}
    if len(rows) > 4:
        out["probs"] = rows[4]
    return out


def compute_sequences_pipelined(model, batches, reverse=False, qscores=False, ub_probs=False):
    """
    The device stage of `basecall`: (key, batch) stream -> (key, sequence (n,T) int8 left-packed ASCII) with several batches
    in flight on the device: batch k+1 is submitted (pinned staging, H2D on a copy stream, fused kernels, D2H) before
    batch k's result is waited for, so the GPU never idles while the host unpacks results.  Where the context co-schedules two
    calls per device pass (Model.pipeline_depth: batches of at most 640 chunks) FOUR batches rotate through four staging
    slots -- batch k+3 is submitted before batch k is collected, so pair (k+2, k+3) is on the device, its H2D copies done,
    while the host waits for pair (k, k+1) -- otherwise two.  Results come out in input order, depth - 1 batches late.
    (compute_scores is the same operator, synchronous, with the reference's full result dict.)
    With qscores every item is instead compute_scores' dict with the device qualities and moves (Viterbi branch), with
    ub_probs compute_scores' dict with the letter-probability planes.
    """
    level = output_level(qscores, ub_probs)
    if reverse or not model.encoder[-1].expand_blanks:
        for key, batch in batches:                       # decode of host-side reverse-complemented scores: synchronous
            res = compute_scores(model, batch, reverse=reverse, qscores=qscores, ub_probs=ub_probs)
            yield key, res if level else res["sequence"]
        return

    def submit(slot, batch):
        return model.submit_chunks(slot, batch, **_LEVEL_FLAGS[level])

    def collect(handle):
        rows = model.collect_chunks(handle)
        return _result_dict(rows, qscores) if level else rows[0]

    pending, slot, depth = deque(), 0, 2
    for key, batch in batches:
        shape = np.asarray(batch).shape
        if pending and not model.context_is_current(shape[-1], shape[0]):
            while pending:                                                # drain before the context is rebuilt
                k, h = pending.popleft()
                yield k, collect(h)
        if not pending:
            depth, slot = model.pipeline_depth(shape[-1], shape[0]), 0
        pending.append((key, submit(slot, batch)))
        slot = (slot + 1) % depth
        if len(pending) == depth:                                         # the slot the next batch goes into
            k, h = pending.popleft()
            yield k, collect(h)
    while pending:
        k, h = pending.popleft()
        yield k, collect(h)


def compute_scores_pipelined(model, batches, reverse=False, qscores=False, ub_probs=False):
    """compute_scores over a stream of (key, batch), two batches in flight; yields the reference's result dicts."""
    if not model.encoder[-1].expand_blanks:              # beam search: qualities and moves are real, one batch at a time
        for key, batch in batches:
            yield key, compute_scores(model, batch, reverse=reverse, ub_probs=ub_probs)
        return
    for key, res in compute_sequences_pipelined(model, batches, reverse=reverse, qscores=qscores, ub_probs=ub_probs):
        yield key, res if (qscores or ub_probs) else _result_dict((res,), False)


def to_str(x, encoding="ascii"):
    """koi.decode.to_str: int8 array -> str without the zero padding."""
    x = np.asarray(x)
    return x[x != 0].astype(np.uint8).tobytes().decode(encoding)


def apply_stride_to_moves(model, attrs):
    """crf/basecall.py:85-93"""
    moves = np.array(attrs["moves"], dtype=bool)
    sig_move = np.full(moves.size * model.stride, False)
    sig_move[np.where(moves)[0] * model.stride] = True
    return {
        "qstring": to_str(attrs["qstring"]),
        "sequence": to_str(attrs["sequence"]),
        "sig_move": sig_move,
    }


def _called(model, sequence):
    """
    The per-read result of crf/basecall.py:85-93 from the stitched left-packed row alone.  The Viterbi branch's quality
    string and moves are placeholders that mirror the sequence (crf/basecall.py:60-76: 'O' wherever a base was written,
    no moves), so stitching them separately and then dropping their padding gives exactly 'O' * len(sequence) and an
    all-False signal-move vector of one entry per stitched slot and stride.
    """
    seq = to_str(sequence)
    return {"qstring": "O" * len(seq), "sequence": seq, "sig_move": np.zeros(np.asarray(sequence).size * model.stride, dtype=bool),
            "mean_qscore": 40.0 if seq else 0.0}           # = mean_qscore_from_qstring('O' * n), util.py:124-131


def _called_beam(model, attrs):
    """crf/basecall.py:85-93 on stitched results with real qualities (beam search, or Viterbi with qscores), plus the mean
    quality the writers print."""
    out = apply_stride_to_moves(model, attrs)
    out["mean_qscore"] = mean_qscore_from_qstring(out["qstring"]) if out["qstring"] else 0.0
    return out


NATURAL = "ACGT"


def ub_letters(model):
    """(plane index b, letter) of the model's alphabet letters outside A, C, G, T: the letters `ub_probs` reports."""
    return [(b, c) for b, c in enumerate(model.alphabet[1:]) if c not in NATURAL]


def _planes(res):
    """compute_scores' (n, nb, T) 'probs' as one (n, T) row set per plane, stitched like the sequence rows."""
    if "probs" not in res:
        return res
    out = dict(res)
    probs = out.pop("probs")
    out["probs"] = {b: probs[:, b] for b in range(probs.shape[1])}
    return out


def ub_tags(model, attrs):
    """SAM / FASTQ tags of the stitched planes: `u<letter>:B:C,v1,..,vL` per letter outside A, C, G, T, one value per
    called base (the plane bytes where the stitched sequence row holds a base)."""
    called = np.asarray(attrs["sequence"]) != 0
    tags = []
    for b, letter in ub_letters(model):
        vals = np.asarray(attrs["probs"][b])[called]
        tags.append("u%s:B:C,%s" % (letter, ",".join(map(str, vals.tolist()))))
    return tags


def _called_ub(model, attrs):
    out = _called_beam(model, attrs)
    if out["sequence"]:
        out["mods"] = ub_tags(model, attrs)
    return out


def basecall(model, reads, chunksize=4000, overlap=100, batchsize=32, reverse=False, qscores=False, ub_probs=False):
    """Basecall `reads` (objects with .signal); yields (read, {'sequence','qstring','sig_move'}) in input order.
    qscores: the Viterbi branch writes the device's per-base qualities (compute_scores) instead of the 'O' placeholders;
    their rows are stitched like the sequence rows, so len(qstring) == len(sequence), and the moves are stitched in time.
    ub_probs: the letter-probability planes are stitched like the sequence rows too (reverse included), and every read's
    result carries their tags in 'mods' (ub_tags), the slot the writers append to a record's tags."""
    chunks = thread_iter(
        ((read, 0, len(read.signal)), chunk(np.asarray(read.signal, dtype=np.float32), chunksize, overlap))
        for read in reads
    )
    batches = thread_iter(batchify(chunks, batchsize=batchsize))
    if qscores or ub_probs or not model.encoder[-1].expand_blanks:
        # the reference's own five stages (crf/basecall.py:96-122): result dicts are unbatched and stitched plane by plane
        scores = thread_iter((key, _planes(res)) for key, res in
                             compute_scores_pipelined(model, batches, reverse=reverse, qscores=qscores, ub_probs=ub_probs))
        results = thread_iter(
            (read, stitch_results(attrs, end - start, chunksize, overlap, model.stride, reverse))
            for ((read, start, end), attrs) in unbatchify(scores)
        )
        called = _called_ub if ub_probs else _called_beam
        return thread_iter((read, called(model, attrs)) for read, attrs in results)
    sequences = thread_iter(compute_sequences_pipelined(model, batches, reverse=reverse))
    results = thread_iter(
        (read, stitch(seq, chunksize, overlap, end - start, model.stride, reverse=reverse))
        for ((read, start, end), seq) in unbatchify(sequences)
    )
    return thread_iter(
        (read, _called(model, stitched))
        for read, stitched in results
    )


def _chunk_batches(chunks, batchsize):
    held = []
    for c in chunks:
        held.append(c)
        if len(held) == batchsize:
            yield held
            held = []
    if held:
        yield held


def basecall_ctc(model, aligner, chunks, batchsize=32, min_accuracy=0.95, min_coverage=0.90, ub_only=False, ub_plus=5,
                 ub_minus=6):
    """The device stage of `basecaller --save-ctc`: `chunks` are ReadChunks, each one whole chunk of the model's chunksize, so
    chunking and stitching have nothing to do (util.py:172-173) and a batch is just `batchsize` signals.  Viterbi models take
    one fused device call per batch (xb_ctc_chunks: basecall, template mapper, verdict and label row, one synchronisation);
    beam-search models take the host-form beam call, then the host forms of the mapper and of xb_ctc_targets -- the same
    kernel.  Batches run one at a time (the fused call is synchronous); the next batch's signals are stacked on a
    background thread meanwhile.  Yields (chunk, {'sequence', 'qstring', 'mean_qscore', 'mapping', 'target', 'verdict'}) in
    input order; a Mapping is built only where verdict == 0 (None elsewhere), 'target' is the label row cut to its length."""
    rule = dict(min_accuracy=min_accuracy, min_coverage=min_coverage, ub_only=ub_only, ub_plus=ub_plus, ub_minus=ub_minus)
    viterbi = bool(model.encoder[-1].expand_blanks)

    def stacked():
        for held in _chunk_batches(chunks, batchsize):
            yield held, np.stack([np.asarray(c.signal, dtype=np.float32) for c in held])

    for held, sig in thread_iter(stacked()):
        if viterbi:
            ctx = model.context(sig.shape[1], sig.shape[0])
            model.chunks_submitted = getattr(model, "chunks_submitted", 0) + sig.shape[0]
            out = ctx.ctc_chunks(sig, model.alphabet, aligner.library, aligner.offsets, aligner.scoring, **rule)
            seqs = [out["seq"][k, :out["seq_len"][k]].tobytes().decode("ascii") for k in range(len(held))]
            quals = [None] * len(held)
            rows = ((k, out, out, k) for k in range(len(held)))
        else:
            res = compute_scores(model, sig[:, None, :])
            seqs = [to_str(r) for r in res["sequence"]]
            quals = [to_str(r) for r in res["qstring"]]
            rows = aligner.ctc_rows(seqs, **rule)
        for k, got, lab, j in rows:
            seq, verdict = seqs[k], int(lab["verdict"][j])
            qstring = "O" * len(seq) if quals[k] is None else quals[k]
            item = {"sequence": seq, "qstring": qstring, "verdict": verdict, "mapping": None, "target": None,
                    "mean_qscore": (40.0 if seq else 0.0) if quals[k] is None else
                    (mean_qscore_from_qstring(qstring) if qstring else 0.0)}
            if verdict == 0:
                item["mapping"] = aligner.mapping(got, j, seq)
                item["target"] = lab["target"][j, :int(lab["target_len"][j])].copy()
            yield held[k], item
