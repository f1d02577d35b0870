"""
`bonito evaluate MODEL_DIR --directory CTC_DATA` (ub-bonito/bonito/cli/evaluate.py): call the validation chunks with every
requested checkpoint and report the mean / median accuracy against the references, the time and samples/s.

Device work = the reference's `model(data)` + `model.decode_batch(log_probs)` per batch (evaluate.py:57-72): here one fused
call per batch (`Model.basecall_chunks`: the same scores and the same decode without moving the scores to the host).
Accuracy = util.accuracy (host side; xb_align_accuracy restates the parasail call, see csrc/xb_align.hip).  --poa (spoa
consensus over several checkpoints) is outside the MI355X path and refused.

--loss adds validate_one_epoch's third figure (training.py:175-181): the batches go through `Model.validate_chunks`, which
also returns each chunk's CTC-CRF loss from the same device-resident scores, and `* loss` is the mean over batches of each
batch's float32 mean.  --weights all runs every weights_N.tar of the model directory in ascending N (run_ub_validation.sh's
loop); --csv FILE writes one row per checkpoint under training.csv's column names.
"""
import csv
import os
import re
import time
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from pathlib import Path

import numpy as np

from ..data import load_validation
from ..util import _model_dir, accuracy, decode_ref, init, load_model


CSV_COLUMNS = ("weights", "validation_loss", "validation_mean", "validation_median", "chunks", "duration")
MAX_POSITIONS = 2048            # target positions (width - state_len + 1) of one label row the loss kernel takes


def checkpoint_numbers(model_directory, spec):
    """--weights: a comma-separated list of checkpoint numbers, or `all` = the N of every weights_N.tar in the directory,
    ascending."""
    if spec != "all":
        return [int(i) for i in spec.split(",")]
    found = (re.fullmatch(r"weights_([0-9]+)\.tar", f) for f in os.listdir(_model_dir(str(model_directory))))
    numbers = sorted(int(m.group(1)) for m in found if m)
    if not numbers:
        raise SystemExit("> error: no weights_N.tar in '%s'" % model_directory)
    return numbers


def mean_of_batch_means(batch_losses):
    """validate_one_epoch's loss (training.py:178-180): every batch's float32 mean (the criterion's reduction), then the mean of
    those figures -- not the mean over all chunks when the last batch is short."""
    return float(np.mean([float(np.asarray(b, dtype=np.float32).mean(dtype=np.float32)) for b in batch_losses]))


def csv_row(weights, loss, accuracies, duration):
    return [str(weights), "%.6f" % loss, "%.4f" % np.mean(accuracies), "%.4f" % np.median(accuracies), str(len(accuracies)),
            "%.2f" % duration]


def write_csv(path, rows):
    with open(str(path), "w", newline="") as f:
        out = csv.writer(f)
        out.writerow(CSV_COLUMNS)
        out.writerows(rows)


def check_loss_inputs(targets, lengths, state_len):
    """What --loss refuses before any device work: label rows wider than the kernel's position limit, a chunk with fewer
    labels than the model's state length (no lattice position)."""
    width = np.asarray(targets).shape[1]
    if width - state_len + 1 > MAX_POSITIONS:
        raise SystemExit("> error: --loss: references.npy is %d labels wide, %d target positions; the loss takes %d positions"
                         % (width, width - state_len + 1, MAX_POSITIONS))
    short = np.flatnonzero(np.asarray(lengths) < state_len)
    if short.size:
        raise SystemExit("> error: --loss: chunk %d has %d labels, fewer than the model's state length %d"
                         % (short[0], np.asarray(lengths)[short[0]], state_len))


def main(args):
    if args.poa:
        raise SystemExit("> error: --poa (spoa consensus) is not part of the MI355X path")
    if args.csv and not args.loss:
        raise SystemExit("> error: --csv needs --loss (its rows carry validation_loss)")
    init(args.seed, args.device)
    print("* loading data")
    chunks, targets, lengths = load_validation(args.chunks, args.directory)
    chunks = np.asarray(chunks, dtype=np.float32)
    rows = []
    for w in checkpoint_numbers(args.model_directory, args.weights):
        print("* loading model", w)
        model = load_model(args.model_directory, args.device, weights=w)
        if args.loss:
            check_loss_inputs(targets, lengths, model.seqdist.state_len)
        print("* calling")
        t0 = time.perf_counter()
        seqs, losses = [], []
        for b0 in range(0, len(chunks), args.batchsize):
            batch = chunks[b0:b0 + args.batchsize]
            if args.loss:
                seq, lens, loss = model.validate_chunks(batch[:, None, :], targets[b0:b0 + args.batchsize],
                                                        lengths[b0:b0 + args.batchsize])
                losses.append(loss)
            else:
                seq, lens = model.basecall_chunks(batch[:, None, :])
            seqs.extend(seq[i, :lens[i]].tobytes().decode() for i in range(len(batch)))
        duration = time.perf_counter() - t0
        print("* decoding refs")
        refs = [decode_ref(t, model.alphabet) for t in targets]
        print("* computing accuracies")
        accuracies = [accuracy(ref, seq, min_coverage=args.min_coverage) if len(seq) else 0. for ref, seq in zip(refs, seqs)]
        print("* mean      %.2f%%" % np.mean(accuracies))
        print("* median    %.2f%%" % np.median(accuracies))
        if args.loss:
            print("* loss      %.4f" % mean_of_batch_means(losses))
            rows.append(csv_row(w, mean_of_batch_means(losses), accuracies, duration))
        print("* time      %.2f" % duration)
        print("* samples/s %.2E" % (len(chunks) * chunks.shape[1] / duration))
    if args.csv:
        write_csv(args.csv, rows)
    return accuracies


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("model_directory")
    parser.add_argument("--directory", type=Path)
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--seed", default=9, type=int)
    parser.add_argument("--weights", default="0", type=str)
    parser.add_argument("--chunks", default=1000, type=int)
    parser.add_argument("--batchsize", default=96, type=int)
    parser.add_argument("--beamsize", default=5, type=int)
    parser.add_argument("--poa", action="store_true", default=False)
    parser.add_argument("--min-coverage", default=0.5, type=float)
    parser.add_argument("--loss", action="store_true", default=False)
    parser.add_argument("--csv", default=None, type=Path)
    return parser
