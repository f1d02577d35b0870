"""
`bonito train TRAINING_DIR --pretrained MODEL_DIR --directory CTC_DATA -F` (ub-bonito/bonito/cli/train.py, training.py): fine-tune
a pretrained model with its bottom layers frozen and the top layer with parameters -- the CRF head, encoder.9.linear -- trainable
(--num-unfreeze-top 1, the reference's default).  That recipe needs no backward pass through the recurrence: a step is one
device call (Model.head_trainer, xb_head_train_step).  --num-unfreeze-top K for K in 2 .. 6 together with --no-amp trains the
head and the top K - 1 LSTM layers, float32 throughout above the frozen bottom (the reference's --no-amp; its default, autocast
with a GradScaler, is not implemented): again one device call per step (Model.top_trainer, xb_top_train_step).  The trained
layers are loaded into the inference path before each epoch's validation and checkpoint (Trainer.publish; the head recipe's
step has already put them there, and publish only refreshes the model's parameters).  Without -F and
with --no-amp EVERY layer trains -- the reference's headline recipes, which never pass -f: the convolutions too have their
float32 forward and backward on the device (Model.full_trainer, xb_full_train_begin), one device call per step as before.

Per epoch, as Trainer.fit: losses_N.csv (chunks, time, grad_norm, lr, loss per step), weights_N.tar (torch.save of the state
dict), the validation pass (evaluate --loss's path, xb_validate_chunks, with the new weights), a training.csv row and the
`[epoch N]` line.  config.toml of the pretrained model goes to TRAINING_DIR with a [training] table of the arguments.  A rerun
with -f continues after the highest weights_N.tar (load_state); AdamW's moments start from zero then, as in the reference
without --restore-optim.  The schedule is linear_warmup_cosine_decay (schedule.py); the shuffle is a numpy permutation seeded
with --seed, drawn once per epoch.

Refused, each with the alternative: training without -F and without --no-amp, or without -F with a --num-unfreeze-top (which the
reference would silently ignore), --num-unfreeze-top 2 .. 6 without --no-amp, --num-unfreeze-top below 1 or above 6 (a partial
unfreeze of the conv stack; drop -F to train every layer), --config (training from scratch),
--grad-accum-split other than 1, --restore-optim, a nonzero drop rate, --skip-top, and the --spike / --stitch-mode family
(run `spike`, `synth` or `splice` beforehand: the augmentation is then fixed per data set, not redrawn per epoch).
"""
import csv
import os
import re
import time
from argparse import ArgumentDefaultsHelpFormatter, ArgumentParser
from datetime import datetime
from pathlib import Path

import numpy as np

from .. import schedule, toml_lite
from ..data import load_numpy_datasets
from ..util import _model_dir, accuracy, decode_ref, init, load_model
from .evaluate import check_loss_inputs, mean_of_batch_means

LOSS_COLUMNS = ("chunks", "time", "grad_norm", "lr", "loss")
TRAINING_COLUMNS = ("time", "duration", "epoch", "train_loss", "validation_loss", "validation_mean", "validation_median")


def refusals(args):
    """The first thing main does, before any file or device is touched: every recipe outside `-F --num-unfreeze-top 1`,
    `-F --num-unfreeze-top 2 .. 6 --no-amp` and `--no-amp` without -F (every layer)."""
    def no(msg):
        raise SystemExit("> error: " + msg)

    if args.config:
        no("--config trains a model from scratch, which needs backward passes through the whole encoder; this package fine-tunes "
           "the head of a pretrained model: use --pretrained MODEL_DIR -F")
    if not args.pretrained:
        no("--pretrained MODEL_DIR is required: only fine-tuning of a pretrained model's head is implemented")
    if not args.freeze_bottom and not args.no_amp:
        no("training every layer is float32 here (no autocast, no GradScaler): add --no-amp to train every layer, or "
           "use -F (--freeze-bottom) to train the CRF head alone, or with --num-unfreeze-top 2 .. 6 --no-amp the top LSTM layers too")
    if not args.freeze_bottom and args.num_unfreeze_top != 1:
        no("--num-unfreeze-top %d without -F: every layer trains when the bottom is not frozen, and the reference would silently "
           "ignore the flag; drop it, or use -F (--freeze-bottom) with it" % args.num_unfreeze_top)
    if args.num_unfreeze_top < 1:
        no("--num-unfreeze-top %d: at least the top layer is trained; use --num-unfreeze-top 1 .. 6" % args.num_unfreeze_top)
    if args.num_unfreeze_top > 6:
        no("--num-unfreeze-top %d would unfreeze some of the convolutions, and a partial unfreeze of the conv stack is not "
           "implemented; the most with -F is --num-unfreeze-top 6 --no-amp (the head and all five LSTM layers), or drop -F to train "
           "every layer (--no-amp)" % args.num_unfreeze_top)
    if args.num_unfreeze_top > 1 and not args.no_amp:
        no("--num-unfreeze-top %d unfreezes LSTM layers, whose backward pass is float32 here (no autocast, no GradScaler): add "
           "--no-amp, or train the head alone with --num-unfreeze-top 1" % args.num_unfreeze_top)
    if args.grad_accum_split != 1:
        no("--grad-accum-split %d: a step is one device pass over the whole batch; lower --batch instead" % args.grad_accum_split)
    if args.restore_optim:
        no("--restore-optim: no optim_N.tar is written; a resumed run restarts AdamW's moments, as the reference does without this flag")
    if args.drop_rate or args.drop_rate_bottom:
        no("--drop-rate / --drop-rate-bottom: dropout is not implemented (the frozen encoder runs in its inference form); leave them unset")
    if args.skip_top:
        no("--skip-top would train a freshly initialised head; start from the pretrained head (drop the flag)")
    if args.spike or args.fully_synth or args.stitch_mode or args.prop_ubs:
        no("--spike / --fully_synth / --stitch-mode / --prop-ubs: augmentation is not drawn during training; write the augmented "
           "ctc-data beforehand with the `spike`, `synth` or `splice` command and pass it as --directory")


def load_training_data(directory, chunks=0, valid_chunks=0):
    """load_numpy (data.py:100-126): (train, valid), each (chunks, targets, lengths); DIRECTORY/validation when it is there,
    otherwise the last 3 % of the (limited) arrays are the validation set and the first 97 % the training set."""
    directory = str(directory)
    train = load_numpy_datasets(limit=chunks or None, directory=directory)
    sub = os.path.join(directory, "validation")
    if os.path.exists(sub):
        valid = load_numpy_datasets(directory=sub)
    else:
        print("[validation set not found: splitting training set (97%-3%)]")
        split = int(np.floor(len(train[0]) * 0.97))
        train, valid = tuple(x[:split] for x in train), tuple(x[split:] for x in train)
    if valid_chunks:
        valid = tuple(x[:valid_chunks] for x in valid)
    return train, valid


def last_epoch(workdir):
    """load_state's epoch (training.py:24-69): the highest N of weights_N.tar in the training directory, 0 without one."""
    found = (re.fullmatch(r"weights_([0-9]+)\.tar", f) for f in os.listdir(workdir))
    return max((int(m.group(1)) for m in found if m), default=0)


def append_row(path, columns, row):
    """bonito.io.CSVLogger: append one row, the header first when the file is new."""
    new = not os.path.exists(path)
    with open(path, "a", newline="") as f:
        out = csv.writer(f)
        if new:
            out.writerow(columns)
        out.writerow(row)


def training_table(args):
    return {k: (str(v) if isinstance(v, Path) else v) for k, v in vars(args).items()
            if v is not None and k not in ("func", "command") and isinstance(v, (bool, int, float, str, list, Path))}


def validate(model, valid, batch):
    """validate_one_epoch (training.py:175-181) through xb_validate_chunks: (loss, mean accuracy, median accuracy)."""
    chunks, targets, lengths = valid
    seqs, losses = [], []
    for b0 in range(0, len(chunks), batch):
        seq, lens, loss = model.validate_chunks(chunks[b0:b0 + batch, None, :], targets[b0:b0 + batch], lengths[b0:b0 + batch])
        losses.append(loss)
        seqs.extend(seq[i, :lens[i]].tobytes().decode() for i in range(len(lens)))
    refs = [decode_ref(t, model.alphabet) for t in targets]
    accs = [accuracy(ref, seq, min_coverage=0.5) if len(seq) else 0. for ref, seq in zip(refs, seqs)]
    return mean_of_batch_means(losses), float(np.mean(accs)), float(np.median(accs))


def main(args):
    refusals(args)
    workdir = os.path.expanduser(args.training_directory)
    if os.path.exists(workdir) and not args.force:
        print("[error] %s exists, use -f to force continue training." % workdir)
        raise SystemExit(1)
    pretrained = _model_dir(args.pretrained)
    config = toml_lite.load(os.path.join(pretrained, "config.toml"))
    enc = config.get("encoder", {})
    if enc.get("drop_rate") or enc.get("drop_rate_bottom"):
        raise SystemExit("> error: %s/config.toml sets a nonzero drop rate; dropout is not implemented: set [encoder] drop_rate = 0"
                         % pretrained)
    try:
        sched = schedule.from_config(config)
    except ValueError as e:
        raise SystemExit("> error: %s" % e)

    init(args.seed, args.device)
    print("[loading data]")
    train, valid = load_training_data(args.directory, args.chunks, args.valid_chunks)
    train = (np.asarray(train[0], dtype=np.float32), np.asarray(train[1]), np.asarray(train[2]))
    valid = (np.asarray(valid[0], dtype=np.float32), np.asarray(valid[1]), np.asarray(valid[2]))
    if not len(train[0]) or not len(valid[0]):
        raise SystemExit("> error: %d training and %d validation chunks: both sets need at least one" % (len(train[0]), len(valid[0])))

    os.makedirs(workdir, exist_ok=True)
    with open(os.path.join(workdir, "config.toml"), "w") as f:
        f.write(toml_lite.dumps({**config, "training": training_table(args)}))

    print("[loading model]")
    print("[using pretrained model {}]".format(args.pretrained))
    model = load_model(pretrained, args.device, half=False)
    start = last_epoch(workdir)
    if start:
        print("[picking up weights state from epoch %s]" % start)
        resumed = load_model(workdir, args.device, weights=start, half=False)
        model.load_state_dict(resumed.state_dict())
        model.to(args.device)
    for t, l in ((train[1], train[2]), (valid[1], valid[2])):
        check_loss_inputs(t, l, model.seqdist.state_len)
    full = not args.freeze_bottom                               # every layer (refusals: --no-amp is set then)
    top_layers = args.num_unfreeze_top - 1                      # LSTM layers trained beside the head
    if not full:
        print("[WARNING: freezing bottom layers]")
        print("> > Unfreezing top/last %d layer(s):\n> > %s" % (args.num_unfreeze_top, ", ".join(["linearcrfencoder"] + ["lstm"] * top_layers)))
    print("> batch_size: {} | epochs: {} | lr: {}".format(args.batch, args.epochs, args.lr))

    n = len(train[0])
    steps_per_epoch = -(-n // args.batch)
    total_steps = args.epochs * steps_per_epoch
    if full:
        trainer = model.full_trainer(train[0].shape[1], args.batch)
    elif top_layers:
        trainer = model.top_trainer(top_layers, train[0].shape[1], args.batch)
    else:
        trainer = model.head_trainer(train[0].shape[1], args.batch)
    import torch  # the checkpoint container only
    rng = np.random.default_rng(args.seed)
    step = 0
    for epoch in range(1 + start, args.epochs + 1 + start):
        order = rng.permutation(n)
        t0 = time.perf_counter()
        seen, smoothed = 0, None
        log = os.path.join(workdir, "losses_%d.csv" % epoch)
        if os.path.exists(log):
            os.remove(log)
        for b0 in range(0, n, args.batch):
            idx = np.sort(order[b0:b0 + args.batch])            # (sorted: one pass over the arrays; the step sums over the batch)
            lr = args.lr * schedule.lr_factor(step, total_steps, start_step=start * steps_per_epoch, **sched)
            loss, grad_norm = trainer.step(train[0][idx, None, :], train[1][idx], train[2][idx], lr)
            step += 1
            seen += len(idx)
            smoothed = loss if smoothed is None else 0.01 * loss + 0.99 * smoothed
            append_row(log, LOSS_COLUMNS, [seen, time.perf_counter() - t0, grad_norm, lr, loss])
        duration = time.perf_counter() - t0
        trainer.publish()                                       # the validation below and the model's parameters see the trained layers
        torch.save(trainer.state_dict(), os.path.join(workdir, "weights_%d.tar" % epoch))
        val_loss, val_mean, val_median = validate(model, valid, args.batch)
        print("[epoch {}] directory={} loss={:.4f} mean_acc={:.3f}% median_acc={:.3f}%".format(
            epoch, workdir, val_loss, val_mean, val_median))
        append_row(os.path.join(workdir, "training.csv"), TRAINING_COLUMNS,
                   [datetime.today(), int(duration), epoch, smoothed, val_loss, val_mean, val_median])
    trainer.close()


def argparser():
    parser = ArgumentParser(formatter_class=ArgumentDefaultsHelpFormatter, add_help=False)
    parser.add_argument("training_directory")
    group = parser.add_mutually_exclusive_group()
    group.add_argument("--config", default=None)
    group.add_argument("--pretrained", default="")
    parser.add_argument("--directory", type=Path)
    parser.add_argument("--device", default="cuda")
    parser.add_argument("--lr", default=2e-3, type=float)
    parser.add_argument("--seed", default=25, type=int)
    parser.add_argument("--epochs", default=5, type=int)
    parser.add_argument("--batch", default=128, type=int)
    parser.add_argument("--chunks", default=0, type=int)
    parser.add_argument("--valid-chunks", default=0, type=int)
    parser.add_argument("--no-amp", action="store_true", default=False)
    parser.add_argument("-f", "--force", action="store_true", default=False)
    parser.add_argument("--restore-optim", action="store_true", default=False)
    parser.add_argument("--grad-accum-split", default=1, type=int)
    parser.add_argument("-F", "--freeze-bottom", action="store_true", default=False)
    parser.add_argument("--num-unfreeze-top", default=1, type=int)
    parser.add_argument("--drop-rate", default=None, type=float)
    parser.add_argument("--drop-rate-bottom", default=None, type=float)
    parser.add_argument("--skip-top", action="store_true", default=False)
    # accepted only to be refused with the alternative (the reference draws these augmentations inside its data loader)
    parser.add_argument("--spike", action="store_true", default=False)
    parser.add_argument("--fully_synth", action="store_true", default=False)
    parser.add_argument("--prop-ubs", type=float, default=0)
    parser.add_argument("--stitch-mode", type=str, default=None)
    return parser
