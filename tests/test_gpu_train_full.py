"""GPU: `train --no-amp` without -F end to end on the synthetic ctc-data directory of tests/test_gpu_train_top.py (96 chunks of 1000
samples, features 32, batch 16): two epochs write the same files with the same columns and print no "freezing" line;
`evaluate --loss --weights 2` on the training directory reports the validation_loss training.csv holds -- every trained layer, the
convolutions included, reached the inference path before the validation pass and the checkpoint; in weights_2.tar every key
differs from the pretrained bytes; a rerun with -f continues at epoch 3."""
import csv

import numpy as np
import pytest
import torch

from conftest import encoder_shapes, make_config, seeded_state_dict
from xna_basecaller_amd import toml_lite
from xna_basecaller_amd.cli import evaluate, train

pytestmark = pytest.mark.gpu
F, L, N, B = 32, 1000, 96, 16


def test_two_epochs_evaluate_and_resume(tmp_path, capsys):
    labels = list("NACGT")
    cfg = make_config(F, labels)
    cfg["basecaller"] = {"batchsize": B, "chunksize": L, "overlap": 100}
    mdir = tmp_path / "pretrained"
    mdir.mkdir()
    (mdir / "config.toml").write_text(toml_lite.dumps(cfg))
    keys, shapes = encoder_shapes(F, 4)
    sd = seeded_state_dict(keys, shapes, seed=5)
    torch.save({k: torch.from_numpy(v) for k, v in sd.items()}, str(mdir / "weights_1.tar"))
    rng = np.random.default_rng(0)
    data = tmp_path / "ctc"
    data.mkdir()
    refs = np.zeros((N, 60), np.uint8)
    lens = rng.integers(20, 61, N).astype(np.uint16)
    for i in range(N):
        refs[i, :lens[i]] = rng.integers(1, 5, lens[i])
    np.save(data / "chunks.npy", rng.standard_normal((N, L)).astype(np.float32))
    np.save(data / "references.npy", refs)
    np.save(data / "reference_lengths.npy", lens)

    work = tmp_path / "run"
    argv = [str(work), "--pretrained", str(mdir), "--directory", str(data), "--no-amp", "--epochs", "2", "--batch", str(B)]
    train.main(train.argparser().parse_args(argv))
    out = capsys.readouterr().out
    assert "freezing" not in out and "Unfreezing" not in out
    assert "[epoch 1]" in out and "[epoch 2]" in out and "[epoch 3]" not in out
    for f in ("weights_1.tar", "weights_2.tar", "losses_1.csv", "losses_2.csv", "training.csv", "config.toml"):
        assert (work / f).exists(), f
    table = toml_lite.load(str(work / "config.toml"))["training"]
    assert table["epochs"] == 2 and table["freeze_bottom"] is False and table["no_amp"] is True
    n_train = int(np.floor(N * 0.97))
    steps = -(-n_train // B)
    for e in (1, 2):
        rows = list(csv.reader(open(work / ("losses_%d.csv" % e))))
        assert rows[0] == ["chunks", "time", "grad_norm", "lr", "loss"] and len(rows) == 1 + steps
        assert int(rows[-1][0]) == n_train and all(np.isfinite(float(x)) for r in rows[1:] for x in r)
    rows = list(csv.reader(open(work / "training.csv")))
    assert rows[0] == ["time", "duration", "epoch", "train_loss", "validation_loss", "validation_mean", "validation_median"]
    assert [r[2] for r in rows[1:]] == ["1", "2"]

    out_csv = tmp_path / "eval.csv"
    evaluate.main(evaluate.argparser().parse_args([str(work), "--directory", str(data), "--batchsize", str(B), "--loss", "--weights", "2",
                                                   "--csv", str(out_csv)]))
    capsys.readouterr()
    got = list(csv.reader(open(out_csv)))[1]
    assert got[0] == "2" and got[1] == "%.6f" % float(rows[2][4]), (got, rows[2])
    assert float(got[2]) == pytest.approx(float(rows[2][5]), abs=1e-3)

    trained = torch.load(str(work / "weights_2.tar"), map_location="cpu")
    assert list(trained) == keys
    for k in keys:                                                      # every layer trained
        assert np.isfinite(trained[k].numpy()).all() and trained[k].numpy().tobytes() != sd[k].tobytes(), k

    train.main(train.argparser().parse_args(argv + ["-f", "--epochs", "1"]))
    out = capsys.readouterr().out
    assert "[picking up weights state from epoch 2]" in out and "[epoch 3]" in out and "[epoch 4]" not in out
    assert (work / "weights_3.tar").exists() and (work / "losses_3.csv").exists()
    assert [r[2] for r in list(csv.reader(open(work / "training.csv")))[1:]] == ["1", "2", "3"]
    resumed = torch.load(str(work / "weights_3.tar"), map_location="cpu")
    for k in ("encoder.0.conv.weight", "encoder.1.conv.bias", "encoder.2.conv.weight", "encoder.4.rnn.weight_hh_l0", "encoder.9.linear.weight"):
        assert resumed[k].numpy().tobytes() != trained[k].numpy().tobytes(), k
