"""CPU: every recipe `train` refuses exits non-zero with a message that names the alternative, before a device context exists
(xna_basecaller_amd/cli/train.py); the data split, the resume point and the CSV helper."""
import numpy as np
import pytest

from conftest import make_config
from xna_basecaller_amd import _lib, toml_lite
from xna_basecaller_amd.cli import train

BASE = ["out_dir", "--pretrained", "model_dir", "--directory", "ctc", "-F"]
REFUSED = [
    (["out_dir", "--pretrained", "model_dir", "--directory", "ctc"], "use -F"),
    (BASE + ["--num-unfreeze-top", "2"], "--num-unfreeze-top 1"),
    (["out_dir", "--config", "some.toml", "--directory", "ctc", "-F"], "--pretrained MODEL_DIR"),
    (["out_dir", "--directory", "ctc", "-F"], "--pretrained MODEL_DIR"),
    (BASE + ["--grad-accum-split", "2"], "lower --batch"),
    (BASE + ["--restore-optim"], "no optim_N.tar is written"),
    (BASE + ["--drop-rate", "0.1"], "leave them unset"),
    (BASE + ["--drop-rate-bottom", "0.2"], "leave them unset"),
    (BASE + ["--skip-top"], "drop the flag"),
    (BASE + ["--spike"], "`spike`, `synth` or `splice`"),
    (BASE + ["--fully_synth"], "`spike`, `synth` or `splice`"),
    (BASE + ["--prop-ubs", "0.05"], "`spike`, `synth` or `splice`"),
    (BASE + ["--stitch-mode", "per_kmer"], "`spike`, `synth` or `splice`"),
]


@pytest.fixture
def no_context(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(_lib, "Context", boom)
    monkeypatch.setattr(_lib, "require_gpu", boom)


@pytest.mark.parametrize("argv,needle", REFUSED, ids=[" ".join(a[0][5:] or a[0][1:3]) or "no -F" for a in REFUSED])
def test_refused_with_the_alternative(argv, needle, no_context, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        train.main(train.argparser().parse_args(argv))
    assert e.value.code not in (0, None) and str(e.value.code).startswith("> error: ") and needle in str(e.value.code)
    assert not (tmp_path / "out_dir").exists()


def _model_dir(tmp_path, **encoder):
    cfg = make_config(32)
    cfg["encoder"].update(encoder.pop("encoder", {}))
    cfg.update(encoder)
    d = tmp_path / "model_dir"
    d.mkdir()
    (d / "config.toml").write_text(toml_lite.dumps(cfg))
    return d


def test_config_drop_rate_and_foreign_schedule_are_refused(no_context, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    _model_dir(tmp_path, encoder={"drop_rate": 0.1})
    with pytest.raises(SystemExit) as e:
        train.main(train.argparser().parse_args(BASE))
    assert "drop_rate = 0" in str(e.value.code) and not (tmp_path / "out_dir").exists()
    (tmp_path / "model_dir" / "config.toml").write_text(toml_lite.dumps(dict(
        make_config(32), lr_scheduler={"package": "bonito.schedule", "symbol": "linear_cooldown"})))
    with pytest.raises(SystemExit) as e:
        train.main(train.argparser().parse_args(BASE))
    assert "linear_warmup_cosine_decay" in str(e.value.code) and not (tmp_path / "out_dir").exists()


def test_existing_directory_needs_force(no_context, tmp_path, monkeypatch, capsys):
    monkeypatch.chdir(tmp_path)
    (tmp_path / "out_dir").mkdir()
    with pytest.raises(SystemExit) as e:
        train.main(train.argparser().parse_args(BASE))
    assert e.value.code == 1 and "use -f to force continue training" in capsys.readouterr().out


def test_split_resume_point_and_csv(tmp_path):
    d = tmp_path / "ctc"
    d.mkdir()
    np.save(d / "chunks.npy", np.arange(200 * 4, dtype=np.float32).reshape(200, 4))
    np.save(d / "references.npy", np.ones((200, 3), np.uint8))
    np.save(d / "reference_lengths.npy", np.full(200, 3, np.uint16))
    tr, va = train.load_training_data(d)
    assert len(tr[0]) == 194 and len(va[0]) == 6 and va[0][0, 0] == 194 * 4
    tr, va = train.load_training_data(d, chunks=100, valid_chunks=2)
    assert len(tr[0]) == 97 and len(va[0]) == 2
    (d / "validation").mkdir()
    for f in ("chunks.npy", "references.npy", "reference_lengths.npy"):
        np.save(d / "validation" / f, np.load(d / f)[:10])
    tr, va = train.load_training_data(d)
    assert len(tr[0]) == 200 and len(va[0]) == 10

    w = tmp_path / "work"
    w.mkdir()
    assert train.last_epoch(w) == 0
    for name in ("weights_2.tar", "weights_11.tar", "weights_x.tar", "optim_20.tar"):
        (w / name).write_text("")
    assert train.last_epoch(w) == 11
    log = w / "training.csv"
    train.append_row(str(log), train.TRAINING_COLUMNS, [1, 2, 3, 4, 5, 6, 7])
    train.append_row(str(log), train.TRAINING_COLUMNS, [8, 9, 10, 11, 12, 13, 14])
    assert log.read_text().splitlines() == ["time,duration,epoch,train_loss,validation_loss,validation_mean,validation_median",
                                            "1,2,3,4,5,6,7", "8,9,10,11,12,13,14"]
