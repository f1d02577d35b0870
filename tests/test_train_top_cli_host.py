"""CPU: `train -F --num-unfreeze-top K` (xna_basecaller_amd/cli/train.py).  K in 2 .. 6 trains LSTM layers in float32, which is the
reference's --no-amp: without that flag it is refused with both alternatives named; K = 7 (the convolutions) and K = 0 are
refused; with --no-amp, K = 2 .. 6 gets past the refusals.  All before a device context exists."""
import pytest

from xna_basecaller_amd import _lib
from xna_basecaller_amd.cli import train

BASE = ["out_dir", "--pretrained", "model_dir", "--directory", "ctc", "-F"]


@pytest.fixture
def no_context(monkeypatch):
    def boom(*a, **k):
        raise AssertionError("a device context was created")
    monkeypatch.setattr(_lib, "Context", boom)
    monkeypatch.setattr(_lib, "require_gpu", boom)


def _refused(argv, tmp_path, monkeypatch):
    monkeypatch.chdir(tmp_path)
    with pytest.raises(SystemExit) as e:
        train.main(train.argparser().parse_args(argv))
    msg = str(e.value.code)
    assert e.value.code not in (0, None) and msg.startswith("> error: ")
    assert not (tmp_path / "out_dir").exists()
    return msg


@pytest.mark.parametrize("K", [2, 3, 4, 5, 6])
def test_lstm_layers_without_no_amp_are_refused_with_both_alternatives(K, no_context, tmp_path, monkeypatch):
    msg = _refused(BASE + ["--num-unfreeze-top", str(K)], tmp_path, monkeypatch)
    assert "--no-amp" in msg and "--num-unfreeze-top 1" in msg and "--num-unfreeze-top %d" % K in msg


@pytest.mark.parametrize("extra", [[], ["--no-amp"]], ids=["amp", "no-amp"])
def test_the_convolutions_and_no_layer_at_all_are_refused(extra, no_context, tmp_path, monkeypatch):
    msg = _refused(BASE + ["--num-unfreeze-top", "7"] + extra, tmp_path, monkeypatch)
    assert "convolutions" in msg and "--num-unfreeze-top 6" in msg
    msg = _refused(BASE + ["--num-unfreeze-top", "0"] + extra, tmp_path, monkeypatch)
    assert "--num-unfreeze-top 1" in msg


@pytest.mark.parametrize("K", [1, 2, 3, 6])
def test_no_amp_gets_past_the_refusals(K, no_context):
    args = train.argparser().parse_args(BASE + ["--num-unfreeze-top", str(K), "--no-amp"])
    assert args.no_amp and train.refusals(args) is None


def test_the_other_refusals_hold_with_no_amp(no_context, tmp_path, monkeypatch):
    msg = _refused(BASE + ["--num-unfreeze-top", "3", "--no-amp", "--grad-accum-split", "2"], tmp_path, monkeypatch)
    assert "lower --batch" in msg
    msg = _refused(["out_dir", "--pretrained", "model_dir", "--directory", "ctc", "--num-unfreeze-top", "3", "--no-amp"], tmp_path, monkeypatch)
    assert "use -F" in msg
