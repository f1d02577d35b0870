"""CPU: `train --no-amp` without -F (xna_basecaller_amd/cli/train.py) trains every layer and gets past the refusals; without --no-amp,
with a --num-unfreeze-top beside it, and at -F --num-unfreeze-top 7 and above it is refused with the alternatives named.  All before
a device context exists."""
import pytest

from xna_basecaller_amd import _lib
from xna_basecaller_amd.cli import train
from xna_basecaller_amd.crf.trainer import CONV_KEYS, full_keys, top_keys

BASE = ["out_dir", "--pretrained", "model_dir", "--directory", "ctc"]


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


def test_every_layer_with_no_amp_gets_past_the_refusals(no_context):
    args = train.argparser().parse_args(BASE + ["--no-amp"])
    assert args.no_amp and not args.freeze_bottom and train.refusals(args) is None


def test_every_layer_without_no_amp_is_refused_with_both_alternatives(no_context, tmp_path, monkeypatch):
    msg = _refused(BASE, tmp_path, monkeypatch)
    assert "use -F" in msg and "--no-amp" in msg and "every layer" in msg


@pytest.mark.parametrize("K", [0, 2, 6, 7])
def test_num_unfreeze_top_without_freeze_bottom_is_refused(K, no_context, tmp_path, monkeypatch):
    msg = _refused(BASE + ["--no-amp", "--num-unfreeze-top", str(K)], tmp_path, monkeypatch)
    assert "use -F" in msg and "--num-unfreeze-top %d" % K in msg


@pytest.mark.parametrize("K", [7, 9])
def test_a_partial_unfreeze_of_the_conv_stack_is_refused(K, no_context, tmp_path, monkeypatch):
    msg = _refused(BASE + ["-F", "--no-amp", "--num-unfreeze-top", str(K)], tmp_path, monkeypatch)
    assert "convolutions" in msg and "--num-unfreeze-top 6" in msg and "drop -F" in msg


@pytest.mark.parametrize("extra,needle", [(["--grad-accum-split", "2"], "lower --batch"), (["--restore-optim"], "optim_N.tar"), (["--drop-rate", "0.1"], "dropout"),
                                          (["--skip-top"], "pretrained head"), (["--spike"], "`spike`")])
def test_the_other_refusals_hold_for_every_layer(extra, needle, no_context, tmp_path, monkeypatch):
    assert needle in _refused(BASE + ["--no-amp"] + extra, tmp_path, monkeypatch)
    msg = _refused(["out_dir", "--config", "c.toml", "--directory", "ctc", "--no-amp"], tmp_path, monkeypatch)
    assert "--config" in msg


def test_the_trainers_keys_are_the_state_dicts():
    from xna_basecaller_amd.synthetic import encoder_shapes
    keys, _ = encoder_shapes(32, 4)
    assert full_keys() == keys and len(keys) == 28 and full_keys()[:6] == list(CONV_KEYS) and full_keys()[6:] == top_keys(5)
