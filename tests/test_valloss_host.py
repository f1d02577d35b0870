"""CPU: the host side of `evaluate --loss` -- the three entry points of the validation loss in the header, the binding's
list and the built library; the evaluator's new flags, its checkpoint expansion, the loss aggregation of validate_one_epoch
(training.py:175-181) and the CSV it writes."""
import ctypes
import os
import re

import numpy as np
import pytest

from conftest import ROOT
from xna_basecaller_amd import _lib
from xna_basecaller_amd.cli import evaluate

NEW = ("xb_ctc_loss", "xb_ctc_loss_dev", "xb_validate_chunks")


def test_validation_loss_symbols_declared_listed_and_exported():
    text = open(os.path.join(ROOT, "include", "xna_basecaller.h")).read()
    declared = set(re.findall(r"XB_API\s+[\w\s\*]+?\b(xb_\w+)\s*\(", text))
    lib = ctypes.CDLL(_lib.LIB_PATH)
    for name in NEW:
        assert name in declared, name
        assert name in _lib.EXPORTS, name
        assert hasattr(lib, name), name
    # the label rows travel as uint8, the lengths as int32, in all three prototypes
    for name in NEW:
        proto = re.search(r"XB_API int %s\((.*?)\);" % name, text, re.S).group(1)
        assert "const uint8_t *" in proto and "int Lt" in proto and "const int32_t *" in proto, proto
    loaded = _lib.load()
    assert len(loaded.xb_ctc_loss.argtypes) == 10 and len(loaded.xb_ctc_loss_dev.argtypes) == 10
    assert len(loaded.xb_validate_chunks.argtypes) == 10
    # argument validation happens before any device work
    assert loaded.xb_ctc_loss(None, None, 1, 1, 1, None, 3, None, None, None) == _lib.XB_ERR_INVALID
    assert loaded.xb_validate_chunks(None, None, 1, b"NACGT", None, 3, None, None, None, None) == _lib.XB_ERR_INVALID


def test_evaluate_argparser_takes_the_new_flags():
    p = evaluate.argparser()
    a = p.parse_args(["model_dir", "--directory", "d"])
    assert (a.loss, a.csv) == (False, None)
    assert (a.device, a.seed, a.weights, a.chunks, a.batchsize, a.beamsize, a.poa, a.min_coverage) == \
        ("cuda", 9, "0", 1000, 96, 5, False, 0.5)
    b = p.parse_args(["model_dir", "--directory", "d", "--loss", "--csv", "out.csv", "--weights", "all"])
    assert b.loss is True and str(b.csv) == "out.csv" and b.weights == "all"


def test_csv_without_loss_exits_with_a_message():
    a = evaluate.argparser().parse_args(["model_dir", "--directory", "d", "--csv", "out.csv"])
    with pytest.raises(SystemExit) as e:
        evaluate.main(a)
    assert "--csv needs --loss" in str(e.value)


def test_weights_all_expands_to_the_sorted_checkpoints(tmp_path):
    for name in ("weights_10.tar", "weights_2.tar", "weights_x.tar", "config.toml", "weights_3.tar.bak"):
        (tmp_path / name).write_bytes(b"")
    assert evaluate.checkpoint_numbers(tmp_path, "all") == [2, 10]
    assert evaluate.checkpoint_numbers(tmp_path, "7,3") == [7, 3]          # a list keeps the order it was given in
    empty = tmp_path / "none"
    empty.mkdir()
    with pytest.raises(SystemExit):
        evaluate.checkpoint_numbers(empty, "all")


def test_loss_is_the_mean_of_batch_means():
    """Two uneven batches: (1 + 2 + 3) / 3 = 2 and 10 / 1 = 10 -> 6, where the mean over all four chunks is 4."""
    batches = [np.array([1.0, 2.0, 3.0], np.float32), np.array([10.0], np.float32)]
    assert evaluate.mean_of_batch_means(batches) == 6.0
    assert float(np.concatenate(batches).mean()) == 4.0
    # every batch mean is taken in float32, as the criterion's reduction is
    b = [np.array([0.1, 0.2, 0.4], np.float32)]
    assert evaluate.mean_of_batch_means(b) == float(b[0].mean(dtype=np.float32))


def test_csv_header_and_row(tmp_path):
    assert evaluate.CSV_COLUMNS == ("weights", "validation_loss", "validation_mean", "validation_median", "chunks", "duration")
    row = evaluate.csv_row(7, 0.12345678, [100.0, 50.0, 75.123456], 3.14159)
    assert row == ["7", "0.123457", "75.0412", "75.1235", "3", "3.14"]
    evaluate.write_csv(tmp_path / "v.csv", [row, evaluate.csv_row(9, 1.0, [90.0], 1.0)])
    lines = (tmp_path / "v.csv").read_text().splitlines()
    assert lines == ["weights,validation_loss,validation_mean,validation_median,chunks,duration",
                     "7,0.123457,75.0412,75.1235,3,3.14", "9,1.000000,90.0000,90.0000,1,1.00"]


def test_loss_inputs_refused_before_any_device_work():
    t = np.ones((4, 12), np.uint8)
    evaluate.check_loss_inputs(t, np.array([12, 3, 5, 3]), 3)
    with pytest.raises(SystemExit) as e:
        evaluate.check_loss_inputs(t, np.array([12, 3, 2, 1]), 3)
    assert "chunk 2 " in str(e.value) and "state length 3" in str(e.value)
    wide = np.ones((1, evaluate.MAX_POSITIONS + 3), np.uint8)
    with pytest.raises(SystemExit) as e:
        evaluate.check_loss_inputs(wide, np.array([5]), 3)
    assert "%d positions" % evaluate.MAX_POSITIONS in str(e.value)
    evaluate.check_loss_inputs(wide[:, :-1], np.array([5]), 3)             # exactly the limit
