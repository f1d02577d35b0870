"""CPU: xna_basecaller_amd/schedule.py against the factors torch's LambdaLR applied under the reference's own schedule.py
(tests/golden/lr_schedule.json, tests/golden/make_lr_schedule_golden.py): exact float64 equality at every step, and the
[lr_scheduler] table of a config."""
import json
import os

import pytest

from conftest import GOLDEN
from xna_basecaller_amd import schedule

CASES = json.load(open(os.path.join(GOLDEN, "lr_schedule.json")))


@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_factor_equals_the_recorded_one_at_every_step(case):
    total = case["steps_per_epoch"] * case["epochs"]
    assert len(case["factors"]) == total
    kwargs = dict(schedule.DEFAULTS, **case["kwargs"])
    got = [schedule.lr_factor(s, total, start_step=case["last_epoch"] * case["steps_per_epoch"], **kwargs) for s in range(total)]
    bad = [s for s in range(total) if got[s] != case["factors"][s]]
    assert not bad, (bad[:5], [(got[s], case["factors"][s]) for s in bad[:5]])


def test_the_cases_cover_what_they_are_named_for():
    by = {c["name"]: c for c in CASES}
    d = by["default"]
    assert d["steps_per_epoch"] * d["epochs"] > schedule.DEFAULTS["warmup_steps"] and d["factors"][0] == pytest.approx(0.1)
    w = by["warmup_longer_than_run"]
    assert w["steps_per_epoch"] * w["epochs"] < schedule.DEFAULTS["warmup_steps"]
    assert all(a < b for a, b in zip(w["factors"], w["factors"][1:]))            # never leaves the linear ramp
    assert by["resumed"]["last_epoch"] == 2


def test_config_table():
    assert schedule.from_config({}) == schedule.DEFAULTS
    assert schedule.from_config({"lr_scheduler": {}}) == schedule.DEFAULTS
    got = schedule.from_config({"lr_scheduler": {"package": "bonito.schedule", "symbol": "linear_warmup_cosine_decay",
                                                 "end_ratio": 0.05, "warmup_steps": 100}})
    assert got == {"end_ratio": 0.05, "warmup_steps": 100, "warmup_ratio": 0.1}
    for bad in ({"package": "bonito.schedule", "symbol": "linear_warmup_const_inverse_sqrt_decay"},
                {"package": "elsewhere", "symbol": "linear_warmup_cosine_decay"}, {"symbol": "linear_cooldown"}):
        with pytest.raises(ValueError, match="linear_warmup_cosine_decay"):
            schedule.from_config({"lr_scheduler": bad})
