"""Writes tests/golden/lr_schedule.json: the factor torch's LambdaLR applies at every step under the reference's default
schedule (bonito/schedule.py: linear_warmup_cosine_decay), recorded by running the reference's own schedule.py.

    python tests/golden/make_lr_schedule_golden.py PATH/TO/bonito/schedule.py

Three configurations: the default warm-up inside a longer run, a warm-up longer than the run, and a run that resumes after
last_epoch = 2.  Only the recorded numbers are committed."""
import importlib.util
import json
import os
import sys

import torch

CASES = [
    {"name": "default", "steps_per_epoch": 300, "epochs": 5, "last_epoch": 0, "kwargs": {}},
    {"name": "warmup_longer_than_run", "steps_per_epoch": 40, "epochs": 3, "last_epoch": 0, "kwargs": {}},
    {"name": "resumed", "steps_per_epoch": 130, "epochs": 4, "last_epoch": 2, "kwargs": {"end_ratio": 0.05, "warmup_steps": 100}},
]


def main(path):
    spec = importlib.util.spec_from_file_location("reference_schedule", path)
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    out = []
    for case in CASES:
        opt = torch.optim.SGD([torch.nn.Parameter(torch.zeros(1))], lr=1.0)      # base rate 1: the rate IS the factor
        loader = range(case["steps_per_epoch"])
        sched = mod.linear_warmup_cosine_decay(**case["kwargs"])(opt, loader, case["epochs"], case["last_epoch"])
        factors = []
        for _ in range(case["steps_per_epoch"] * case["epochs"]):
            factors.append(float(sched.get_last_lr()[0]))
            opt.step()
            sched.step()
        out.append(dict(case, factors=factors))
    dst = os.path.join(os.path.dirname(os.path.abspath(__file__)), "lr_schedule.json")
    with open(dst, "w") as f:
        json.dump(out, f)
    print("wrote", dst, [len(c["factors"]) for c in out])


if __name__ == "__main__":
    main(sys.argv[1])
