"""The learning-rate schedule of `train`: the reference's default, linear_warmup_cosine_decay through func_scheduler
(schedule.py:7-17, 110-120), as a plain function of the step -- the factor LambdaLR multiplies the base rate by.  Restated
operation by operation: tests/test_schedule_train_host.py holds it to recorded factors with exact float64 equality."""
import numpy as np

DEFAULTS = {"end_ratio": 0.01, "warmup_steps": 500, "warmup_ratio": 0.1}
SYMBOL = "linear_warmup_cosine_decay"


def _cosine(t, y0, y1):
    return y1 + 0.5 * (y0 - y1) * (np.cos(t * np.pi) + 1.0)


def lr_factor(step, total_steps, start_step=0, end_ratio=0.01, warmup_steps=500, warmup_ratio=0.1):
    """The factor at scheduler step `step` (0 for the first optimiser step) of a run of total_steps = epochs * steps per epoch
    that resumes after start_step = last_epoch * steps per epoch."""
    t = (step + start_step) / total_steps
    if not warmup_steps:
        return float(_cosine(t, 1.0, end_ratio))
    y0 = _cosine(0.0, 1.0, end_ratio)
    knot = warmup_steps / total_steps
    if t <= knot:                          # piecewise_schedule: np.searchsorted([knot], t) == 0
        u = (t - 0.0) / (knot - 0.0)
        return float(warmup_ratio * y0 + (y0 - warmup_ratio * y0) * u)
    u = (t - knot) / (1.0 - knot)
    return float(_cosine(u, 1.0, end_ratio))


def from_config(config):
    """Keyword arguments of lr_factor from a model config: [lr_scheduler] may name linear_warmup_cosine_decay (with end_ratio,
    warmup_steps); any other schedule is refused."""
    sched = dict((config or {}).get("lr_scheduler") or {})
    if not sched:
        return dict(DEFAULTS)
    symbol = sched.get("symbol")
    if symbol != SYMBOL or sched.get("package", "bonito.schedule") != "bonito.schedule":
        raise ValueError("[lr_scheduler] %s.%s is not supported: train implements %s only; remove the table or name that schedule"
                         % (sched.get("package"), symbol, SYMBOL))
    out = dict(DEFAULTS)
    for k in ("end_ratio", "warmup_steps"):          # what linear_warmup_cosine_decay takes; the rest falls into its **kwargs
        if k in sched:
            out[k] = sched[k]
    return out
