"""xb_adamw_step_dev (include/xna_basecaller.h) in numpy, operation by operation in fp32: torch.optim.AdamW's single-tensor update
with torch's defaults (betas 0.9 / 0.999, eps 1e-8, weight decay 0.01).  The device is held to this text bit for bit
(tests/test_gpu_headtrain.py); this text is held to torch on the CPU (tests/test_adamw_host.py)."""
import math

import numpy as np

B1, B2 = np.float32(0.9), np.float32(0.999)
C1, C2 = np.float32(1.0 - 0.9), np.float32(1.0 - 0.999)
EPS = np.float32(1e-8)
MAX_NORM = 2.0


def scalars(lr, step, weight_decay=0.01):
    """(decay, step_size, bc2_sqrt) of step 1, 2, .. at learning rate lr: computed in double, rounded once."""
    lr = float(lr)
    return (np.float32(1.0 - lr * weight_decay), np.float32(lr / (1.0 - 0.9 ** step)),
            np.float32(math.sqrt(1.0 - 0.999 ** step)))


def clip_factor(norm):
    """clip_grad_norm_(max_norm = 2.0)'s factor from the fp32 norm: computed in double, rounded once."""
    return np.float32(min(1.0, MAX_NORM / (float(np.float32(norm)) + 1e-6)))


def step(p, g, m, v, clip, decay, step_size, bc2_sqrt):
    """One update of fp32 arrays -> new (p, g, m, v); g is the clipped gradient."""
    p, g, m, v = (np.asarray(a, np.float32) for a in (p, g, m, v))
    clip, decay, step_size, bc2_sqrt = (np.float32(s) for s in (clip, decay, step_size, bc2_sqrt))
    g = g * clip
    p = p * decay
    m = B1 * m + C1 * g
    v = B2 * v + (C2 * g) * g
    den = np.sqrt(v) / bc2_sqrt + EPS
    p = p - (step_size * m) / den
    return p, g, m, v
