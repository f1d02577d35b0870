"""CPU: tests/adamw_ref.py -- the text xb_adamw_step_dev is held to bit for bit -- against torch.optim.AdamW(foreach=False) over
50 steps with random gradients, a varying learning rate and clipping.

Measured on the CPU (torch 2.x): the largest deviation of a parameter from torch's is 2.0 ulps of the parameter (MEASURED_ULPS) over
50 steps of parameters of magnitude 0.5 .. 1 (torch forms the first moment by lerp, m + (1 - beta1) (g - m), and scales by 1 / bias_correction where this text
divides); the assertion is 4 x that."""
import numpy as np
import torch

import adamw_ref as A

MEASURED_ULPS = 2.0          # measured: three seeds, 4096 parameters, 50 steps
STEPS = 50


def _run(seed, n=4096):
    rng = np.random.default_rng(seed)
    # magnitudes in [0.5, 1): 50 steps of at most lr each never bring a parameter near zero, where an ulp of it means nothing
    p0 = (rng.uniform(0.5, 1.0, n) * rng.choice([-1.0, 1.0], n)).astype(np.float32)
    tp = torch.nn.Parameter(torch.from_numpy(p0.copy()))
    opt = torch.optim.AdamW([tp], lr=2e-3, foreach=False)
    p, m, v = p0.copy(), np.zeros(n, np.float32), np.zeros(n, np.float32)
    worst = 0.0
    for t in range(1, STEPS + 1):
        lr = 2e-3 * (0.1 + 0.9 * t / STEPS)
        g = (rng.standard_normal(n) * 10.0 ** rng.uniform(-6, -2, n)).astype(np.float32)
        clip = np.float32(1.0 if t % 3 else 0.37)
        for pg in opt.param_groups:
            pg["lr"] = lr
        tp.grad = torch.from_numpy(g * clip)            # clip_grad_norm_ multiplies the gradient in place before the step
        opt.step()
        p, _, m, v = A.step(p, g, m, v, clip, *A.scalars(lr, t))
        ulps = np.abs(p.astype(np.float64) - tp.detach().numpy().astype(np.float64)) / np.spacing(np.abs(tp.detach().numpy()))
        worst = max(worst, float(ulps.max()))
    return worst


def test_restatement_follows_torch_within_a_few_ulps():
    worst = max(_run(seed) for seed in (0, 1, 2))
    print("adamw_ref against torch.optim.AdamW: largest deviation %.2f ulps over %d steps" % (worst, STEPS))
    assert worst <= 4 * MEASURED_ULPS, worst


def test_zero_gradient_only_decays():
    p = np.linspace(-1, 1, 65, dtype=np.float32)
    z = np.zeros_like(p)
    decay, step_size, bc2 = A.scalars(2e-3, 1)
    p1, g1, m1, v1 = A.step(p, z, z, z, 1.0, decay, step_size, bc2)
    assert np.array_equal(p1, p * decay) and not g1.any() and not m1.any() and not v1.any()
