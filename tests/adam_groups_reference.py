"""Restatement of FusedAdam's update with per-parameter multipliers (lr_scales / wd_scales), coupled L2 or AdamW's decoupled decay
and the linear warm-up, on numpy arrays in the precision of choice: float64 is the yardstick of the kernel tests
(tests/test_gpu_param_groups.py), the same statements in float32 are the "float32 CPU evaluation" whose distance from float64
bounds what the kernel may differ by.  tests/test_param_groups_cpu.py holds it against torch.optim.Adam / torch.optim.AdamW with
one param group per parameter, in double.

For an element with multipliers (a, w), at optimiser step t (1-based):
    lr_t = lr * min(1, t / warmup_steps) * a
    coupled:    g' = grad_scale * g + (wd * w) * p;  m, v from g';  p -= lr_t / (1 - b1^t) * m / (sqrt(v) / sqrt(1 - b2^t) + eps)
    decoupled:  p *= 1 - lr_t * wd * w;  m, v from grad_scale * g;  the same p update
"""
import math

import numpy as np


def warmup_factor(step, warmup_steps):
    return min(1.0, step / warmup_steps) if warmup_steps > 0 else 1.0


def adam_groups_step(p, g, m, v, step, lr, wd, a=1.0, w=1.0, decoupled=False, warmup_steps=0, grad_scale=1.0, b1=0.9, b2=0.999,
                     eps=1e-8, dtype=np.float64):
    """One step on arrays of `dtype`; `a` and `w` are scalars or arrays of p's shape.  Returns the new (p, m, v).  Every operation
    of the update's formula as csrc/optim.hip states it ("in floats: ...") is made in `dtype`, the differences 1 - b1 and 1 - b2
    included: in float32 1 - 0.999 is 1.3e-5 away from 0.001, which is part of what a float32 evaluation of that formula is - with
    the two coefficients rounded from double instead, the float32 evaluation sits ten times closer to float64 in v than any
    evaluation of the formula in floats can (measured on the kernel, n = 64: 1.4e-6 of max |v| against 1.5e-7).  The scalars the
    launcher's contract forms in double - the step size, 1 / sqrt(1 - b2^t), the decay products - are formed in double here and
    rounded to `dtype` once, as a torch param group's Python floats are."""
    T = dtype
    p, g, m, v = (np.asarray(x, dtype=T) for x in (p, g, m, v))
    a, w = np.asarray(a, dtype=np.float64), np.asarray(w, dtype=np.float64)
    lr_t = lr * warmup_factor(step, warmup_steps) * a
    step_size = (lr_t / (1.0 - b1 ** step)).astype(T)
    inv_bc2_sqrt = T(1.0 / math.sqrt(1.0 - b2 ** step))
    gi = g * T(grad_scale)
    if decoupled:
        p = p * (1.0 - lr_t * wd * w).astype(T)
    else:
        gi = gi + (wd * w).astype(T) * p
    m = T(b1) * m + (T(1) - T(b1)) * gi
    v = T(b2) * v + (T(1) - T(b2)) * gi * gi
    denom = np.sqrt(v) * inv_bc2_sqrt + T(eps)
    p = p - step_size * (m / denom)
    return p.astype(T), m.astype(T), v.astype(T)
