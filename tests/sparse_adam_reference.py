"""Float64 NumPy statement of the sparse table update (`--sparse_embedding True`; test helper, not a test module; CPU only).

torch.optim.SparseAdam(lr, betas=(b1, b2), eps) on an nn.Embedding(sparse=True): for the rows R a step names, with g the row's
summed token gradient (times grad_scale),
    m = b1 m + (1 - b1) g
    v = b2 v + (1 - b2) g g
    p -= lr * sqrt(1 - b2^t) / (1 - b1^t) * m / (sqrt(v) + eps)        (eps next to sqrt(v) itself - not dense Adam's form)
with t the optimiser's global step count; a row outside R keeps p, m and v.  No weight decay.
`dtype=np.float32` evaluates the same formula in float32 - the yardstick of the gate (coattn_decisions.gate).
tests/test_sparse_adam_reference.py checks the float64 form against torch.optim.SparseAdam itself.
"""
import numpy as np


def row_update(p, m, v, rows, grad, step, lr, beta1=0.9, beta2=0.999, eps=1e-8, grad_scale=1.0, dtype=np.float64):
    """p, m, v [vocab][E]; rows: the distinct ids of R; grad [len(rows)][E].  Returns new (p, m, v) in `dtype`; the inputs stay as
    they are.  The scalars are formed in float64 and rounded once to `dtype`, as a kernel's launcher forms them."""
    p, m, v = (np.array(a, dtype=dtype) for a in (p, m, v))
    rows = np.asarray(rows, dtype=np.int64).reshape(-1)
    assert np.unique(rows).size == rows.size, "the ids of a step's index set are distinct"
    f = dtype
    b1, b2, e = f(beta1), f(beta2), f(eps)
    step_size = f(lr * np.sqrt(1.0 - beta2 ** step) / (1.0 - beta1 ** step))
    g = np.asarray(grad, dtype=dtype).reshape(rows.size, -1) * f(grad_scale)
    mr = b1 * m[rows] + (f(1) - b1) * g
    vr = b2 * v[rows] + (f(1) - b2) * g * g
    m[rows], v[rows] = mr, vr
    p[rows] = p[rows] - step_size * (mr / (np.sqrt(vr) + e))
    return p, m, v


def named_rows(ids_list, vocab):
    """the step's index set R, ascending: every id in [0, vocab) any token of any source names"""
    flat = np.concatenate([np.asarray(i, dtype=np.int64).reshape(-1) for i in ids_list]) if ids_list else np.zeros(0, np.int64)
    return np.unique(flat[(flat >= 0) & (flat < vocab)])
