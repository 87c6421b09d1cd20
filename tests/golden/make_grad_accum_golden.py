#!/usr/bin/env python3
"""Writes tests/golden/grad_accum_umpr_r.npz: four UMPR-R optimiser steps of the oracle (oracle/umpr_ref.py, torch CPU, fp32), each
over TWO micro-batches of different size (4 and 3 samples) in the ordinary torch idiom - (loss / 2).backward() twice,
torch.nn.utils.clip_grad_norm_(max_norm=5.6936), torch.optim.Adam.step() in the reference's grouping - what
FusedAdam(max_grad_norm=5.6936) driven by train_step(update=False) / train_step(update=True) has to reproduce on the GPU
(tests/test_gpu_grad_accum.py).  About a minute on a CPU.

    norms_clipped / norms_unclipped   total norm of the accumulated gradient of every step, with and without clipping (steps 3 and 4 clip)
    param/<name>                      parameters after the fourth step
    mask/<name>                       np.packbits of the elements whose accumulated oracle gradient was above 1e-4 of the tensor's
                                      maximum in EVERY step (below that Adam's sign-like steps move an element by +-lr on rounding noise)
    separation/<mutant>               max over those elements of |mutant - golden| / (2e-5 + 1e-4 |golden|) for four wrong
                                      implementations run by the oracle itself: how far each lands outside the test's tolerance
        sum      the micro-batch gradients summed, not averaged
        last     only the last micro-batch of a group reaches the step
        every    a step after every micro-batch
        noclip   the right gradient, never clipped
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import umpr_ref as R  # noqa: E402
from umpr_amd.synthetic import make_batch, make_param_state  # noqa: E402

MAX_NORM, LR, L2, STEPS, K = 5.6936, 1e-3, 1e-3, 4, 2


def micro_batch(s, j):
    return make_batch(500 + 2 * s + j, 4 if j == 0 else 3, 1000, review_net_only=True)


def run(max_norm, mode="mean"):
    P = make_param_state(31, 50, 1000, 1, True, m_scale=0.05)
    for k, p in P.items():
        if k != "embedding.weight":
            p.requires_grad_(True)
    train = {k: p for k, p in P.items() if p.requires_grad}
    opt = R.adam_reference(P, LR, L2)
    norms, mask = [], None

    def update():
        norms.append(float(torch.nn.utils.clip_grad_norm_(list(train.values()), max_norm)))
        opt.step()

    for s in range(STEPS):
        opt.zero_grad()
        for j in range(K):
            _, loss = R.umpr_forward(P, micro_batch(s, j), review_net_only=True, aten=True, train=True)
            if mode in ("last", "every"):
                opt.zero_grad()
            (loss if mode in ("sum", "last", "every") else loss / K).backward()
            if mode == "every":
                update()
        if mode != "every":
            big = {k: p.grad.abs() > 1e-4 * p.grad.abs().max() for k, p in train.items()}
            mask = big if mask is None else {k: mask[k] & big[k] for k in big}
            update()
    return norms, {k: p.detach().clone() for k, p in train.items()}, mask


def main():
    torch.manual_seed(0)
    n_clip, p_clip, mask = run(MAX_NORM)
    mutants = {"sum": run(MAX_NORM, "sum"), "last": run(MAX_NORM, "last"), "every": run(MAX_NORM, "every"),
               "noclip": run(float("inf"))}
    n_free = mutants["noclip"][0]
    out = {"max_norm": np.float64(MAX_NORM), "lr": np.float64(LR), "l2": np.float64(L2),
           "norms_clipped": np.asarray(n_clip, np.float64), "norms_unclipped": np.asarray(n_free, np.float64)}
    for k in p_clip:
        out["param/" + k] = p_clip[k].numpy()
        out["mask/" + k] = np.packbits(mask[k].numpy().reshape(-1))
    for name, (_, p_mut, _) in mutants.items():
        worst = 0.0
        for k in p_clip:
            d = (p_mut[k] - p_clip[k]).abs() / (2e-5 + 1e-4 * p_clip[k].abs())
            if mask[k].any():
                worst = max(worst, float(d[mask[k]].max()))
        out["separation/" + name] = np.float64(worst)
    path = os.path.join(ROOT, "tests", "golden", "grad_accum_umpr_r.npz")
    np.savez_compressed(path, **out)
    print("norms clipped  ", n_clip)
    print("norms unclipped", n_free)
    print("separation / tolerance:", {k[11:]: round(float(out[k]), 1) for k in out if k.startswith("separation/")})
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
