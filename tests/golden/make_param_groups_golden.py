#!/usr/bin/env python3
"""Writes tests/golden/param_groups_umpr_r.npz: four UMPR-R training steps of the oracle (oracle/umpr_ref.py, torch CPU, fp32) with
ONE torch param group per parameter - its own lr = LR * warm-up * a and weight_decay = l2 * w (0 for a bias) - what
FusedAdam(lr_scales=, wd_scales=, decoupled_decay=, warmup_steps=) has to reproduce on the GPU (tests/test_gpu_param_groups.py).
Two legs, both with lr_scale review_net.r_net.=0.25,review_net.=0.5 (longest prefix wins), wd_scale linear_fusion.=0,
review_net.s_net_u.=4 and a warm-up of 3 steps:

    coupled     torch.optim.Adam,  lr 1e-3, l2 1e-3
    decoupled   torch.optim.AdamW, lr 1e-3, l2 1.0   (at l2 1e-3 AdamW's decay moves a parameter by 1e-6 of itself per step: a run
                                                      without it would stay inside the tolerance)

    <leg>/param/<name>          parameters after the fourth step; the decoupled leg's are stored as decoupled/param_xor_coupled/<name>,
                                their float32 bit patterns XORed with the coupled leg's (uint32): the file stays below the
                                repository's 1 MiB limit for a committed file, and nothing is lost
    <leg>/mask/<name>           np.packbits of the elements whose oracle gradient was above 1e-4 of the tensor's maximum in EVERY
                                step (below that Adam's sign-like steps move an element by +-lr on rounding noise)
    <leg>/separation/<variant>  max over those elements of all parameters of |variant - leg| / (2e-5 + 1e-4 |leg|) for the leg's own
                                wrong variants - no lr scale, no wd scale, the other decay mode, no warm-up, no decay, shortest
                                instead of longest prefix: how far a run with that mistake lands outside the test's tolerance.
                                Every one is asserted to be above 10 here.

About two minutes on a CPU.
"""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
from oracle import umpr_ref as R  # noqa: E402
from umpr_amd.synthetic import make_batch, make_param_state  # noqa: E402

LR, STEPS, WARMUP = 1e-3, 4, 3
LR_SCALE = {"review_net.r_net.": 0.25, "review_net.": 0.5}
WD_SCALE = {"linear_fusion.": 0.0, "review_net.s_net_u.": 4.0}
LEGS = {"coupled": (False, 1e-3), "decoupled": (True, 1.0)}


def pick(name, scales, longest=True):
    hits = [p for p in scales if name.startswith(p)]
    if not hits:
        return 1.0
    return scales[max(hits, key=len) if longest else min(hits, key=len)]


def run(decoupled, l2, lr_scale=LR_SCALE, wd_scale=WD_SCALE, warmup=WARMUP, longest=True):
    P = make_param_state(31, 50, 1000, 1, True, m_scale=0.05)
    for k, p in P.items():
        if k != "embedding.weight":
            p.requires_grad_(True)
    train = {k: p for k, p in P.items() if p.requires_grad}
    a = {k: pick(k, lr_scale, longest) for k in train}
    groups = [{"params": [p], "lr": LR * a[k], "weight_decay": 0.0 if "bias" in k else l2 * pick(k, wd_scale, longest)}
              for k, p in train.items()]
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(groups, lr=LR)
    mask = None
    for s in range(STEPS):
        batch = make_batch(500 + s, 4, 1000, review_net_only=True)
        _, loss = R.umpr_forward(P, batch, review_net_only=True, aten=True, train=True)
        opt.zero_grad()
        loss.backward()
        big = {k: p.grad.abs() > 1e-4 * p.grad.abs().max() for k, p in train.items()}
        mask = big if mask is None else {k: mask[k] & big[k] for k in big}
        f = min(1.0, (s + 1) / warmup) if warmup > 0 else 1.0
        for grp, k in zip(opt.param_groups, train):
            grp["lr"] = LR * f * a[k]
        opt.step()
    return {k: p.detach().clone() for k, p in train.items()}, mask


def main():
    torch.manual_seed(0)
    out = {"lr": np.float64(LR), "warmup_steps": np.int64(WARMUP),
           "lr_scale": np.array(",".join(f"{k}={v:g}" for k, v in LR_SCALE.items())),
           "wd_scale": np.array(",".join(f"{k}={v:g}" for k, v in WD_SCALE.items()))}
    for leg, (decoupled, l2) in LEGS.items():
        ref, mask = run(decoupled, l2)
        out[f"{leg}/l2"] = np.float64(l2)
        for k in ref:
            assert mask[k].any(), k
            bits = ref[k].numpy().view(np.uint32)
            if leg == "coupled":
                out[f"{leg}/param/{k}"] = ref[k].numpy()
            else:       # lossless, and half the bytes once compressed: the two legs share sign, exponent and leading digits
                out[f"{leg}/param_xor_coupled/{k}"] = bits ^ out[f"coupled/param/{k}"].view(np.uint32)
            out[f"{leg}/mask/{k}"] = np.packbits(mask[k].numpy().reshape(-1))
        variants = {"no_lr_scale": dict(lr_scale={}), "no_wd_scale": dict(wd_scale={}), "other_decay_mode": dict(flip=True),
                    "no_warmup": dict(warmup=0), "no_decay": dict(l2=0.0), "shortest_prefix": dict(longest=False)}
        for name, kw in variants.items():
            got, _ = run(decoupled != kw.pop("flip", False), kw.pop("l2", l2), **kw)
            sep = max(float(((got[k] - ref[k]).abs() / (2e-5 + 1e-4 * ref[k].abs()))[mask[k]].max()) for k in ref)
            print(f"{leg}: {name}: {sep:.1f} x the tolerance")
            assert sep > 10, (leg, name, sep)
            out[f"{leg}/separation/{name}"] = np.float64(sep)
    path = os.path.join(ROOT, "tests", "golden", "param_groups_umpr_r.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
