#!/usr/bin/env python3
"""What do per-module learning rates, decoupled decay and warm-up (FusedAdam(lr_scales=, wd_scales=, decoupled_decay=, warmup_steps=))
cost per step, and how fast is the segmented Adam kernel?

For every workload two model / optimiser pairs live in ONE process - the options off and on - and take turns in blocks of --steps
steps (host clock around a block that ends in a device synchronise), so that both see the same machine; the median block of
--rounds rounds is reported per leg, the spread (min .. max) next to it, and the difference to the leg with the options off.  The
leg with them scales the learning rate and the decay of one module (the VGG; the R-Net in UMPR-R), decays decoupled and warms up
over 16 steps: every dense Adam launch is then umpr_adam_step_groups.

Behind the first workload the kernel is timed alone with device events on buffers of that workload's weight arena, in turns inside
one process: umpr_adam_step (the plain form), umpr_adam_step_groups with 4 and with 16 segments under coupled decay, and with 4
segments under decoupled decay - 28 bytes per element each (p, g, m, v read, p, m, v written) - with their achieved bandwidth.

    python tools/bench_param_groups.py [--workloads full_f32,full_bf16,umpr_r] [--rounds 7] [--steps 8] [--warmup 4]

One JSON line per measurement on stdout."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from umpr_amd._lib import lib, stream_ptr  # noqa: E402
from umpr_amd.config import Config  # noqa: E402
from umpr_amd.model import UMPR  # noqa: E402
from umpr_amd.optim import FusedAdam  # noqa: E402
from umpr_amd.synthetic import make_batch, make_param_state  # noqa: E402
from umpr_amd.train import train_step  # noqa: E402

# bench.py's workloads (BASELINE.json configs[1], configs[4] per GPU, configs[0])
WORKLOADS = {
    "full_f32": dict(dtype="fp32", emb=50, batch=64, review_net_only=False),
    "full_bf16": dict(dtype="bf16", emb=300, batch=64, review_net_only=False),
    "umpr_r": dict(dtype="fp32", emb=50, batch=32, review_net_only=True),
}
VOCAB = 400003
LEGS = ("off", "on")


def options(w):
    prefix = "review_net.r_net." if w["review_net_only"] else "visual_net.vgg16."
    return dict(lr_scales={prefix: 0.25}, wd_scales={prefix: 4.0}, decoupled_decay=True, warmup_steps=16)


def build(w, dev, leg):
    """(optimiser, step function) of one leg"""
    torch.manual_seed(0)
    Config.extend({"dtype": "fp32"})
    cfg = Config(argv=[])
    cfg.review_net_only, cfg.dtype, cfg.views = w["review_net_only"], w["dtype"], ["v0"]
    P = make_param_state(0, w["emb"], VOCAB, 1, w["review_net_only"])
    model = UMPR(cfg, P["embedding.weight"].numpy())
    model.load_state_dict(P)
    model = model.to(dev)
    opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay, **(options(w) if leg == "on" else {}))
    u, i_, ui, ul, il, uil, photos, labels = make_batch(1234, w["batch"], VOCAB, 1, review_net_only=w["review_net_only"],
                                                        full_pad=True)
    batch = (u.to(dev), i_.to(dev), ui.to(dev), ul, il, uil, photos.to(dev), labels.to(dev))
    return opt, lambda: train_step(model, opt, batch)


def time_kernels(opt, reps=20, rounds=7):
    """Device-event time of the plain and the segmented launches over buffers of this optimiser's weight arena, in turns.  The
    training state is left alone."""
    L = lib()
    n = opt.groups[0].numel
    p, g, m = (torch.randn(n, device=opt.groups[0].p.device) * s for s in (1.0, 0.1, 0.01))
    v = torch.rand(n, device=p.device) * 1e-3
    scalars = (1e-6, 0.9, 0.999, 1e-8, 1e-3, 1, 1.0)

    def table(k):
        ends = [n * (j + 1) // k // 64 * 64 for j in range(k - 1)] + [n]
        return ((ctypes.c_long * k)(*ends), (ctypes.c_float * k)(*[0.25 + 0.5 * (j % 4) for j in range(k)]),
                (ctypes.c_float * k)(*[4.0 - (j % 4) for j in range(k)]), k)

    def groups(tab, decoupled):
        e, a, w, k = tab
        return lambda: L.call("umpr_adam_step_groups", p, g, m, v, n, *scalars, None, None, ctypes.addressof(e), ctypes.addressof(a),
                              ctypes.addressof(w), k, decoupled, stream_ptr())

    t4, t16 = table(4), table(16)
    legs = (("plain", lambda: L.call("umpr_adam_step", p, g, m, v, n, *scalars, stream_ptr())),
            ("segments_4", groups(t4, 0)), ("segments_16", groups(t16, 0)), ("segments_4_decoupled", groups(t4, 1)))
    for _, fn in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _ in legs}
    for r in range(rounds):
        for name, fn in (legs if r % 2 == 0 else legs[::-1]):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps)
    out = []
    for name, _ in legs:
        t = statistics.median(ms[name])
        out.append({"kernel": name, "elements": n, "bytes": 28 * n, "ms": round(t, 5),
                    "ms_min_max": [round(min(ms[name]), 5), round(max(ms[name]), 5)], "TB_per_s": round(28 * n / (t * 1e-3) / 1e12, 3),
                    "ms_over_plain": round(t - statistics.median(ms["plain"]), 5)})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="full_f32,full_bf16,umpr_r")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args(argv)
    names = [n for n in a.workloads.split(",") if n]
    for n in names:
        if n not in WORKLOADS:
            ap.error(f"unknown workload {n!r} (known: {', '.join(WORKLOADS)})")
    if not torch.cuda.is_available():
        sys.exit("bench_param_groups.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    kernels_done = False
    for name in names:
        w = WORKLOADS[name]
        sides = {leg: build(w, dev, leg) for leg in LEGS}
        for _, step in sides.values():
            for _ in range(a.warmup):
                step()
        torch.cuda.synchronize()
        ms = {leg: [] for leg in LEGS}
        for r in range(a.rounds):
            for leg in (LEGS if r % 2 == 0 else LEGS[::-1]):
                step = sides[leg][1]
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                ms[leg].append(1e3 * (time.perf_counter() - t0) / a.steps)
        for leg in LEGS:
            med = statistics.median(ms[leg])
            opt = sides[leg][0]
            assert opt.step_count == a.warmup + a.rounds * a.steps
            print(json.dumps({"workload": name, **w, "options": leg,
                              "segments": [sum(len(s) for _, _, s in opt.plan(gi, 0, g.numel)) for gi, g in enumerate(opt.groups)],
                              "steps_per_block": a.steps, "rounds": a.rounds, "ms_per_step": round(med, 4),
                              "min_max": [round(min(ms[leg]), 4), round(max(ms[leg]), 4)],
                              "samples_per_s": round(w["batch"] / (med * 1e-3), 1),
                              "diff_ms_to_off": round(med - statistics.median(ms["off"]), 4)}), flush=True)
        if not kernels_done:
            for line in time_kernels(sides["off"][0]):
                print(json.dumps({"arena_of": name, **line}), flush=True)
            kernels_done = True
        del sides
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
