#!/usr/bin/env python3
"""What does gradient accumulation (train_step(update=False), --accum_steps k) cost per micro-batch?

For every workload three model / optimiser pairs live in ONE process - k = 1 (a step per batch), k = 2 and k = 4 - and take
turns in blocks of --steps micro-batches (host clock around a block that ends in a device synchronise; --steps is a multiple of
4, so every block ends on an optimiser step), so that all see the same machine; the median block of --rounds rounds is reported
per leg, and the spread (min .. max) next to it.  Per micro-batch a leg with k > 1 adds one pass of umpr_grad_accumulate over the
gradient arenas (8 bytes per element for the first micro-batch of a group, 12 for the others) and takes 1 / k of an Adam pass
(28 bytes per element); it also gives up the early update of the classifier slice.  The captured UMPR-R step (umpr_r_graph) takes
single-batch steps only: it runs the k = 1 leg.

Behind the first workload the kernels are timed alone with device events on that workload's arenas, in turns inside one process:
umpr_grad_accumulate over every gradient arena with first = 1 and first = 0, and umpr_adam_step over the same arenas (on copies
of p, m and v), with their achieved bandwidth and accumulate's share of Adam's.

    python tools/bench_accum.py [--workloads full_f32,full_bf16,umpr_r,umpr_r_graph] [--rounds 7] [--steps 8] [--warmup 4]

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

# bench.py's workloads: BASELINE.json configs[1], configs[4] per GPU, configs[0] eager and as a graph
WORKLOADS = {
    "full_f32": dict(dtype="fp32", emb=50, batch=64, review_net_only=False, graph=False),
    "full_bf16": dict(dtype="bf16", emb=300, batch=64, review_net_only=False, graph=False),
    "umpr_r": dict(dtype="fp32", emb=50, batch=32, review_net_only=True, graph=False),
    "umpr_r_graph": dict(dtype="fp32", emb=50, batch=32, review_net_only=True, graph=True),
}
VOCAB = 400003
LEGS = (1, 2, 4)


def build(w, dev, k):
    """(optimiser, micro-batch function) of one leg: the function runs one micro-batch, the k-th of each group with its step"""
    torch.manual_seed(0)
    Config.extend({"dtype": "fp32"})
    cfg = Config(argv=[])
    cfg.review_net_only = w["review_net_only"]
    cfg.views = ["v0"]
    cfg.dtype = w["dtype"]
    P = make_param_state(0, w["emb"], VOCAB, 1, w["review_net_only"])
    model = UMPR(cfg, P["embedding.weight"].numpy())
    model.load_state_dict(P)
    model = model.to(dev)
    opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay)
    u, i_, ui, ul, il, uil, photos, labels = make_batch(1234, w["batch"], VOCAB, 1, review_net_only=w["review_net_only"],
                                                        full_pad=True)
    batch = (u.to(dev), i_.to(dev), ui.to(dev), ul, il, uil, photos.to(dev), labels.to(dev))
    if w["graph"]:
        assert k == 1
        from umpr_amd.graphs import GraphedTrainStep
        graphed = GraphedTrainStep(model, opt, batch)
        batch = graphed.resident(batch)
        return opt, lambda: graphed(batch)
    count = [0]

    def micro():
        count[0] += 1
        train_step(model, opt, batch, update=count[0] % k == 0)
    return opt, micro


def time_kernels(opt, reps=20, rounds=5):
    """Device-event time of umpr_grad_accumulate (first = 1, first = 0) and umpr_adam_step over this optimiser's arenas, in turns"""
    L = lib()
    groups = [g for g in opt.groups if g.numel]
    n_all = sum(g.numel for g in groups)
    acc = [torch.empty_like(g.g) for g in groups]
    table = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    pa, pg, cn = table(acc), table([g.g for g in groups]), (ctypes.c_long * len(groups))(*[g.numel for g in groups])
    pmv = [(g.p.clone(), g.m.clone(), g.v.clone()) for g in groups]        # the training state is left alone

    def accumulate(first):
        L.call("umpr_grad_accumulate", ctypes.addressof(pa), ctypes.addressof(pg), ctypes.addressof(cn), len(groups), first,
               stream_ptr())

    def adam():
        for g, (p, m, v) in zip(groups, pmv):
            L.call("umpr_adam_step", p, g.g, m, v, g.numel, 1e-6, 0.9, 0.999, 1e-8, g.weight_decay, 1, 1.0, stream_ptr())

    legs = (("grad_accumulate_first", lambda: accumulate(1), 8 * n_all), ("grad_accumulate_add", lambda: accumulate(0), 12 * n_all),
            ("adam_step", adam, 28 * n_all))
    for _, fn, _ in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in legs}
    for r in range(rounds):
        for name, fn, _ in (legs if r % 2 == 0 else legs[::-1]):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms[name].append(a.elapsed_time(b) / reps)
    out, rate = [], {}
    for name, _, nbytes in legs:
        t = statistics.median(ms[name])
        rate[name] = nbytes / (t * 1e-3) / 1e12
        out.append({"kernel": name, "elements": n_all, "bytes": nbytes, "ms": round(t, 5),
                    "ms_min_max": [round(min(ms[name]), 5), round(max(ms[name]), 5)], "TB_per_s": round(rate[name], 3)})
    for name in ("grad_accumulate_first", "grad_accumulate_add"):
        out.append({"kernel": name, "share_of_adam_step_rate": round(rate[name] / rate["adam_step"], 3)})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="full_f32,full_bf16,umpr_r,umpr_r_graph")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args(argv)
    names = [n for n in a.workloads.split(",") if n]
    for n in names:
        if n not in WORKLOADS:
            ap.error(f"unknown workload {n!r} (known: {', '.join(WORKLOADS)})")
    if a.steps % max(LEGS) or a.warmup % max(LEGS):
        ap.error(f"--steps and --warmup must be multiples of {max(LEGS)}: every block ends on an optimiser step of every leg")
    if not torch.cuda.is_available():
        sys.exit("bench_accum.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    kernels_done = False
    for name in names:
        w = WORKLOADS[name]
        legs = (1,) if w["graph"] else LEGS
        sides = {k: build(w, dev, k) for k in legs}
        for _, micro in sides.values():
            for _ in range(a.warmup):
                micro()
        torch.cuda.synchronize()
        ms = {k: [] for k in legs}
        for r in range(a.rounds):
            for k in (legs if r % 2 == 0 else legs[::-1]):
                micro = sides[k][1]
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    micro()
                torch.cuda.synchronize()
                ms[k].append(1e3 * (time.perf_counter() - t0) / a.steps)
        for k in legs:
            med = statistics.median(ms[k])
            opt = sides[k][0]
            assert opt.pending == 0 and opt.step_count * k >= a.rounds * a.steps
            print(json.dumps({"workload": name, **w, "accum_steps": k, "micro_batches_per_block": a.steps, "rounds": a.rounds,
                              "ms_per_micro_batch": round(med, 4), "min_max": [round(min(ms[k]), 4), round(max(ms[k]), 4)],
                              "samples_per_s": round(w["batch"] / (med * 1e-3), 1),
                              "diff_ms_to_k1": round(med - statistics.median(ms[1]), 4)}), flush=True)
        if not kernels_done:
            for line in time_kernels(sides[1][0]):
                print(json.dumps({"arenas_of": name, **line}), flush=True)
            kernels_done = True
        del sides
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
