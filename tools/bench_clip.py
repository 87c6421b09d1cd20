#!/usr/bin/env python3
"""What does gradient clipping (FusedAdam(max_grad_norm=)) cost per training step?

For every workload two model / optimiser pairs live in ONE process, clipping off and on, and take turns in blocks of --steps
steps (host clock around a block that ends in a device synchronise), so that both see the same machine; the median block of
--rounds rounds is reported per side, and the spread (min .. max) next to it.  Before that the two kernels are timed alone with
device events on the first workload's arenas: the norm pass (both launches of umpr_grad_norm over every gradient arena; it reads
4 bytes per element) and the Adam kernel on the weight arena (reads p, g, m, v and writes p, m, v: 28 bytes per element), with
their achieved bandwidth.

    python tools/bench_clip.py [--workloads full_f32,full_bf16,umpr_r,umpr_r_graph] [--rounds 7] [--steps 10] [--warmup 3]

One JSON line per measurement on stdout.  With clipping on the early update of the classifier slice is off as well
(umpr_amd/optim.py::arm_early): the whole-step difference is the sum of both effects."""
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


def build(w, dev, max_grad_norm):
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
    opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay, max_grad_norm=max_grad_norm)
    u, i_, ui, ul, il, uil, photos, labels = make_batch(1234, w["batch"], VOCAB, 1, review_net_only=w["review_net_only"],
                                                        full_pad=True)
    batch = (u.to(dev), i_.to(dev), ui.to(dev), ul, il, uil, photos.to(dev), labels.to(dev))
    if w["graph"]:
        from umpr_amd.graphs import GraphedTrainStep
        graphed = GraphedTrainStep(model, opt, batch)
        batch = graphed.resident(batch)
        return opt, lambda: graphed(batch)
    return opt, lambda: train_step(model, opt, batch)


def time_kernels(opt, reps=20):
    """Device-event time of the norm pass and of the Adam kernel (plain and with the coefficient) on this optimiser's arenas."""
    L = lib()
    c = opt._clip_buffers()
    g = opt.groups[0]
    n_all = sum(a.numel() for a in opt.grad_arenas())

    def norm():
        L.call("umpr_grad_norm", ctypes.addressof(c.ptrs), ctypes.addressof(c.counts), c.n_arenas, 1e30, 1.0, None, c.ws,
               c.ws_bytes, c.state, stream_ptr())

    def adam_clip():      # on copies of p, m, v: the training state is left alone
        L.call("umpr_adam_step_clip", p, g.g, m, v, g.numel, 1e-6, 0.9, 0.999, 1e-8, 1e-3, 1, 1.0, c.state, stream_ptr())

    def adam_plain():
        L.call("umpr_adam_step", p, g.g, m, v, g.numel, 1e-6, 0.9, 0.999, 1e-8, 1e-3, 1, 1.0, stream_ptr())

    p, m, v = g.p.clone(), g.m.clone(), g.v.clone()
    out = []
    for name, fn, nbytes in (("grad_norm", norm, 4 * n_all), ("adam_step", adam_plain, 28 * g.numel),
                             ("adam_step_clip", adam_clip, 28 * g.numel)):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(5):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(reps):
                fn()
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b) / reps)
        t = statistics.median(ms)
        out.append({"kernel": name, "elements": n_all if name == "grad_norm" else g.numel, "bytes": nbytes, "ms": round(t, 5),
                    "ms_min_max": [round(min(ms), 5), round(max(ms), 5)], "TB_per_s": round(nbytes / (t * 1e-3) / 1e12, 3)})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="full_f32,full_bf16,umpr_r,umpr_r_graph")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--max_grad_norm", type=float, default=1.0)
    a = ap.parse_args(argv)
    names = [n for n in a.workloads.split(",") if n]
    for n in names:
        if n not in WORKLOADS:
            ap.error(f"unknown workload {n!r} (known: {', '.join(WORKLOADS)})")
    if not torch.cuda.is_available():
        sys.exit("bench_clip.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    kernels_done = False
    for name in names:
        w = WORKLOADS[name]
        sides = {"off": build(w, dev, 0.0), "on": build(w, dev, a.max_grad_norm)}
        for _, step in sides.values():
            for _ in range(a.warmup):
                step()
        torch.cuda.synchronize()
        ms = {"off": [], "on": []}
        for r in range(a.rounds):
            for side in (("off", "on") if r % 2 == 0 else ("on", "off")):
                step = sides[side][1]
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                ms[side].append(1e3 * (time.perf_counter() - t0) / a.steps)
        off, on = statistics.median(ms["off"]), statistics.median(ms["on"])
        stats = sides["on"][0].clip_stats()
        print(json.dumps({"workload": name, **w, "steps_per_block": a.steps, "rounds": a.rounds,
                          "ms_per_step_off": round(off, 4), "ms_per_step_on": round(on, 4), "diff_ms": round(on - off, 4),
                          "off_min_max": [round(min(ms["off"]), 4), round(max(ms["off"]), 4)],
                          "on_min_max": [round(min(ms["on"]), 4), round(max(ms["on"]), 4)],
                          "clip_stats": stats}), flush=True)
        if not kernels_done:
            for line in time_kernels(sides["on"][0]):
                print(json.dumps({"arenas_of": name, **line}), flush=True)
            kernels_done = True
        del sides
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
