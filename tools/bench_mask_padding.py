#!/usr/bin/env python3
"""What do the key-padding masks - of the ReviewNet (UMPR(mask_padding=True), --mask_padding True) and of the ControlNet
(UMPR(mask_control=True), --mask_control True) - and own GRU states (--unsort_gru True) cost per training step?

For every workload two model / optimiser pairs live in ONE process - the mask off and on - and take turns in blocks of --steps
steps (host clock around a block that ends in a device synchronise), so that both see the same machine; the median block of
--rounds rounds is reported per leg, the spread (min .. max) next to it, and the difference to the off leg, which is the
yardstick.  The on leg adds one umpr_token_mask launch and runs coattn_scores*_masked / coattn_finish_masked / snet_pool_fwd_masked
in place of the unmasked kernels; nothing else differs.  The batch is the ragged synthetic one (sentence counts 5..20, lengths
6..20, padded to the batch maximum: about 60 % of the S x L positions are padding).
Legs: off, on (mask_padding), control (mask_control alone: two umpr_token_mask launches, cnet_head_fwd_masked three times and
snet_pool_fwd_masked once in place of the unmasked kernels; it changes nothing in the UMPR-R workloads, which have no ControlNet),
both; unsort (unsort_gru alone: the same kernels, the GRUs write every sentence's states to its own row), all (the three options).

    python tools/bench_mask_padding.py [--workloads umpr_r,umpr_r_graphed,full_f32] [--legs off,on] [--rounds 7] [--steps 8]
    python tools/bench_mask_padding.py --workloads full_f32 --legs off,control,both,unsort,all

Per-kernel times come from one trace per leg (kernel tracing only, no counters in the same run), e.g.

    rocprofv3 --kernel-trace --stats -d out_on -o on -- python tools/bench_mask_padding.py --workloads umpr_r --legs on --rounds 3
    python tools/bench_mask_padding.py --stats out_on        # the rows of coattn_scores*, coattn_finish*, snet_pool_fwd*, token_mask,
                                                             # cnet_head_fwd* (a trace of legs off,control holds both head kernels)

One JSON line per measurement on stdout."""
import argparse
import csv
import glob
import json
import os
import re
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from umpr_amd.config import Config  # noqa: E402
from umpr_amd.synthetic import make_batch, make_param_state  # noqa: E402

WORKLOADS = {
    "umpr_r": dict(dtype="fp32", emb=50, batch=32, review_net_only=True, graphed=False),
    "umpr_r_graphed": dict(dtype="fp32", emb=50, batch=32, review_net_only=True, graphed=True),
    "full_f32": dict(dtype="fp32", emb=50, batch=64, review_net_only=False, graphed=False),
}
VOCAB = 400003
KERNELS = ("coattn_scores", "coattn_finish", "snet_pool_fwd", "token_mask", "review_collate", "cnet_head_fwd")
LEGS = {"off": (False, False, False), "on": (True, False, False), "control": (False, True, False), "both": (True, True, False),
        "unsort": (False, False, True), "all": (True, True, True)}   # (mask_padding, mask_control, unsort_gru)


def build(w, dev, leg):
    """the step function of one leg"""
    from umpr_amd.graphs import GraphedTrainStep
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    from umpr_amd.train import train_step
    torch.manual_seed(0)
    Config.extend({"dtype": "fp32", "mask_padding": False, "mask_control": False, "unsort_gru": False})
    cfg = Config(argv=[])
    cfg.review_net_only, cfg.dtype, cfg.views = w["review_net_only"], w["dtype"], ["v0"]
    cfg.mask_padding, cfg.mask_control, cfg.unsort_gru = LEGS[leg]
    P = make_param_state(0, w["emb"], VOCAB, 1, w["review_net_only"])
    model = UMPR(cfg, P["embedding.weight"].numpy())
    model.load_state_dict(P)
    model = model.to(dev)
    assert (model.mask_padding, model.mask_control, model.unsort_gru) == LEGS[leg]
    opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay)
    u, i_, ui, ul, il, uil, photos, labels = make_batch(1234, w["batch"], VOCAB, 1, review_net_only=w["review_net_only"])
    batch = (u.to(dev), i_.to(dev), ui.to(dev), ul, il, uil, photos.to(dev), labels.to(dev))
    pad = 1.0 - float((u != 0).float().mean())
    if w["graphed"]:
        g = GraphedTrainStep(model, opt, batch)
        return (lambda: g(batch)), pad, tuple(u.shape)
    return (lambda: train_step(model, opt, batch)), pad, tuple(u.shape)


def stats_rows(directory):
    """the rows of the kernels this change touches from the kernel_stats CSV files below `directory`"""
    rows = []
    for path in sorted(glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)):
        with open(path, newline="") as f:
            for r in csv.DictReader(f):
                name = re.sub(r"^void ", "", r.get("Name", "").replace("(anonymous namespace)::", "")).split("(")[0]
                if any(k in name for k in KERNELS):
                    rows.append({"file": os.path.relpath(path, directory), "kernel": name, "calls": int(r["Calls"]),
                                 "avg_us": round(float(r["AverageNs"]) / 1e3, 2), "min_us": round(float(r["MinNs"]) / 1e3, 2),
                                 "max_us": round(float(r["MaxNs"]) / 1e3, 2), "total_ms": round(float(r["TotalDurationNs"]) / 1e6, 3)})
    return rows


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="umpr_r,umpr_r_graphed,full_f32")
    ap.add_argument("--legs", default="off,on")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--stats", default="", help="print the touched kernels' rows of a rocprofv3 --kernel-trace --stats output directory")
    a = ap.parse_args(argv)
    if a.stats:
        for row in stats_rows(a.stats):
            print(json.dumps(row), flush=True)
        return 0
    names = [n for n in a.workloads.split(",") if n]
    legs = tuple(x for x in a.legs.split(",") if x)
    for n in names:
        if n not in WORKLOADS:
            ap.error(f"unknown workload {n!r} (known: {', '.join(WORKLOADS)})")
    if not legs or any(x not in LEGS for x in legs):
        ap.error("--legs takes a comma-separated choice of " + ", ".join(LEGS))
    if not torch.cuda.is_available():
        sys.exit("bench_mask_padding.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    for name in names:
        w = WORKLOADS[name]
        sides = {leg: build(w, dev, leg) for leg in legs}
        for step, _, _ in sides.values():
            for _ in range(a.warmup):
                step()
        torch.cuda.synchronize()
        ms = {leg: [] for leg in legs}
        for r in range(a.rounds):
            for leg in (legs if r % 2 == 0 else legs[::-1]):
                step = sides[leg][0]
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                ms[leg].append(1e3 * (time.perf_counter() - t0) / a.steps)
        for leg in legs:
            med = statistics.median(ms[leg])
            line = {"workload": name, **w, "leg": leg, "mask_padding": "on" if LEGS[leg][0] else "off",
                    "mask_control": "on" if LEGS[leg][1] else "off", "unsort_gru": "on" if LEGS[leg][2] else "off", "shape_B_S_L": sides[leg][2], "padding_share": round(sides[leg][1], 3),
                    "steps_per_block": a.steps, "rounds": a.rounds, "ms_per_step": round(med, 4),
                    "min_max": [round(min(ms[leg]), 4), round(max(ms[leg]), 4)], "samples_per_s": round(w["batch"] / (med * 1e-3), 1)}
            if "off" in ms:
                line["diff_ms_to_off"] = round(med - statistics.median(ms["off"]), 4)
                line["off_spread_ms"] = round(max(ms["off"]) - min(ms["off"]), 4)
            print(json.dumps(line), flush=True)
        del sides
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
