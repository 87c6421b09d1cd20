#!/usr/bin/env python3
"""What does the moving average of the weights (FusedAdam(ema_decay=), --ema_decay) cost per step, and how fast are its kernels?

For every workload two model / optimiser pairs live in ONE process - the average off and on (decay 0.999) - and take turns in
blocks of --steps steps (host clock around a block that ends in a device synchronise), so that both see the same machine; the
median block of --rounds rounds is reported per leg, the spread (min .. max) next to it, and the difference to the leg without
the average.  The leg with it adds one umpr_ema_update over the parameter arenas behind every step (12 bytes per element).

Behind the first workload the kernels are timed alone with device events on that workload's arenas, in turns inside one process:
umpr_ema_update with first = 0 (12 B/element) and first = 1 (8 B/element), umpr_arena_swap (16 B/element) and, as the yardstick,
umpr_grad_accumulate in its add form over the same arenas (12 B/element, two reads and one write like the update), with their
achieved bandwidth, the update's rate as a share of the yardstick's, and what a validation pass pays for its two swaps.

The freeze_conv workload trains on a warm pool5 store: a small corpus is written to a temporary directory, each leg gets its own
store (a store belongs to one set of conv weights) and one batch collated against it, which the warm-up steps make resident.

    python tools/bench_ema.py [--workloads full_f32,full_bf16,freeze_conv,umpr_r] [--rounds 7] [--steps 8] [--warmup 4]

One JSON line per measurement on stdout."""
import argparse
import ctypes
import json
import os
import statistics
import sys
import tempfile
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from umpr_amd._lib import lib, stream_ptr  # noqa: E402
from umpr_amd.config import Config  # noqa: E402
from umpr_amd.model import UMPR  # noqa: E402
from umpr_amd.optim import FusedAdam  # noqa: E402
from umpr_amd.synthetic import make_batch, make_param_state  # noqa: E402
from umpr_amd.train import train_step  # noqa: E402

# bench.py's workloads (BASELINE.json configs[1], configs[4] per GPU, configs[0]) and the frozen conv base on its pool5 store
WORKLOADS = {
    "full_f32": dict(dtype="fp32", emb=50, batch=64, review_net_only=False, freeze_conv=False),
    "full_bf16": dict(dtype="bf16", emb=300, batch=64, review_net_only=False, freeze_conv=False),
    "freeze_conv": dict(dtype="fp32", emb=50, batch=64, review_net_only=False, freeze_conv=True),
    "umpr_r": dict(dtype="fp32", emb=50, batch=32, review_net_only=True, freeze_conv=False),
}
VOCAB = 400003
DECAY = 0.999
LEGS = ("off", "on")


def corpus(directory, batch):
    """A Dataset of at least `batch` samples with photos on disk (tools/bench_loader.py's corpus), and its word vectors"""
    from bench_loader import write_corpus
    from umpr_amd.data import Dataset, Word2vec
    write_corpus(directory, 40, 80)
    cfg = Config(argv=[])
    cfg.views = ["food"]
    w2v = Word2vec(os.path.join(directory, "glove.txt"))
    ds = Dataset(os.path.join(directory, "train.csv"), os.path.join(directory, "photos.json"), os.path.join(directory, "photos"),
                 w2v, cfg)
    assert len(ds) >= batch
    return ds, w2v


def build(w, dev, leg, data=None):
    """(optimiser, step function) of one leg"""
    torch.manual_seed(0)
    Config.extend({"dtype": "fp32", "freeze_conv": False})
    cfg = Config(argv=[])
    cfg.review_net_only, cfg.dtype, cfg.freeze_conv = w["review_net_only"], w["dtype"], w["freeze_conv"]
    kw = {"ema_decay": DECAY} if leg == "on" else {}
    if w["freeze_conv"]:
        from main import _Collate
        from umpr_amd.photos import Pool5Store
        ds, w2v = data
        cfg.views = ["food"]
        model = UMPR(cfg, w2v.embedding).to(dev)
        store = Pool5Store(dev, capacity_bytes=int(1e9)).register(ds.photo_paths())
        batch = _Collate(False, store=store.index)([ds[i] for i in range(w["batch"])])
        opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay, **kw)
        return opt, lambda: train_step(model, opt, batch), store
    cfg.views = ["v0"]
    P = make_param_state(0, w["emb"], VOCAB, 1, w["review_net_only"])
    model = UMPR(cfg, P["embedding.weight"].numpy())
    model.load_state_dict(P)
    model = model.to(dev)
    opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay, **kw)
    u, i_, ui, ul, il, uil, photos, labels = make_batch(1234, w["batch"], VOCAB, 1, review_net_only=w["review_net_only"],
                                                        full_pad=True)
    batch = (u.to(dev), i_.to(dev), ui.to(dev), ul, il, uil, photos.to(dev), labels.to(dev))
    return opt, lambda: train_step(model, opt, batch), None


def time_kernels(opt, reps=20, rounds=7):
    """Device-event time of umpr_ema_update (first = 0, first = 1), umpr_arena_swap and umpr_grad_accumulate (add) over this
    optimiser's arenas, in turns.  The training state is left alone: the kernels run on buffers of their own."""
    L = lib()
    groups = [g for g in opt.groups if g.numel]
    n_all = sum(g.numel for g in groups)
    a = [torch.randn_like(g.p) for g in groups]
    b = [torch.randn_like(g.p) for g in groups]
    table = lambda ts: (ctypes.c_void_p * len(ts))(*[t.data_ptr() for t in ts])
    pa, pb, cn = table(a), table(b), (ctypes.c_long * len(groups))(*[g.numel for g in groups])
    A = ctypes.addressof
    legs = (("ema_update", lambda: L.call("umpr_ema_update", A(pa), A(pb), A(cn), len(groups), DECAY, 0, stream_ptr()), 12 * n_all),
            ("grad_accumulate_add", lambda: L.call("umpr_grad_accumulate", A(pa), A(pb), A(cn), len(groups), 0, stream_ptr()),
             12 * n_all),
            ("ema_update_first", lambda: L.call("umpr_ema_update", A(pa), A(pb), A(cn), len(groups), DECAY, 1, stream_ptr()),
             8 * n_all),
            ("arena_swap", lambda: L.call("umpr_arena_swap", A(pa), A(pb), A(cn), len(groups), stream_ptr()), 16 * n_all))
    for _, fn, _ in legs:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    ms = {name: [] for name, _, _ in legs}
    for r in range(rounds):
        for name, fn, _ in (legs if r % 2 == 0 else legs[::-1]):
            for t in a:
                t.zero_()                              # (the add form would run a up to inf over the repetitions)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(reps):
                fn()
            e1.record()
            e1.synchronize()
            ms[name].append(e0.elapsed_time(e1) / reps)
    out, rate = [], {}
    for name, _, nbytes in legs:
        t = statistics.median(ms[name])
        rate[name] = nbytes / (t * 1e-3) / 1e12
        out.append({"kernel": name, "elements": n_all, "bytes": nbytes, "ms": round(t, 5),
                    "ms_min_max": [round(min(ms[name]), 5), round(max(ms[name]), 5)], "TB_per_s": round(rate[name], 3)})
    share = rate["ema_update"] / rate["grad_accumulate_add"]
    out.append({"kernel": "ema_update", "share_of_grad_accumulate_add_rate": round(share, 3), "at_least_0.9": share >= 0.9})
    out.append({"two_swaps_per_validation_pass_ms": round(2 * statistics.median(ms["arena_swap"]), 5)})
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="full_f32,full_bf16,freeze_conv,umpr_r")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=4)
    a = ap.parse_args(argv)
    names = [n for n in a.workloads.split(",") if n]
    for n in names:
        if n not in WORKLOADS:
            ap.error(f"unknown workload {n!r} (known: {', '.join(WORKLOADS)})")
    if not torch.cuda.is_available():
        sys.exit("bench_ema.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    kernels_done = False
    with tempfile.TemporaryDirectory() as tmp:
        data = corpus(tmp, WORKLOADS["freeze_conv"]["batch"]) if "freeze_conv" in names else None
        for name in names:
            w = WORKLOADS[name]
            sides = {leg: build(w, dev, leg, data) for leg in LEGS}
            for _, step, _ in sides.values():
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
                opt, _, store = sides[leg]
                assert opt.ema_ready == (leg == "on") and opt.step_count == a.warmup + a.rounds * a.steps
                line = {"workload": name, **w, "ema": leg, "ema_decay": opt.ema_decay, "ema_MB": round(opt.ema_bytes() / 1e6, 1),
                        "steps_per_block": a.steps, "rounds": a.rounds, "ms_per_step": round(med, 4),
                        "min_max": [round(min(ms[leg]), 4), round(max(ms[leg]), 4)],
                        "samples_per_s": round(w["batch"] / (med * 1e-3), 1),
                        "diff_ms_to_off": round(med - statistics.median(ms["off"]), 4)}
                if store is not None:
                    line["pool5_store"] = str(store.stats())
                print(json.dumps(line), flush=True)
            if not kernels_done:
                for line in time_kernels(sides["on"][0]):
                    print(json.dumps({"arenas_of": name, **line}), flush=True)
                kernels_done = True
            del sides
            torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
