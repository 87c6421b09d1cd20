#!/usr/bin/env python3
"""What does a trainable embedding table (UMPR(train_embedding=True), `--train_embedding True`) cost per training step?

For every workload three model / optimiser pairs live in ONE process - table frozen ("off"), trainable with the dense update
("on"), trainable with the sparse update (`--sparse_embedding True`, "sparse") - and take turns in blocks of --steps steps (host
clock around a block that ends in a device synchronise), in an order that rotates from round to round, so that all see the same
machine; the median block of --rounds rounds is reported per side, and the spread (min .. max) next to it.  What the dense option
adds to a step: two fp32 GEMMs per GRU backward (the token gradient dx), one id sort, umpr_embed_grad, and vocab * E more elements
in the Adam step.  The sparse one replaces the last two by umpr_embed_grad_rows and umpr_sparse_adam_rows, which touch T * E
elements, and allocates no gradient arena for the table (vocab * E * 4 bytes).  Before the steps umpr_embed_grad,
umpr_embed_grad_rows and umpr_sparse_adam_rows are timed alone with device events on the workload's token ids (random dx).

    python tools/bench_embed_grad.py [--workloads umpr_r,full_f32,full_bf16_e300] [--rounds 7] [--steps 10] [--warmup 3]

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

# UMPR-R at batch 32, the full model in fp32 at batch 64, bf16 with GloVe-300d at batch 64 (BASELINE.json configs[0], [1], [4])
WORKLOADS = {
    "umpr_r": dict(dtype="fp32", emb=50, batch=32, review_net_only=True),
    "full_f32": dict(dtype="fp32", emb=50, batch=64, review_net_only=False),
    "full_bf16_e300": dict(dtype="bf16", emb=300, batch=64, review_net_only=False),
}
VOCAB = 400003


def build(w, dev, train_embedding, sparse_embedding=False):
    torch.manual_seed(0)
    Config.extend({"dtype": "fp32", "train_embedding": False, "sparse_embedding": False})
    cfg = Config(argv=[])
    cfg.review_net_only = w["review_net_only"]
    cfg.views = ["v0"]
    cfg.dtype = w["dtype"]
    cfg.train_embedding = train_embedding
    cfg.sparse_embedding = sparse_embedding
    P = make_param_state(0, w["emb"], VOCAB, 1, w["review_net_only"])
    model = UMPR(cfg, P["embedding.weight"].numpy())
    model.load_state_dict(P)
    model = model.to(dev)
    opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay)
    u, i_, ui, ul, il, uil, photos, labels = make_batch(1234, w["batch"], VOCAB, 1, review_net_only=w["review_net_only"],
                                                        full_pad=True)
    batch = (u.to(dev), i_.to(dev), ui.to(dev), ul, il, uil, photos.to(dev), labels.to(dev))
    return batch, lambda: train_step(model, opt, batch)


def time_scatter(batch, w, dev, reps=20):
    """Device-event time of umpr_embed_grad (its three launches), of umpr_embed_grad_rows and umpr_sparse_adam_rows on the
    workload's token sources, and of the id sort."""
    L = lib()
    E = w["emb"]
    pair = torch.cat([batch[0].reshape(-1), batch[1].reshape(-1)])
    ids = [pair] if w["review_net_only"] else [pair, pair, batch[2].reshape(-1)]
    dx = [torch.randn(i.numel(), E, device=dev) for i in ids]
    T = sum(i.numel() for i in ids)
    d_emb = torch.empty(VOCAB, E, device=dev)
    wsb = L.size("umpr_embed_grad_ws_bytes", T, E)
    ws = torch.empty(wsb // 4 + 64, device=dev)
    iarr = (ctypes.c_void_p * len(ids))(*[t.data_ptr() for t in ids])
    darr = (ctypes.c_void_p * len(ids))(*[t.data_ptr() for t in dx])
    counts = (ctypes.c_long * len(ids))(*[t.numel() for t in ids])
    box = {}

    def sort():
        box["pos"] = torch.sort(torch.cat(ids), stable=True).indices.to(torch.int32)

    def scatter():
        L.call("umpr_embed_grad", ctypes.addressof(iarr), ctypes.addressof(darr), ctypes.addressof(counts), len(ids), E, VOCAB,
               box["pos"], d_emb, ws, wsb, stream_ptr())

    row_id = torch.empty(T, dtype=torch.int64, device=dev)
    row_grad = torch.empty(T, E, device=dev)
    p, m, v = (torch.zeros(VOCAB, E, device=dev) for _ in range(3))
    n_rows = int(torch.unique(torch.cat(ids)).numel())

    def rows():
        L.call("umpr_embed_grad_rows", ctypes.addressof(iarr), ctypes.addressof(darr), ctypes.addressof(counts), len(ids), E, VOCAB,
               box["pos"], row_id, row_grad, ws, wsb, stream_ptr())

    def adam_rows():
        L.call("umpr_sparse_adam_rows", p, m, v, VOCAB, E, row_id, row_grad, T, 1e-6, 0.9, 0.999, 1e-8, 1, 1.0, None, stream_ptr())

    out = []
    for name, fn, nbytes in (("id_sort", sort, 0), ("embed_grad", scatter, 4 * E * (T + VOCAB)),
                             ("embed_grad_rows", rows, 4 * E * 2 * T), ("sparse_adam_rows", adam_rows, 4 * E * (T + 6 * n_rows))):
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
        row = {"kernel": name, "tokens": T, "unique_ids": n_rows, "E": E, "vocab": VOCAB,
               "ms": round(t, 5), "ms_min_max": [round(min(ms), 5), round(max(ms), 5)]}
        if nbytes:
            row.update(bytes=nbytes, TB_per_s=round(nbytes / (t * 1e-3) / 1e12, 3))
        out.append(row)
    return out


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--workloads", default="umpr_r,full_f32,full_bf16_e300")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args(argv)
    names = [n for n in a.workloads.split(",") if n]
    for n in names:
        if n not in WORKLOADS:
            ap.error(f"unknown workload {n!r} (known: {', '.join(WORKLOADS)})")
    if not torch.cuda.is_available():
        sys.exit("bench_embed_grad.py measures on an MI355X: no GPU found")
    dev = torch.device("cuda:0")
    for name in names:
        w = WORKLOADS[name]
        sides = {"off": build(w, dev, False), "on": build(w, dev, True), "sparse": build(w, dev, True, True)}
        for line in time_scatter(sides["on"][0], w, dev):
            print(json.dumps({"sources_of": name, **line}), flush=True)
        for _, step in sides.values():
            for _ in range(a.warmup):
                step()
        torch.cuda.synchronize()
        ms = {"off": [], "on": [], "sparse": []}
        order = list(ms)
        for r in range(a.rounds):
            for side in order[r % 3:] + order[:r % 3]:
                step = sides[side][1]
                t0 = time.perf_counter()
                for _ in range(a.steps):
                    step()
                torch.cuda.synchronize()
                ms[side].append(1e3 * (time.perf_counter() - t0) / a.steps)
        off, on, sp = (statistics.median(ms[k]) for k in order)
        print(json.dumps({"workload": name, **w, "steps_per_block": a.steps, "rounds": a.rounds,
                          "ms_per_step_off": round(off, 4), "ms_per_step_on": round(on, 4), "ms_per_step_sparse": round(sp, 4),
                          "diff_ms": round(on - off, 4), "diff_ms_sparse": round(sp - off, 4),
                          "samples_per_s_off": round(1e3 * w["batch"] / off, 1), "samples_per_s_on": round(1e3 * w["batch"] / on, 1),
                          "samples_per_s_sparse": round(1e3 * w["batch"] / sp, 1),
                          "off_min_max": [round(min(ms["off"]), 4), round(max(ms["off"]), 4)],
                          "on_min_max": [round(min(ms["on"]), 4), round(max(ms["on"]), 4)],
                          "sparse_min_max": [round(min(ms["sparse"]), 4), round(max(ms["sparse"]), 4)],
                          "table_grad_arena_bytes_not_allocated": 4 * VOCAB * w["emb"]}), flush=True)
        del sides
        torch.cuda.empty_cache()
    return 0


if __name__ == "__main__":
    sys.exit(main())
