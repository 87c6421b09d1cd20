#!/usr/bin/env python3
"""The sampled review collate (reviews.ReviewStore.collate(draw=), csrc/reviews.hip::umpr_review_collate_sampled; main.py
--review_pool / --word_dropout) against the plain collate of the same store, in the same process.

1. The call: umpr_review_collate and umpr_review_collate_sampled (without and with word dropout) on preallocated outputs, in
   alternating order, device time per call between two events around a run of calls.  On tools/bench_loader.py's corpus with its
   real pool sizes (Dataset(review_pool=200)) at batch 32 and 64, and on a worst case where every user and item pool holds 1024
   sentences.
2. The host side of a sampled batch alone: ReviewTable.drawn_shape (the numpy draw: shapes and lengths) against the plain
   collate's shape + host_lengths, ms per batch.
3. Whole training epochs, loader + collate + train step with a synchronise at the end, options off and on, interleaved: UMPR-R at
   batch 32 and the frozen conv base on a warm pool5 store at batch 64, fp32.

    python tools/bench_review_sample.py [--items 2000] [--repeats 3] [--workloads umpr_r,freeze_conv] [--calls 2000]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

POOL, DROPOUT = 200, 0.1


def call_times(store, batch, calls, rounds=5):
    """us per call (device time between events, launch-bound calls back to back) of the three entry points on one batch"""
    from umpr_amd._lib import lib
    from umpr_amd.reviews import ReviewDraw
    dev = store.device
    idx = np.random.default_rng(0).integers(0, store.n_samples, size=batch)
    draws = {"sampled": ReviewDraw(1, 0), f"sampled, dropout {DROPOUT}": ReviewDraw(1, 0, DROPOUT, 1)}
    S, L, S_ui, L_ui = store.shape(idx)
    for d in draws.values():                                   # one shape for all three: the largest
        (s, l, _, _), _ = store.drawn_shape(idx, d)
        S, L = max(S, s), max(L, l)
    pair = torch.empty((2, batch, S, L), dtype=torch.int64, device=dev)
    ui = torch.empty((batch, S_ui, L_ui), dtype=torch.int64, device=dev)
    labels = torch.empty(batch, dtype=torch.float32, device=dev)
    host_idx = np.ascontiguousarray(idx, dtype=np.int32)
    p, s = store.d_row_ptr, store.d_sent_id
    tables = (store.d_tokens, store.d_sent_off, store.n_sent, p["user"], s["user"], p["item"], s["item"], p["ui"], s["ui"],
              store.d_ratings, store.n_samples, host_idx.ctypes.data, batch, S, L, S_ui, L_ui, 0)
    outs = (pair, ui, labels, torch.cuda.current_stream(dev).cuda_stream)
    legs = {"plain": lambda: lib().call("umpr_review_collate", *tables, *outs)}
    for name, d in draws.items():
        legs[name] = (lambda d=d: lib().call("umpr_review_collate_sampled", *tables, store.draw_keep(), d.key, d.threshold,
                                             -1 if d.unk is None else d.unk, *outs))
    times = {k: [] for k in legs}
    for f in legs.values():
        f()
    torch.cuda.synchronize()
    for r in range(rounds):
        order = list(legs) if r % 2 == 0 else list(legs)[::-1]
        for k in order:
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(calls):
                legs[k]()
            b.record()
            torch.cuda.synchronize()
            times[k].append(1e3 * a.elapsed_time(b) / calls)
    return (S, L, S_ui, L_ui), {k: statistics.median(v) for k, v in times.items()}


def host_times(store, batch, reps=200):
    """ms per batch of the host half: the plain collate's shape + lengths gather, and the sampled collate's numpy draw"""
    from umpr_amd.reviews import ReviewDraw
    rng = np.random.default_rng(1)
    batches = [rng.integers(0, store.n_samples, size=batch) for _ in range(reps)]
    draw = ReviewDraw(1, 0, DROPOUT, 1)
    t0 = time.perf_counter()
    for idx in batches:
        S, _, S_ui, _ = store.shape(idx)
        store.host_lengths(idx, S, S_ui)
    t1 = time.perf_counter()
    for idx in batches:
        store.drawn_shape(idx, draw)
    t2 = time.perf_counter()
    return 1e3 * (t1 - t0) / reps, 1e3 * (t2 - t1) / reps


def report_calls(name, store, calls):
    wide = (store.pool_count["user"] > store.draw_keep()) | (store.pool_count["item"] > store.draw_keep())
    print(f"{name}: {store!r}; keep {store.draw_keep()}, mean pool {store.pool_count['user'].mean():.1f} user / "
          f"{store.pool_count['item'].mean():.1f} item sentences, largest {int(store.pool_count['user'].max())} / "
          f"{int(store.pool_count['item'].max())}, {wide.mean():.1%} of the samples above keep", flush=True)
    for batch in (32, 64):
        shape, t = call_times(store, batch, calls)
        plain_ms, drawn_ms = host_times(store, batch)
        print(f"    batch {batch}, (S, L, S_ui, L_ui) = {shape}: " + "; ".join(f"{k} {v:.2f} us" for k, v in t.items())
              + f" per call | host side per batch: plain {plain_ms:.3f} ms, with the draw {drawn_ms:.3f} ms", flush=True)


def worst_case(dev):
    """64 samples whose user and item pools hold 1024 sentences each, out of 20000 distinct ones of 7 .. 18 tokens"""
    from umpr_amd.reviews import ReviewStore
    rng = np.random.default_rng(2)
    sents = [[int(t) for t in rng.integers(3, 2003, size=int(k))] for k in rng.integers(7, 19, size=20000)]
    pool = lambda: [sents[int(j)] for j in rng.integers(0, len(sents), size=1024)]
    n = 64
    return ReviewStore.from_lists([pool() for _ in range(n)], [pool() for _ in range(n)], [pool()[:3] for _ in range(n)],
                                  [3.0] * n, dev, keep=20)


def workload(name, ds, cfg, w2v, store, repeats):
    from bench_review_store import BATCH, epoch
    from torch.utils.data import DataLoader
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    from umpr_amd.photos import Pool5Store
    from umpr_amd.reviews import IndexView, PhotoCollate, ReviewDraw, StoreLoader
    from umpr_amd.train import train_step
    dev = torch.device("cuda:0")
    batch = BATCH[name]
    cfg.review_net_only, cfg.freeze_conv, cfg.dtype = name == "umpr_r", name == "freeze_conv", "fp32"
    torch.manual_seed(0)
    model = UMPR(cfg, w2v.embedding).to(dev)
    opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay)
    step = lambda b: train_step(model, opt, b)
    pool5 = Pool5Store(dev, capacity_bytes=int(1e9)).register(ds.photo_paths()) if name == "freeze_conv" else None
    collate = PhotoCollate(cfg.review_net_only, store=pool5.index if pool5 else None)

    def leg(draw):
        dl = DataLoader(IndexView(ds), batch_size=batch, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(0),
                        collate_fn=collate, num_workers=0, pin_memory=True)
        return StoreLoader(dl, store, draw=draw)

    unk = w2v.word2index[w2v.unknown]
    legs = {"options off (plain collate)": leg(None), f"--review_pool {POOL}": leg(ReviewDraw(1, 0)),
            f"--review_pool {POOL} --word_dropout {DROPOUT}": leg(ReviewDraw(1, 0, DROPOUT, unk))}
    for v in legs.values():                          # warm-up: allocator, workspaces, and the pool5 store fills
        epoch(v, step)
    times = {k: [] for k in legs}
    for r in range(repeats):
        for k, v in (list(legs.items()) if r % 2 == 0 else list(legs.items())[::-1]):
            v.set_epoch(r + 1)
            ms, n = epoch(v, step)
            times[k].append(ms)
    print(f"{name}, batch {batch}, fp32, {n} batches per epoch, review store on the training thread"
          + (f"; pool5 store {pool5.stats()}" if pool5 else ""), flush=True)
    for k, v in times.items():
        print(f"    {k:44s} {statistics.median(v):7.3f} ms per batch   runs: " + ", ".join(f"{x:.3f}" for x in v), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--users", type=int, default=None, help="default items / 2 (8 reviews per user)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--calls", type=int, default=2000, help="calls between two events")
    ap.add_argument("--workloads", default="umpr_r,freeze_conv", help="'' for the calls only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_review_sample.py needs an MI355X: the store lives in device memory")
    from bench_loader import write_corpus
    from umpr_amd.config import Config
    from umpr_amd.data import Dataset, Word2vec
    from umpr_amd.reviews import ReviewStore
    dev = torch.device("cuda:0")
    with tempfile.TemporaryDirectory() as d:
        n = write_corpus(d, a.users or max(200, a.items // 2), a.items)
        cfg = Config(argv=[])
        cfg.views, cfg.review_pool = ["food"], POOL
        w2v = Word2vec(os.path.join(d, "glove.txt"))
        ds = Dataset(os.path.join(d, "train.csv"), os.path.join(d, "photos.json"), os.path.join(d, "photos"), w2v, cfg)
        store = ReviewStore(ds, dev)
        print(f"corpus: {n} reviews -> {len(ds)} samples, Dataset(review_pool={POOL})", flush=True)
        report_calls("bench_loader corpus", store, a.calls)
        report_calls("worst case", worst_case(dev), a.calls)
        for w in filter(None, a.workloads.split(",")):
            workload(w, ds, cfg, w2v, store, a.repeats)


if __name__ == "__main__":
    main()
