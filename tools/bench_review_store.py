#!/usr/bin/env python3
"""The review store (umpr_amd/reviews.py::ReviewStore, main.py --review_store True) against the host collate, in whole training
epochs of tools/bench_loader.py's corpus, end to end (loader + collate + train step), with a device synchronise at the end of
every epoch.  Two workloads: UMPR-R (--review_net_only True) at batch 32, and the frozen conv base with a warm pool5 store
(--freeze_conv True --pool5_store_gb) at batch 64, fp32.  Three legs each, interleaved and repeated three times after one warm-up
epoch per leg: host collate on the training thread, host collate in 4 workers, review store on the training thread.  Beside them
the text-only host collate alone on the training thread (ms per batch) and the store's device bytes against the per-sample token
count.  The last line of a workload says whether the store leg's time per batch is at most the host leg's minus 0.8 x the host
collate's (the 20 % is for the host work that stays: the index draw, the length gather, the launch).

    python tools/bench_review_store.py [--items 2000] [--repeats 3] [--workloads umpr_r,freeze_conv]

The kernel's time per call beside the feature fetch's comes from a run of its own, a short frozen-conv epoch from the store:

    rocprofv3 --kernel-trace --stats --output-format csv -d DIR -- python tools/bench_review_store.py --trace
    python tools/bench_review_store.py --stats DIR
"""
import argparse
import csv
import glob
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

BATCH = {"umpr_r": 32, "freeze_conv": 64}


def kernel_stats(directory):
    """time per call of the review collate and of the feature fetch from a rocprofv3 --kernel-trace --stats directory"""
    files = glob.glob(os.path.join(directory, "**", "*kernel_stats.csv"), recursive=True)
    if not files:
        sys.exit(f"no *kernel_stats.csv under {directory}")
    for f in files:
        for row in csv.DictReader(open(f)):
            name = next((k for k in ("review_collate_kernel", "feature_fetch_f32_kernel") if k in row.get("Name", "")), None)
            if name:
                print(f"{name:26s} calls {row['Calls']:>6s}  average {float(row['AverageNs']) / 1e3:7.2f} us  "
                      f"min {float(row['MinNs']) / 1e3:7.2f} us  max {float(row['MaxNs']) / 1e3:7.2f} us", flush=True)


def loaders(ds, reviews, batch, review_net_only, photo_index):
    from torch.utils.data import DataLoader
    from main import _Collate
    from umpr_amd.reviews import IndexView, PhotoCollate, StoreLoader

    def dl(data, collate, workers):
        kw = dict(collate_fn=collate, num_workers=workers, pin_memory=True)
        if workers:
            kw.update(prefetch_factor=2, persistent_workers=True)
        return DataLoader(data, batch_size=batch, shuffle=True, drop_last=True, generator=torch.Generator().manual_seed(0), **kw)

    host = _Collate(review_net_only, store=photo_index)
    return {"host collate, training thread": dl(ds, host, 0), "host collate, 4 workers": dl(ds, host, 4),
            "review store, training thread": StoreLoader(dl(IndexView(ds), PhotoCollate(review_net_only, store=photo_index), 0),
                                                         reviews)}


def epoch(loader, step):
    """(ms per batch, batches) of one epoch, the final synchronise included"""
    t0 = time.perf_counter()
    k = 0
    for b in loader:
        step(b)
        k += 1
    torch.cuda.synchronize()
    return 1e3 * (time.perf_counter() - t0) / k, k


def collate_alone(ds, batch):
    """the text-only host collate on this thread, ms per batch over one epoch's batches"""
    from umpr_amd.data import batch_loader
    order = torch.randperm(len(ds), generator=torch.Generator().manual_seed(0)).tolist()
    groups = [[ds[i] for i in order[k:k + batch]] for k in range(0, len(order) - batch + 1, batch)]
    batch_loader(groups[0], ignore_photos=True)
    t0 = time.perf_counter()
    for g in groups:
        batch_loader(g, ignore_photos=True)
    return 1e3 * (time.perf_counter() - t0) / len(groups)


def workload(name, ds, cfg, w2v, reviews, repeats, trace=False):
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    from umpr_amd.photos import Pool5Store
    from umpr_amd.train import train_step
    dev = torch.device("cuda:0")
    batch = BATCH[name]
    cfg.review_net_only, cfg.freeze_conv, cfg.dtype = name == "umpr_r", name == "freeze_conv", "fp32"
    torch.manual_seed(0)
    model = UMPR(cfg, w2v.embedding).to(dev)
    opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay)
    step = lambda b: train_step(model, opt, b)
    pool5 = None
    if name == "freeze_conv":
        pool5 = Pool5Store(dev, capacity_bytes=int(1e9)).register(ds.photo_paths())
    legs = loaders(ds, reviews, batch, cfg.review_net_only, pool5.index if pool5 else None)
    if trace:
        legs = {k: v for k, v in legs.items() if k.startswith("review store")}
    for leg in legs.values():                       # warm-up: allocator, workspaces, worker pool, and the pool5 store fills
        epoch(leg, step)
    if trace:
        return epoch(legs["review store, training thread"], step)
    times = {k: [] for k in legs}
    for _ in range(repeats):
        for k, leg in legs.items():
            ms, n = epoch(leg, step)
            times[k].append(ms)
    alone = collate_alone(ds, batch)
    print(f"{name}, batch {batch}, fp32, {n} batches per epoch" + (f"; pool5 store {pool5.stats()}" if pool5 else ""), flush=True)
    med = {}
    for k, v in times.items():
        med[k] = statistics.median(v)
        print(f"    {k:32s} {med[k]:7.3f} ms per batch ({1e3 * batch / med[k]:9.1f} samples/s)   runs: "
              + ", ".join(f"{x:.3f}" for x in v), flush=True)
    print(f"    {'host collate alone (text only)':32s} {alone:7.3f} ms per batch", flush=True)
    host, store = med["host collate, training thread"], med["review store, training thread"]
    bound = host - 0.8 * alone
    print(f"    store leg {store:.3f} ms <= host leg {host:.3f} ms - 0.8 x {alone:.3f} ms = {bound:.3f} ms: "
          f"{'yes' if store <= bound else 'NO'}", flush=True)
    del legs
    return store <= bound


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=2000)
    ap.add_argument("--users", type=int, default=None, help="default items / 2 (8 reviews per user)")
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--workloads", default="umpr_r,freeze_conv")
    ap.add_argument("--trace", action="store_true", help="one short frozen-conv epoch from the store only (for rocprofv3)")
    ap.add_argument("--stats", default="", help="print the two kernels' lines of a rocprofv3 --stats directory and exit")
    a = ap.parse_args()
    if a.stats:
        return kernel_stats(a.stats)
    if not torch.cuda.is_available():
        sys.exit("bench_review_store.py needs an MI355X: the store lives in device memory")
    from bench_loader import write_corpus
    from umpr_amd.config import Config
    from umpr_amd.data import Dataset, Word2vec
    from umpr_amd.reviews import ReviewStore
    if a.trace:
        a.items = min(a.items, 400)
    with tempfile.TemporaryDirectory() as d:
        n = write_corpus(d, a.users or max(200, a.items // 2), a.items)
        cfg = Config(argv=[])
        cfg.views = ["food"]
        w2v = Word2vec(os.path.join(d, "glove.txt"))
        ds = Dataset(os.path.join(d, "train.csv"), os.path.join(d, "photos.json"), os.path.join(d, "photos"), w2v, cfg)
        t0 = time.perf_counter()
        reviews = ReviewStore(ds, torch.device("cuda:0"))
        print(f"corpus: {n} reviews -> {len(ds)} samples; {reviews!r}, built in {time.perf_counter() - t0:.2f} s", flush=True)
        st = reviews.stats()
        print(f"    {st['bytes']} B on the device; {st['tokens']} tokens stored against {st['per_sample_tokens']} per sample "
              f"({st['per_sample_tokens'] / max(st['tokens'], 1):.1f} x)", flush=True)
        if a.trace:
            ms, k = workload("freeze_conv", ds, cfg, w2v, reviews, 1, trace=True)
            print(f"traced epoch: {k} batches, {ms:.3f} ms per batch", flush=True)
            return
        ok = [workload(w, ds, cfg, w2v, reviews, a.repeats) for w in a.workloads.split(",")]
        sys.exit(0 if all(ok) else 1)


if __name__ == "__main__":
    main()
