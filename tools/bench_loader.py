#!/usr/bin/env python3
"""Real-data path throughput: a synthetic corpus in the reference's on-disk layout
(train.csv, photos.json, photos/*.jpg, GloVe text) -> umpr_amd.data.Dataset -> DataLoader(batch_loader) -> UMPR.
Prints, for both forms of the photo element (host: decode + resize + /255 on the host, float32 upload; gpu: decode on the
host, uint8 upload, resize in csrc/photos.hip - what main.py uses), loader-only samples/s for several worker counts and
where the host time of one photo goes; then end-to-end training samples/s with each form at its best worker count.

    python tools/bench_loader.py [--items 64] [--users 200] [--batch 64] [--workers 0,4,8,12] [--steps 20]

With `--photo_store_gb X` it measures the device-resident photo store (umpr_amd/photos.py::PhotoStore) instead: per worker
count (default 0,4,8) whole epochs of the gpu form with the store off (twice: the spread), on and cold, on and warm, the
forms alternating; then end-to-end training, fp32 and bf16, store off and warm, beside bench.py's resident-batch rate.

    python tools/bench_loader.py --items 2000 --photo_store_gb 1

With `--freeze_vgg True` it measures the frozen VGG and the feature store (umpr_amd/photos.py::FeatureStore, capacity
`--feature_store_gb`, default 1): per arithmetic mode and worker count, end-to-end training epochs with the VGG trainable (photo
store warm), frozen without a store, frozen with the photo store warm, frozen with the feature store cold, and frozen with it warm.

    python tools/bench_loader.py --items 2000 --freeze_vgg True --workers 0,4

With `--freeze_conv True` it measures the frozen conv base and the pool5 store (umpr_amd/photos.py::Pool5Store, capacity
`--pool5_store_gb`, default 1): the same five legs with the classifier training - trainable with the photo store warm, conv base
frozen without a store, with the photo store warm, with the pool5 store cold, and with it warm.

    python tools/bench_loader.py --items 2000 --freeze_conv True --workers 0,4
"""
import argparse
import functools
import json
import os
import random
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def write_corpus(root, n_users, n_items, seed=3):
    from PIL import Image
    rnd = random.Random(seed)
    words = ["w%d" % i for i in range(2000)]
    with open(os.path.join(root, "glove.txt"), "w") as f:
        for w in words:
            f.write(w + " " + " ".join("%.4f" % rnd.uniform(-1, 1) for _ in range(50)) + "\n")
    rows = []
    for u in range(n_users):
        for it in rnd.sample(range(n_items), 8):
            sents = [" ".join(rnd.choice(words) for _ in range(rnd.randint(7, 18))) for _ in range(rnd.randint(2, 4))]
            rows.append(dict(userID="U%d" % u, itemID="I%d" % it, review=" . ".join(sents) + " .",
                             rating=float(rnd.randint(1, 5)), user_num=u, item_num=it))
    import pandas as pd
    pd.DataFrame(rows).to_csv(os.path.join(root, "train.csv"), index=False)
    os.makedirs(os.path.join(root, "photos"))
    g = np.random.default_rng(seed)
    with open(os.path.join(root, "photos.json"), "w") as f:
        for it in range(n_items):
            f.write(json.dumps(dict(business_id="I%d" % it, photo_id="p%d" % it, label="food")) + "\n")
            # smooth random field at a typical photo size: JPEG decode cost close to a real picture's
            low = g.random((24, 32, 3))
            img = Image.fromarray((low * 255).astype(np.uint8)).resize((500, 375), Image.BICUBIC)
            img.save(os.path.join(root, "photos", "p%d.jpg" % it), quality=90)
    return len(rows)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--items", type=int, default=64)
    ap.add_argument("--users", type=int, default=None, help="default 200; items / 2 with --photo_store_gb (8 reviews per "
                    "user: 4 per item on average, so that most items pass the dataset's minimum sentence count)")
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--workers", default=None, help="default 0,4,8,12; 0,4,8 with --photo_store_gb")
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--photo_store_gb", type=float, default=0.0, help="measure the photo store with this capacity")
    ap.add_argument("--freeze_vgg", type=lambda t: t == "True", default=False, help="True: measure the frozen VGG")
    ap.add_argument("--feature_store_gb", type=float, default=0.0, help="capacity of the feature store (with --freeze_vgg True; "
                    "default 1)")
    ap.add_argument("--freeze_conv", type=lambda t: t == "True", default=False, help="True: measure the frozen conv base")
    ap.add_argument("--pool5_store_gb", type=float, default=0.0, help="capacity of the pool5 store (with --freeze_conv True; "
                    "default 1)")
    ap.add_argument("--dtypes", default="fp32,bf16", help="arithmetic modes of the --freeze_vgg / --freeze_conv legs")
    a = ap.parse_args()
    if a.feature_store_gb > 0 and not a.freeze_vgg:
        sys.exit("--feature_store_gb needs --freeze_vgg True")
    if a.pool5_store_gb > 0 and not a.freeze_conv:
        sys.exit("--pool5_store_gb needs --freeze_conv True")
    if a.freeze_conv and a.freeze_vgg:
        sys.exit("--freeze_conv True and --freeze_vgg True exclude each other")
    stores = a.photo_store_gb > 0 or a.freeze_vgg or a.freeze_conv
    a.workers = a.workers or ("0,4,8" if stores else "0,4,8,12")
    a.users = a.users or (max(200, a.items // 2) if stores else 200)
    resident = resident_rates(a.batch) if a.photo_store_gb > 0 and not (a.freeze_vgg or a.freeze_conv) else None
    from torch.utils.data import DataLoader
    from main import _Collate
    from umpr_amd.config import Config
    from umpr_amd.data import Dataset, Word2vec, batch_loader
    with tempfile.TemporaryDirectory() as d:
        n = write_corpus(d, a.users, a.items)
        cfg = Config(argv=[])
        cfg.views = ["food"]
        w2v = Word2vec(os.path.join(d, "glove.txt"))
        t0 = time.perf_counter()
        ds = Dataset(os.path.join(d, "train.csv"), os.path.join(d, "photos.json"), os.path.join(d, "photos"), w2v, cfg)
        print(f"corpus: {n} reviews -> {len(ds)} samples, Dataset built in {time.perf_counter() - t0:.2f} s", flush=True)
        photo = ds[0][3][0][0]
        per_photo(photo)
        if a.freeze_vgg or a.freeze_conv:
            return frozen_vgg(a, ds, cfg, w2v)
        if a.photo_store_gb > 0:
            return photo_store(a, ds, cfg, w2v, resident)
        forms = {"host": functools.partial(batch_loader, ignore_photos=False, resize_on_gpu=False), "gpu": _Collate(False)}
        best = {}
        for w in [int(x) for x in a.workers.split(",")]:
            for form, collate in forms.items():
                kw = dict(collate_fn=collate, num_workers=w, pin_memory=torch.cuda.is_available())
                if w:
                    kw.update(prefetch_factor=2, persistent_workers=True)
                dl = DataLoader(ds, batch_size=a.batch, shuffle=True, **kw)
                it = iter(dl)
                next(it)  # workers started, first batch decoded
                t0 = time.perf_counter()
                k = 0
                for b in it:
                    k += 1
                    if k >= a.steps:
                        break
                dt = time.perf_counter() - t0
                rate = k * a.batch / dt
                print(f"loader only, {form:4s} form, {w:2d} workers: {rate:8.1f} samples/s ({1e3 * dt / k:.1f} ms per batch of "
                      f"{a.batch})", flush=True)
                if rate > best.get(form, (0.0, 0))[0]:
                    best[form] = (rate, w)
                del it, dl
        if not torch.cuda.is_available():
            return
        from umpr_amd.model import UMPR
        from umpr_amd.optim import FusedAdam
        from umpr_amd.train import train_step
        dev = torch.device("cuda:0")
        for form in ("gpu", "host"):
            torch.manual_seed(0)
            model = UMPR(cfg, w2v.embedding).to(dev)
            opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay)
            w = best[form][1]
            kw = dict(collate_fn=forms[form], num_workers=w, pin_memory=True)
            if w:
                kw.update(prefetch_factor=2, persistent_workers=True)
            dl = DataLoader(ds, batch_size=a.batch, shuffle=True, drop_last=True, **kw)
            it = iter(dl)
            for _ in range(3):
                train_step(model, opt, next(it))
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            k = 0
            for b in it:
                train_step(model, opt, b)
                k += 1
                if k >= a.steps:
                    break
            torch.cuda.synchronize()
            dt = time.perf_counter() - t0
            print(f"end to end (CSV + JPEG decode + collate + H2D + train step), {form} form, {w} workers: "
                  f"{k * a.batch / dt:.1f} samples/s ({1e3 * dt / k:.1f} ms per step)", flush=True)
            del it, dl, model, opt


def _loader(a, ds, w, store):
    from torch.utils.data import DataLoader
    from main import _Collate
    kw = dict(collate_fn=_Collate(False, store=store.index if store else None), num_workers=w, pin_memory=True)
    if w:
        kw.update(prefetch_factor=2, persistent_workers=True)
    return DataLoader(ds, batch_size=a.batch, shuffle=True, drop_last=True, **kw)


def _epoch(a, dl, step=None):
    """samples/s of one epoch of `dl`, timed from the first batch's arrival (which leaves the workers' start out)."""
    it = iter(dl)
    first = next(it)
    if step:
        step(first)
    t0 = time.perf_counter()
    k = 0
    for b in it:
        if step:
            step(b)
        k += 1
    torch.cuda.synchronize()
    return k * a.batch / (time.perf_counter() - t0)


def frozen_vgg(a, ds, cfg, w2v):
    """End-to-end training epochs of `ds` (CSV + JPEG decode + collate + H2D + train step): the VGG trainable with the photo store
    warm, frozen without a store (the loader decodes every photo: on few workers that, not the GPU, sets the rate), frozen with the
    photo store warm (the same loader work as the trainable leg: the difference is the VGG alone), frozen with the feature store
    cold (the epoch that fills it) and warm.  Every leg runs one warm-up epoch first (allocator, workspaces, first-use setup, the
    worker pool's start) - except the cold epoch, which can only happen once: its model has run epochs before, and its worker
    pool has served one loader-only epoch, which makes nothing resident.
    With --freeze_conv True the same legs for the frozen conv base (the classifier trains) and the pool5 store."""
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    from umpr_amd.photos import FeatureStore, PhotoStore, Pool5Store
    from umpr_amd.train import train_step
    if not torch.cuda.is_available():
        sys.exit("--freeze_vgg / --freeze_conv need an MI355X")
    flag, frozen, kept = ("freeze_conv", "conv frozen", "pool5 store") if a.freeze_conv else ("freeze_vgg", "frozen", "feature store")
    dev = torch.device("cuda:0")
    paths = list(ds.photo_paths())
    print(f"an epoch: {len(ds) // a.batch} batches of {a.batch}, {len(set(paths) - {'unknown'})} distinct photos", flush=True)
    for dtype in a.dtypes.split(","):
        cfg.dtype = dtype
        for w in [int(x) for x in a.workers.split(",")]:
            rates = {}

            def leg(freeze):
                setattr(cfg, flag, freeze)
                torch.manual_seed(0)
                model = UMPR(cfg, w2v.embedding).to(dev)
                opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay)
                return model, opt, (lambda b: train_step(model, opt, b))

            model, opt, step = leg(False)
            store = PhotoStore(dev, capacity_bytes=int((a.photo_store_gb or 1.0) * 1e9)).register(paths)
            dl = _loader(a, ds, w, store)
            _epoch(a, dl, step)
            rates["trainable, photo store warm"] = _epoch(a, dl, step)
            del model, opt, step, dl, store
            model, opt, step = leg(True)
            dl = _loader(a, ds, w, None)
            _epoch(a, dl, step)
            rates[f"{frozen}, no store"] = _epoch(a, dl, step)
            del dl
            store = PhotoStore(dev, capacity_bytes=int((a.photo_store_gb or 1.0) * 1e9)).register(paths)
            dl = _loader(a, ds, w, store)
            _epoch(a, dl, step)
            rates[f"{frozen}, photo store warm"] = _epoch(a, dl, step)
            del dl, store
            if a.freeze_conv:
                store = Pool5Store(dev, capacity_bytes=int((a.pool5_store_gb or 1.0) * 1e9)).register(paths)
            else:
                store = FeatureStore(dev, capacity_bytes=int((a.feature_store_gb or 1.0) * 1e9)).register(paths)
            dl = _loader(a, ds, w, store)
            _epoch(a, dl)
            rates[f"{frozen}, {kept} cold"] = _epoch(a, dl, step)
            rates[f"{frozen}, {kept} warm"] = _epoch(a, dl, step)
            print(f"end to end, {dtype}, {w:2d} workers: " + ", ".join(f"{k} {v:.1f} samples/s" for k, v in rates.items()),
                  flush=True)
            print(f"    {kept}: {store.stats()}", flush=True)
            del model, opt, step, dl, store
    setattr(cfg, flag, False)


def photo_store(a, ds, cfg, w2v, resident):
    """The store against the plain gpu form, in whole epochs of `ds` (timed from the first batch's arrival, which leaves the
    workers' start out).  A store epoch includes RawPhotos.to(device) for every batch - that is what makes photos resident -
    and a final synchronize; the store-off epochs are the loader alone, as in the plain run."""
    from torch.utils.data import DataLoader
    from main import _Collate
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    from umpr_amd.photos import PhotoStore
    from umpr_amd.train import train_step
    if not torch.cuda.is_available():
        sys.exit("--photo_store_gb needs an MI355X: the store lives in device memory")
    dev = torch.device("cuda:0")
    print(f"an epoch: {len(ds) // a.batch} batches of {a.batch}, {len(set(ds.photo_paths()) - {'unknown'})} distinct photos",
          flush=True)

    def loader(w, store):
        kw = dict(collate_fn=_Collate(False, store=store.index if store else None), num_workers=w, pin_memory=True)
        if w:
            kw.update(prefetch_factor=2, persistent_workers=True)
        return DataLoader(ds, batch_size=a.batch, shuffle=True, drop_last=True, **kw)

    def epoch(dl, step=None):
        it = iter(dl)
        first = next(it)
        if step:
            step(first)
        t0 = time.perf_counter()
        k = 0
        for b in it:
            if step:
                step(b)
            k += 1
        torch.cuda.synchronize()
        return k * a.batch / (time.perf_counter() - t0)

    # one worker pool at a time: off, on (cold, then warm on the same persistent workers), off again
    for w in [int(x) for x in a.workers.split(",")]:
        dl = loader(w, None)
        print(f"loader only, store off,       {w:2d} workers: {epoch(dl):8.1f} samples/s", flush=True)
        del dl
        store = PhotoStore(dev, capacity_bytes=int(a.photo_store_gb * 1e9)).register(ds.photo_paths())
        fetch = lambda b: b[6].to(dev, non_blocking=True)
        dl = loader(w, store)
        print(f"loader only, store on (cold), {w:2d} workers: {epoch(dl, fetch):8.1f} samples/s", flush=True)
        print(f"loader only, store on (warm), {w:2d} workers: {epoch(dl, fetch):8.1f} samples/s   {store.stats()}", flush=True)
        del dl
        dl = loader(w, None)
        print(f"loader only, store off again, {w:2d} workers: {epoch(dl):8.1f} samples/s", flush=True)
        del dl
        for dtype in ("fp32", "bf16"):
            cfg.dtype = dtype
            rates = {}
            for name, st in (("store off", None), ("store on, warm", store)):
                torch.manual_seed(0)
                model = UMPR(cfg, w2v.embedding).to(dev)
                opt = FusedAdam(model, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay)
                step = lambda b: train_step(model, opt, b)
                dl = loader(w, st)
                epoch(dl, step)                      # warm-up: allocator, workspaces, first-use setup
                rates[name] = epoch(dl, step)
                del model, opt, dl
            print(f"end to end, {dtype}, {w:2d} workers: " + ", ".join(f"{k} {v:.1f} samples/s" for k, v in rates.items()),
                  flush=True)
        del store
    for dtype, rate in resident.items():
        print(f"resident batch (bench.py --dtype {dtype}): {rate:.1f} samples/s", flush=True)


def resident_rates(batch):
    """bench.py's training samples/s on a batch resident in HBM, fp32 and bf16: child processes, run before this process
    touches the GPU (a process that has initialised the GPU starts no other GPU program)."""
    import subprocess
    rates = {}
    for dtype in ("fp32", "bf16"):
        out = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", "20", "--warmup", "5",
                              "--batch", str(batch), "--dtype", dtype], capture_output=True, text=True, check=True).stdout
        rates[dtype] = [json.loads(l) for l in out.splitlines() if l.startswith("{")][-1]["value"]
    return rates


def per_photo(path, reps=20):
    """Host time of one photo on this thread, by stage: the host form's get_image and float32 cast, and the gpu form's
    decode, tap tables + compaction, and share of RawPhotos.pack."""
    from PIL import Image
    from umpr_amd.data import _column_taps, _row_taps, get_image
    from umpr_amd.photos import RawPhotos, decode_for_gpu

    def ms(f):
        f()
        t0 = time.perf_counter()
        for _ in range(reps):
            f()
        return 1e3 * (time.perf_counter() - t0) / reps

    def decode():
        with Image.open(path) as im:
            return np.asarray(im.convert("RGB"), dtype=np.uint8)

    one = decode_for_gpu(path)
    t_dec = ms(decode)
    t_host = ms(lambda: get_image(path).astype(np.float32))
    t_gpu = ms(lambda: decode_for_gpu(path))
    t_pack = ms(lambda: RawPhotos.pack([one] * 64, (64, 1, 1), (224, 224))) / 64
    t_pin = ms(lambda: RawPhotos.pack([one] * 64, (64, 1, 1), (224, 224)).pin_memory()) / 64 - t_pack \
        if torch.cuda.is_available() else float("nan")
    print(f"per photo ({path.rsplit('/', 1)[-1]}): decode {t_dec:.2f} ms; host form get_image + float32 {t_host:.2f} ms; "
          f"gpu form decode_for_gpu {t_gpu:.2f} ms (taps + compaction {t_gpu - t_dec:.2f}), pack {t_pack:.3f} ms, "
          f"pin {t_pin:.3f} ms; upload {one[0].nbytes + 16 * 448} B vs {3 * 224 * 224 * 4} B", flush=True)


if __name__ == "__main__":
    main()
