#!/usr/bin/env python3
"""What the augmented photo fetch (umpr_photo_fetch_augment_u8, --photo_flip / --photo_crop) costs on an MI355X.

    python tools/bench_augment.py --kernel [--windows 0.08|0.5|flip|all]
        64 resident 224 x 224 photos: the plain fetch (photo_fetch_u8_kernel) and the augmented fetch (photo_augment_u8_kernel) on
        the same 64 slots, alternating in one process, timed with device events; ONE JSON line.  Under
        `rocprofv3 --kernel-trace --stats -- python tools/bench_augment.py --kernel --windows 0.5` the per-kernel times of that
        window set are in the stats file (a run of its own; the event timings of such a run carry the tracer's overhead).
    python tools/bench_augment.py --step [--legs fp32,bf16,freeze_conv]
        training steps at batch 64 on a warm photo store (every photo a hit), augmentation off / on interleaved: ms per step of each
        leg and the spread over the rounds; one JSON line per leg.

No photo files are needed: the slots are filled from random decoded sources through the library itself."""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SIZE = (224, 224)
N = 64


def resident_batch(store, seed=0):
    """Fills N slots of `store` through a cold fetch of random sources; returns a RawPhotos of the same N photos as hits."""
    from umpr_amd.data import _column_taps, _row_taps
    from umpr_amd.photos import RawPhotos
    g = np.random.default_rng(seed)
    dw, dh = SIZE
    dec = []
    for _ in range(N):
        h, w = int(g.integers(200, 400)), int(g.integers(200, 400))
        taps = np.concatenate([*_column_taps(dw, w), *_row_taps(dh, h)]).astype(np.int32)
        dec.append((g.integers(0, 256, (h, w, 3), dtype=np.uint8), taps))
    store.register(f"photo{k}" for k in range(N))
    ids = torch.arange(N, dtype=torch.int32)
    cold = RawPhotos.pack(dec, (N, 1, 1), SIZE)
    cold.ids, cold.hits, cold.store_key = ids, torch.zeros(N, dtype=torch.uint8), store.key
    cold.to(store.device)
    warm = RawPhotos.pack([None] * N, (N, 1, 1), SIZE)
    warm.ids, warm.hits, warm.store_key = ids, torch.ones(N, dtype=torch.uint8), store.key
    assert store.stats()["used"] == N
    return warm


def kernel(args):
    from umpr_amd._lib import lib
    from umpr_amd.photos import PhotoAugment, PhotoStore, tap_tables
    dev = torch.device("cuda:0")
    dw, dh = SIZE
    store = PhotoStore(dev, SIZE, capacity_bytes=N * 150528)
    warm = resident_batch(store)
    src, dst = np.arange(N, dtype=np.int32), np.full(N, -1, dtype=np.int32)
    packed = warm.data.to(dev)
    out = torch.empty(N, 3, dh, dw, device=dev)
    xt, yt = (torch.from_numpy(t).to(dev) for t in tap_tables(SIZE))
    st = torch.cuda.current_stream(dev).cuda_stream
    torch.manual_seed(0)
    sets = {"0.08": PhotoAugment(True, 0.08).draw(1, N), "0.5": PhotoAugment(True, 0.5).draw(1, N),
            "flip": np.tile(np.asarray([0, 0, dw, dh, 1], dtype=np.int32), (N, 1))}
    names = list(sets) if args.windows == "all" else [args.windows]

    def plain():
        lib().call("umpr_photo_fetch_u8", packed, packed.numel(), warm.data, src.ctypes.data, dst.ctypes.data, N, dh, dw, store.buffer,
                   store.slots, out, st)

    def augmented(rec):
        lib().call("umpr_photo_fetch_augment_u8", packed, packed.numel(), warm.data, src.ctypes.data, dst.ctypes.data,
                   rec.ctypes.data, N, dh, dw, store.buffer, store.slots, None, 0, xt, yt, out, st)

    def timed(f):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(args.calls):
            f()
        b.record()
        b.synchronize()
        return 1e3 * a.elapsed_time(b) / args.calls      # us per call

    recs = {k: np.ascontiguousarray(sets[k]) for k in names}
    for k in names:                                       # warm-up: code objects, both kernels
        plain(), augmented(recs[k])
    torch.cuda.synchronize()
    us = {"plain": []}
    for _ in range(args.rounds):                          # alternating: plain, then every window set
        us["plain"].append(timed(plain))
        for k in names:
            us.setdefault(k, []).append(timed(lambda: augmented(recs[k])))
    written = N * 3 * dh * dw * 4
    res = {"bench": "augment_kernel", "photos": N, "calls_per_timing": args.calls, "rounds": args.rounds, "bytes_written": written,
           "note": "device events around back-to-back calls: kernel time plus launch gaps; kernel times alone come from rocprofv3"}
    for k, v in us.items():
        res[k] = {"us_min": round(min(v), 2), "us_median": round(float(np.median(v)), 2), "us_max": round(max(v), 2),
                  "write_TBps_at_median": round(written / np.median(v) / 1e6, 3)}
    for k in names:
        res[k]["ratio_to_plain_median"] = round(float(np.median(us[k]) / np.median(us["plain"])), 3)
    print(json.dumps(res))


def step(args):
    from umpr_amd.config import Config
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    from umpr_amd.photos import PhotoStore
    from umpr_amd.synthetic import make_batch, make_param_state
    from umpr_amd.train import train_step
    dev = torch.device("cuda:0")
    legs = {"fp32": dict(dtype="fp32", emb=50), "bf16": dict(dtype="bf16", emb=300), "freeze_conv": dict(dtype="fp32", emb=50, freeze_conv=True)}
    store = PhotoStore(dev, SIZE, capacity_bytes=N * 150528)
    warm = resident_batch(store)
    vocab = 20003
    for name in args.legs.split(","):
        leg = dict(legs[name])
        emb = leg.pop("emb")
        torch.manual_seed(0)
        P = make_param_state(0, emb, vocab, 1, False)
        text = make_batch(1234, N, vocab, 1, review_net_only=False)
        batch = tuple(text[:6]) + (warm, text[7])
        runs = {}
        for mode in ("off", "on"):
            Config.extend({"dtype": "fp32", "freeze_conv": False, "photo_flip": False, "photo_crop": 1.0})
            cfg = Config(argv=[])
            cfg.review_net_only, cfg.views = False, ["v0"]
            for k, v in leg.items():
                setattr(cfg, k, v)
            if mode == "on":
                cfg.photo_flip, cfg.photo_crop = True, 0.3
            m = UMPR(cfg, P["embedding.weight"].numpy())
            m.load_state_dict(P)
            m = m.to(dev)
            runs[mode] = (m, FusedAdam(m, cfg.learning_rate, cfg.l2_regularization, cfg.lr_decay))
        ms = {"off": [], "on": []}
        for mode, (m, opt) in runs.items():
            for _ in range(args.warmup):
                train_step(m, opt, batch)
        torch.cuda.synchronize()
        for _ in range(args.rounds):
            for mode, (m, opt) in runs.items():
                t0 = time.perf_counter()
                for _ in range(args.steps):
                    train_step(m, opt, batch)
                torch.cuda.synchronize()
                ms[mode].append(1e3 * (time.perf_counter() - t0) / args.steps)
        assert runs["on"][0].photo_augment._calls == args.warmup + args.rounds * args.steps and runs["off"][0].photo_augment is None
        res = {"bench": "augment_step", "leg": name, "batch": N, "steps_per_round": args.steps, "rounds": args.rounds}
        for mode, v in ms.items():
            res[mode] = {"ms_min": round(min(v), 3), "ms_median": round(float(np.median(v)), 3), "ms_max": round(max(v), 3)}
        res["on_minus_off_ms_median"] = round(float(np.median(ms["on"]) - np.median(ms["off"])), 3)
        print(json.dumps(res), flush=True)
        del runs, m, opt
        torch.cuda.empty_cache()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--kernel", action="store_true")
    ap.add_argument("--step", action="store_true")
    ap.add_argument("--windows", default="all", choices=["0.08", "0.5", "flip", "all"])
    ap.add_argument("--calls", type=int, default=50, help="--kernel: calls per timing")
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--legs", default="fp32,bf16,freeze_conv")
    ap.add_argument("--steps", type=int, default=10, help="--step: timed steps per round")
    ap.add_argument("--warmup", type=int, default=3)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        sys.exit("bench_augment.py measures on an MI355X: no GPU, no number")
    if args.kernel:
        kernel(args)
    if args.step:
        step(args)


if __name__ == "__main__":
    main()
