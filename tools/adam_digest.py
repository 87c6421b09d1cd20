"""usage: python tools/adam_digest.py OUT.json
sha256 of what the dense Adam update writes, through public names only, so that the same file runs against two trees:
  - p, m, v after three steps through each of the four entry points umpr_adam_step[_dev][_clip], for the element counts and
    start offsets of tests/test_gpu_grad_clip.py, weight decay 1e-3 and 0, clip coefficient 1 and 0.37 and a non-finite step;
  - every parameter / moment arena (and the clip state) after three optimiser steps of a seeded UMPR-R at batch 4: plain, clipped,
    as a captured graph, with two micro-batches per step, with a sparse table - each without and with clipping;
  - the arenas after two steps of the full fp32 model at batch 2, with the early classifier update armed and with
    UMPR_EARLY_ADAM=0 (each in a child process: the switch is read at import).
Run it on two builds and compare the files: equal digests = byte-identical optimiser state (how a change to the Adam kernels or to
FusedAdam's step path is held against its parent)."""
import hashlib
import json
import math
import os
import subprocess
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from umpr_amd._lib import lib  # noqa: E402
from umpr_amd.config import Config  # noqa: E402
from umpr_amd.model import UMPR  # noqa: E402
from umpr_amd.optim import FusedAdam  # noqa: E402
from umpr_amd.synthetic import make_batch, make_param_state  # noqa: E402
from umpr_amd.train import train_step  # noqa: E402

SIZES = [1, 257, 100003, 8192 * 256 + 77]
OFFSETS = [0, 1]
PAD = 64


def digest(*tensors):
    torch.cuda.synchronize()
    h = hashlib.sha256()
    for t in tensors:
        h.update(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes())
    return h.hexdigest()


# ---- the four entry points ----------------------------------------------------------------------------------------------------
def kernels(out, dev):
    L = lib()
    st = torch.cuda.current_stream().cuda_stream
    for n in SIZES:
        g = torch.Generator().manual_seed(9)
        start = [torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.rand(n, generator=g) * 0.1,
                 torch.rand(n, generator=g) * 0.01]
        for off in OFFSETS:
            for wd in (1e-3, 0.0):
                for entry in ("umpr_adam_step", "umpr_adam_step_dev", "umpr_adam_step_clip", "umpr_adam_step_dev_clip"):
                    clip = entry.endswith("_clip")
                    for coef, finite in (((1.0, 1.0), (0.37, 1.0), (0.0, 0.0)) if clip else ((None, None),)):
                        bufs = [torch.full((PAD + off + n + PAD,), -7.5, device=dev) for _ in start]
                        p, gr, m, v = [b[PAD + off:PAD + off + n] for b in bufs]
                        for t, s in zip((p, gr, m, v), start):
                            t.copy_(s)
                        state = torch.tensor([coef, 1.0, finite, 1.0, 0, 0, 0, 0], dtype=torch.float32, device=dev) if clip else None
                        tail = (state, st) if clip else (st,)
                        for step in (1, 2, 3):
                            if "_dev" in entry:
                                hyper = torch.tensor([0.5, 1e-3 / (1 - 0.9 ** step), 1 / math.sqrt(1 - 0.999 ** step), wd],
                                                     dtype=torch.float32, device=dev)
                                L.call(entry, p, gr, m, v, n, 0.9, 0.999, 1e-8, hyper, *tail)
                            else:
                                L.call(entry, p, gr, m, v, n, 1e-3, 0.9, 0.999, 1e-8, wd, step, 0.5, *tail)
                        # the whole buffers: what the kernel wrote and the elements on both sides of it
                        out[f"kernel {entry} n={n} off={off} wd={wd} coef={coef} finite={finite}"] = digest(*bufs)


# ---- FusedAdam on UMPR-R ------------------------------------------------------------------------------------------------------
def optimiser_state(opt):
    ts = [t for g in opt.groups for t in (g.p, g.m, g.v)]
    if opt.sparse is not None:
        _, table, m, v = opt.sparse
        ts += [table, m, v]
    if opt.clip_state is not None:
        ts.append(opt.clip_state)
    return digest(*ts)


def _config(**kw):
    cfg = Config(argv=[])
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def umpr_r(out, dev):
    from umpr_amd.graphs import GraphedTrainStep
    P = make_param_state(31, 50, 1000, 1, True, m_scale=0.05)
    batches = [make_batch(500 + s, 4, 1000, review_net_only=True, full_pad=True) for s in range(6)]
    for mode in ("plain", "graph", "accum2", "sparse"):
        for max_norm in (0.0, 0.5):
            torch.manual_seed(5)
            kw = dict(train_embedding=True, sparse_embedding=True) if mode == "sparse" else {}
            model = UMPR(_config(review_net_only=True, **kw), P["embedding.weight"].numpy())
            model.load_state_dict(P)
            model = model.to(dev)
            opt = FusedAdam(model, 1e-3, 1e-3, max_grad_norm=max_norm)
            if mode == "graph":
                graphed = GraphedTrainStep(model, opt, batches[0])
                for b in batches[:3]:
                    graphed(b)
            elif mode == "accum2":
                for k in range(3):
                    train_step(model, opt, batches[2 * k], update=False)
                    train_step(model, opt, batches[2 * k + 1])
            else:
                for b in batches[:3]:
                    train_step(model, opt, b)
            assert opt.step_count == 3
            key = f"umpr_r {mode} max_grad_norm={max_norm}"
            if max_norm > 0.0:
                stats = opt.clip_stats()
                assert stats["clipped"] > 0 and stats["skipped"] == 0, stats
                out[key + " clip_stats"] = stats
            out[key] = optimiser_state(opt)
            opt.close()


# ---- FusedAdam on the full model (a child process per UMPR_EARLY_ADAM setting) ------------------------------------------------
def full_model(out_path):
    dev = torch.device("cuda:0")
    P = make_param_state(121, 50, 500, 1, False, m_scale=0.05)
    model = UMPR(_config(views=["unknown"]), P["embedding.weight"].numpy())
    model.load_state_dict(P)
    model = model.to(dev)
    torch.manual_seed(5)
    opt = FusedAdam(model, 1e-3, 1e-3)
    for i in range(2):
        train_step(model, opt, make_batch(130 + i, 2, 500, 1))
    with open(out_path, "w") as fh:
        json.dump({"digest": optimiser_state(opt)}, fh)


def full_model_children(out, out_path):
    for early in ("1", "0"):
        tmp = f"{out_path}.full{early}"
        subprocess.run([sys.executable, os.path.abspath(__file__), "--full-model", tmp], check=True,
                       env=dict(os.environ, UMPR_EARLY_ADAM=early))
        with open(tmp) as fh:
            out[f"full_f32 batch 2, two steps, UMPR_EARLY_ADAM={early}"] = json.load(fh)["digest"]
        os.remove(tmp)


def main(out_path):
    out = {}
    full_model_children(out, out_path)      # first: this process has not touched the GPU yet, each child has it to itself
    dev = torch.device("cuda:0")
    kernels(out, dev)
    umpr_r(out, dev)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print(f"{len(out)} entries -> {out_path}")


if __name__ == "__main__":
    if sys.argv[1] == "--full-model":
        full_model(sys.argv[2])
    else:
        main(sys.argv[1])
