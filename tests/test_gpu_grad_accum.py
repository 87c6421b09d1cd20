"""Gradient accumulation on the GPU (umpr_grad_accumulate in csrc/optim.hip, FusedAdam.accumulate, train_step(update=),
--accum_steps): the kernel against np.float32 addition bit for bit, the optimiser's plumbing against a twin that is handed the
chained sum and the scale 1 / k, with clipping, on the full model, against the oracle driven with (loss / 2).backward() twice +
clip_grad_norm_ + Adam (fixture grad_accum_umpr_r, written by tests/golden/make_grad_accum_golden.py), across a checkpoint, and
that a run which never accumulates is the run it was."""
import ctypes
import math

import numpy as np
import pytest
import torch

from conftest import load_golden

pytestmark = pytest.mark.gpu

# umpr_grad_accumulate: 2048 workgroups of 256 threads; one pass of the grid covers that many float4s where acc and grads sit
# alike inside a 16-byte line, that many floats where they do not; four passes per iteration of the unrolled loop
BLOCKS, THREADS = 2048, 256
SWEEP = BLOCKS * THREADS * 4
GUARD = 64
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, BLOCKS * THREADS + 3, SWEEP + 5, 4 * SWEEP + 9]


@pytest.fixture(scope="module")
def L():
    from umpr_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


def _cfg(**kw):
    from umpr_amd.config import Config
    cfg = Config(argv=[])
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.fixture(scope="module")
def pool():
    """three gradients of 4 * SWEEP + 9 normal-range floats with exact zeros of both signs at the same places (so that
    -0 + -0, +0 + -0 and x + -0 all occur) and one +inf; every test takes prefixes"""
    rng = np.random.default_rng(17)
    gs = [rng.standard_normal(4 * SWEEP + 9).astype(np.float32) * np.float32(10.0 ** (j - 1)) for j in range(3)]
    for g in gs:
        g[7::64] = -0.0
    gs[0][13::64], gs[1][13::64], gs[2][13::64] = 0.0, -0.0, -0.0
    gs[1][19::64] = 0.0
    gs[1][2] = np.inf
    return gs


class _Buf:
    """n floats behind `off` floats of padding, between two NaN guard bands of 64 floats (the padding is guard as well)"""

    def __init__(self, vals, off, dev):
        n = len(vals)
        self.host = np.full(GUARD + off + n + GUARD, np.nan, np.float32)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.host[self.lo:self.hi] = vals
        self.dev = torch.from_numpy(self.host.copy()).to(dev)
        self.n, self.ptr = n, self.dev.data_ptr() + 4 * self.lo      # (an empty view would report a null pointer)
        assert self.dev.data_ptr() % 256 == 0 and self.ptr % 16 == 4 * (off % 4)

    def check(self, want, what):
        got = self.dev.cpu().numpy()
        assert _bits(got[:self.lo]).tobytes() == _bits(self.host[:self.lo]).tobytes(), what + ": guard in front"
        assert _bits(got[self.hi:]).tobytes() == _bits(self.host[self.hi:]).tobytes(), what + ": guard behind"
        bad = np.flatnonzero(_bits(got[self.lo:self.hi]) != _bits(want))
        assert bad.size == 0, (what, bad[:5], got[self.lo:self.hi][bad[:5]], np.asarray(want)[bad[:5]])


def _accumulate(L, accs, grads, first, counts=None):
    k = max(len(accs), 1)
    pa = (ctypes.c_void_p * k)(*[a.ptr for a in accs])
    pg = (ctypes.c_void_p * k)(*[g.ptr for g in grads])
    cn = (ctypes.c_long * k)(*(counts if counts is not None else [a.n for a in accs]))
    L.call("umpr_grad_accumulate", ctypes.addressof(pa), ctypes.addressof(pg), ctypes.addressof(cn), len(accs), first, st())


@pytest.mark.parametrize("n", SIZES)
def test_kernel_equals_float32_addition_bit_for_bit(L, dev, pool, n):
    """first = 1 onto a NaN-filled acc, then first = 0 twice: acc is (g1 + g2) + g3 in np.float32, bit for bit, the gradients
    and every guard band are untouched - with acc and the gradients on 16-byte boundaries, both one float behind one (the
    float4 path with a head and a tail), and one of them only (the path that goes element by element)"""
    with np.errstate(invalid="ignore", over="ignore"):
        want = [pool[0][:n], pool[0][:n] + pool[1][:n], (pool[0][:n] + pool[1][:n]) + pool[2][:n]]
    assert want[2].dtype == np.float32
    if n > 19:
        assert np.signbit(want[2][7]) and want[2][7] == 0 and not np.signbit(want[2][13]) and want[2][13] == 0
        assert np.isinf(want[2][2]) and np.isfinite(want[2][3:]).all()
    for off_acc, off_g in ((0, 0), (1, 1), (0, 1), (1, 0)):
        what = f"n={n} acc+{off_acc} g+{off_g}"
        acc = _Buf(np.full(n, np.nan, np.float32), off_acc, dev)
        gs = [_Buf(pool[j][:n], off_g, dev) for j in range(3)]
        for j in range(3):
            _accumulate(L, [acc], [gs[j]], int(j == 0))
            acc.check(want[j], f"{what} after micro-batch {j + 1}")
        for j in range(3):
            gs[j].check(pool[j][:n], f"{what} gradient {j + 1}")


def test_kernel_three_arenas_with_an_empty_one_in_the_middle(L, dev, pool):
    sizes, offs = (1025, 0, 257), (0, 0, 1)
    lo = (0, 5000, 9000)
    accs = [_Buf(np.full(n, np.nan, np.float32), o, dev) for n, o in zip(sizes, offs)]
    gs = [[_Buf(pool[j][s:s + n], o, dev) for n, o, s in zip(sizes, offs, lo)] for j in range(3)]
    for j in range(3):
        _accumulate(L, accs, gs[j], int(j == 0))
    for a, (n, s) in enumerate(zip(sizes, lo)):
        with np.errstate(invalid="ignore"):
            accs[a].check((pool[0][s:s + n] + pool[1][s:s + n]) + pool[2][s:s + n], f"arena {a}")
        for j in range(3):
            gs[j][a].check(pool[j][s:s + n], f"arena {a} gradient {j + 1}")
    # a table of nothing, and a table whose counts are all zero, are successful no-ops
    _accumulate(L, [], [], 1)
    _accumulate(L, accs, gs[0], 1, counts=[0, 0, 0])
    with np.errstate(invalid="ignore"):
        accs[0].check((pool[0][:1025] + pool[1][:1025]) + pool[2][:1025], "after the no-ops")


def test_kernel_refusals_leave_everything_untouched(L, dev, pool):
    from umpr_amd._lib import UmprHipError
    acc, g = _Buf(np.full(100, np.nan, np.float32), 0, dev), _Buf(pool[0][:100], 0, dev)
    pa, pg = (ctypes.c_void_p * 1)(acc.ptr), (ctypes.c_void_p * 1)(g.ptr)
    null, cn, neg = (ctypes.c_void_p * 1)(None), (ctypes.c_long * 1)(100), (ctypes.c_long * 1)(-1)
    A = ctypes.addressof
    for args, text in (((None, A(pg), A(cn), 1), "null arena table"), ((A(pa), None, A(cn), 1), "null arena table"),
                       ((A(pa), A(pg), None, 1), "null arena table"), ((A(null), A(pg), A(cn), 1), "bad pointer / count"),
                       ((A(pa), A(null), A(cn), 1), "bad pointer / count"), ((A(pa), A(pg), A(cn), 9), "arenas outside 0..8"),
                       ((A(pa), A(pg), A(cn), -1), "arenas outside 0..8"),
                       ((A(pa), A(pg), A(neg), 1), "bad pointer / count")):
        for first in (0, 1):
            with pytest.raises(UmprHipError, match=text):
                L.call("umpr_grad_accumulate", *args, first, st())
    acc.check(np.full(100, np.nan, np.float32), "acc after the refusals")
    g.check(pool[0][:100], "gradient after the refusals")


# ------------------------------------------------------------------------------------------------ the optimiser on UMPR-R
def _umpr_r(dev):
    from umpr_amd.model import UMPR
    from umpr_amd.synthetic import make_param_state
    P = make_param_state(31, 50, 1000, 1, True, m_scale=0.05)
    model = UMPR(_cfg(review_net_only=True), P["embedding.weight"].numpy())
    model.load_state_dict(P)
    return model.to(dev)


def _fresh_r(dev, **kw):
    from umpr_amd.optim import FusedAdam
    model = _umpr_r(dev)
    return model, FusedAdam(model, 1e-3, 1e-3, **kw)


def _host(arenas):
    return [a.detach().cpu().numpy().copy() for a in arenas]


def _chain(copies):
    """acc = g_1, then acc = acc + g_2, ...: np.float32, in micro-batch order"""
    total = [c.copy() for c in copies[0]]
    for c in copies[1:]:
        total = [t + x for t, x in zip(total, c)]
    assert all(t.dtype == np.float32 for t in total)
    return total


def _load(opt, total):
    """hand an optimiser the gradient `total` as if one backward had left it in the arenas"""
    for a, t in zip(opt.grad_arenas(), total):
        a.copy_(torch.from_numpy(t))
    for g in opt.groups:
        for p in g.direct:
            p._umpr_fresh = False


def _snap(opt):
    return [t.clone() for g in opt.groups for t in (g.p, g.m, g.v)]


def _same(a, b):
    return len(a) == len(b) and all(torch.equal(x, y) for x, y in zip(a, b))


def _group(model, opt, batches):
    """one optimiser step over `batches` through train_step; the gradient arenas behind every backward, on the host"""
    from umpr_amd.train import train_step
    copies = []
    for j, b in enumerate(batches):
        train_step(model, opt, b, update=j == len(batches) - 1)
        assert opt.pending == (j + 1 if j < len(batches) - 1 else 0)
        copies.append(_host(opt.grad_arenas()))       # (neither accumulate() nor step() writes the gradient arenas)
    return copies


@pytest.fixture(scope="module")
def micro():
    from umpr_amd.synthetic import make_batch
    return [make_batch(700 + j, B, 1000, review_net_only=True) for j, B in enumerate((3, 4, 2, 4, 3, 4))]


def test_umpr_r_group_of_three_equals_a_step_on_the_chained_sum(dev, micro):
    from umpr_amd.train import train_step
    model, opt = _fresh_r(dev)
    twin_model, twin = _fresh_r(dev)
    assert opt.accum_arenas() is None
    start = _snap(opt)
    copies = _group(model, opt, micro[:3])
    assert not any(np.array_equal(a, b) for a, b in zip(copies[0], copies[1]))
    total = _chain(copies)
    for a, t in zip(opt.accum_arenas(), total):
        assert _bits(a.cpu().numpy()).tobytes() == _bits(t).tobytes()
    assert opt.pending == 0 and opt.step_count == 1
    _load(twin, total)
    twin.step(grad_scale=1 / 3)
    assert _same(_snap(opt), _snap(twin)) and not _same(_snap(opt), start)
    # and the plain step that follows is the plain step: nothing of the group is left behind
    train_step(model, opt, micro[3])
    train_step(twin_model, twin, micro[3])
    assert opt.pending == 0 and opt.step_count == 2 and twin.accum_arenas() is None
    assert _same(_snap(opt), _snap(twin))


def test_umpr_r_accumulation_with_clipping_and_a_skipped_group(dev, micro):
    """the norm is that of the mean gradient; an inf in one micro-batch skips that one optimiser step, and the next group
    overwrites what it left in the accumulation arenas"""
    from umpr_amd.streams import wait_for_gradients
    max_norm = 3.0
    model, opt = _fresh_r(dev, max_grad_norm=max_norm)
    twin_model, twin = _fresh_r(dev, max_grad_norm=max_norm)
    total = _chain(_group(model, opt, micro[:3]))
    stats = opt.clip_stats()
    ref = math.sqrt(sum(float(np.sum((t.astype(np.float64) / 3.0) ** 2)) for t in total))
    print(f"norm {stats['norm']!r} float64 norm of sum / 3 {ref!r} coef {stats['coef']!r}")
    assert abs(stats["norm"] - ref) <= 1e-3 * ref, (stats, ref)
    coef = min(1.0, max_norm / (float(np.float32(stats["norm"])) + 1e-6))
    assert abs(stats["coef"] - coef) <= 2 * float(np.spacing(np.float32(coef))) and stats["seen"] == 1 and stats["skipped"] == 0
    _load(twin, total)
    twin.step(grad_scale=1 / 3)
    assert twin.clip_stats() == stats and _same(_snap(opt), _snap(twin))
    # a group whose second micro-batch carries an inf (written into the arena between backward and accumulate())
    before = _snap(opt)
    for j, b in enumerate(micro[:2]):
        model.train()
        _, loss = model(*b)
        opt.zero_grad()
        loss.backward()
        if j == 1:
            wait_for_gradients(dev)
            opt.groups[0].g[12345] = float("inf")
        opt.accumulate()
    assert opt.pending == 2
    opt.step()
    stats = opt.clip_stats()
    assert stats["skipped"] == 1 and stats["seen"] == 2 and stats["coef"] == 0.0 and opt.pending == 0 and opt.step_count == 2
    assert _same(before, _snap(opt))
    assert not torch.isfinite(opt.accum_arenas()[0]).all()           # the inf is still in there ...
    twin.step_count += 1                                             # (a skipped step counts: the bias corrections are host values)
    _group(model, opt, micro[3:5])                                   # ... and the next group never reads it
    _group(twin_model, twin, micro[3:5])
    stats = opt.clip_stats()
    assert stats["skipped"] == 1 and stats["seen"] == 3 and math.isfinite(stats["norm"]) and stats["coef"] > 0.0
    assert stats["norm"] == twin.clip_stats()["norm"] and stats["coef"] == twin.clip_stats()["coef"]
    assert _same(_snap(opt), _snap(twin)) and not _same(before, _snap(opt))


# ------------------------------------------------------------------------------------------------ the full model
@pytest.fixture(scope="module")
def full_state():
    from umpr_amd.synthetic import make_batch, make_param_state
    return make_param_state(121, 50, 500, 1, False, m_scale=0.05), [make_batch(130, 2, 500, 1), make_batch(131, 1, 500, 1)]


@pytest.mark.parametrize("variant", ["fp32", "fp32_freeze_conv", "bf16"])
def test_full_model_group_of_two_equals_a_step_on_the_chained_sum(dev, full_state, variant):
    """V = 1, micro-batches of 2 and 1 samples: direct parameters no backward node wrote, the gradients the weight-gradient
    stream writes and the classifier slice (no early update while accumulating) all reach the accumulation arenas"""
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    P, batches = full_state
    cfg = _cfg(views=["unknown"], dtype="bf16" if variant == "bf16" else "fp32", freeze_conv=variant == "fp32_freeze_conv")
    model = UMPR(cfg, P["embedding.weight"].numpy())
    model.load_state_dict(P)
    model = model.to(dev)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}

    def restart():
        torch.manual_seed(5)
        model.load_state_dict(start)
        for m in model.modules():
            if hasattr(m, "_calls"):
                m._calls = 0
        return FusedAdam(model, 1e-3, 1e-3)

    opt = restart()
    assert opt.early_bucket() is not None
    seen, step = [], opt.step
    opt.step = lambda *a, **kw: (seen.append((opt._early, opt._early_done, opt.pending)), step(*a, **kw))[1]
    total = _chain(_group(model, opt, batches))
    assert seen == [(None, None, 2)]                  # one step, of two micro-batches, and nothing was updated early
    for a, t in zip(opt.accum_arenas(), total):
        assert _bits(a.cpu().numpy()).tobytes() == _bits(t).tobytes()
    assert all(np.isfinite(t).all() and np.any(t) for t in total)
    got = _snap(opt)
    del opt
    twin = restart()
    before = _snap(twin)
    _load(twin, total)
    twin.step(grad_scale=1 / 2)
    assert _same(got, _snap(twin)) and not _same(got, before)


# ------------------------------------------------------------------------------------------------ against the oracle
def _worst_ratio(model, g):
    """max over the compared elements of |p - oracle| / (2e-5 + 1e-4 |oracle|): test_gpu_grad_clip._worst_ratio's rule"""
    worst = {}
    for k, p in model.named_parameters():
        if not p.requires_grad:
            continue
        ref = torch.from_numpy(g["param/" + k])
        mask = torch.from_numpy(np.unpackbits(g["mask/" + k])[:ref.numel()].astype(bool)).view(ref.shape)
        assert mask.any(), k
        d = (p.detach().cpu() - ref).abs() / (2e-5 + 1e-4 * ref.abs())
        worst[k] = float(d[mask].max())
    return worst


def test_accumulated_trajectory_vs_oracle(dev):
    """Four optimiser steps of two micro-batches (4 and 3 samples) at lr 1e-3, l2 1e-3, max_norm 5.6936 against the oracle driven
    with (loss / 2).backward() twice, clip_grad_norm_ and torch.optim.Adam: steps 3 and 4 clip."""
    from umpr_amd.synthetic import make_batch
    from umpr_amd.train import train_step
    g = load_golden("grad_accum_umpr_r")
    assert np.allclose(g["norms_unclipped"], [4.8565, 4.5183, 7.7015, 6.5307], rtol=0, atol=5e-4)
    max_norm = float(g["max_norm"])
    assert max_norm == 5.6936 and min(abs(x / max_norm - 1) for x in g["norms_clipped"]) > 0.09
    assert [x > max_norm for x in g["norms_clipped"]] == [False, False, True, True]
    # each of the wrong implementations the oracle ran ends far outside the tolerance: passing means none of them is at work
    for mutant in ("sum", "last", "every", "noclip"):
        assert float(g["separation/" + mutant]) > 10, mutant
    model, opt = _fresh_r(dev, max_grad_norm=max_norm)
    assert float(g["lr"]) == 1e-3 and float(g["l2"]) == 1e-3
    for s in range(4):
        for j in range(2):
            train_step(model, opt, make_batch(500 + 2 * s + j, 4 if j == 0 else 3, 1000, review_net_only=True), update=j == 1)
        stats = opt.clip_stats()
        ref = float(g["norms_clipped"][s])
        print(f"step {s + 1}: norm {stats['norm']:.6f} oracle {ref:.6f} coef {stats['coef']:.6f}")
        assert abs(stats["norm"] - ref) <= 1e-3 * ref, (s, stats, ref)
        assert (stats["coef"] < 1.0) == (ref > max_norm), (s, stats)
    assert stats["clipped"] == 2 and stats["skipped"] == 0 and stats["seen"] == 4 and opt.step_count == 4
    worst = _worst_ratio(model, g)
    print("accumulated run, error / tolerance:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ resume
def test_resume_inside_an_accumulated_epoch_is_exact(dev, tmp_path):
    """k = 2 over 5 batches per epoch: optimiser steps behind batches 2 and 4 and one on the fifth alone.  A run stopped after
    its first epoch left its checkpoint behind the second step (4 batches in); resumed in a fresh model it re-forms the tail
    group and the second epoch's groups, and ends on the bits of the uninterrupted run."""
    from torch.utils.data import DataLoader
    from umpr_amd.checkpoint import load_checkpoint
    from umpr_amd.config import Config
    from umpr_amd.model import UMPR
    from umpr_amd.synthetic import make_batch, make_param_state
    from umpr_amd.train import training
    P = make_param_state(181, 50, 300, 1, True, m_scale=0.05)
    samples = [make_batch(190 + i, 2 + i % 2, 300, review_net_only=True, max_sent_count=6, min_sent_count=6, full_pad=True)
               for i in range(5)]

    def run(resume, path, epochs):
        cfg = _cfg(review_net_only=True, train_epochs=epochs, learning_rate=1e-3, lr_decay=0.5, valid_every=2, resume=resume,
                   accum_steps=2, grad_clip=0.0)
        torch.manual_seed(11)
        m = UMPR(cfg, P["embedding.weight"].numpy())
        m.load_state_dict(P)
        m = m.to(dev)
        gen = torch.Generator().manual_seed(0)
        train = DataLoader(samples, batch_size=None, shuffle=True, generator=gen)   # each "sample" is a collated batch
        lines = []
        opt, saved = training(train, [samples[0]], m, cfg, path, logger=type("L", (), {"info": staticmethod(lines.append)}))
        return m, opt, saved, lines

    full, full_opt, _, _ = run("", str(tmp_path / "full.pt"), 2)
    assert full_opt.step_count == 6 and full_opt.pending == 0
    part, part_opt, saved, _ = run("", str(tmp_path / "part.pt"), 1)
    assert saved and part_opt.step_count == 3
    meta = load_checkpoint(str(tmp_path / "part.pt"), part, map_location=dev)
    assert meta["epoch"] == 0 and meta["batch_counter"] == 2 and meta["batch_in_epoch"] == 4
    res, res_opt, _, lines = run(str(tmp_path / "part.pt"), str(tmp_path / "res.pt"), 2)
    assert any(ln.startswith("Resumed from") for ln in lines)
    assert res_opt.step_count == 6 and res_opt.pending == 0
    for (k, a), (_, c) in zip(full.state_dict().items(), res.state_dict().items()):
        assert torch.equal(a, c), k
    assert _same(_snap(full_opt), _snap(res_opt))


# ------------------------------------------------------------------------------------------------ k = 1
def test_without_accumulation_the_trajectory_and_the_allocations_are_the_old_ones(dev):
    """train_step(update=True) with nothing pending is the plain step: the Adam trajectory fixture (adam_umpr_r) at its own
    tolerances, and no accumulation arena is ever allocated"""
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_batch
    from umpr_amd.train import train_step
    g = load_golden("adam_umpr_r")
    model = _umpr_r(dev)
    opt = FusedAdam(model, float(g["lr"]), float(g["l2"]), lr_decay=0.99)
    twin_model = _umpr_r(dev)
    twin = FusedAdam(twin_model, float(g["lr"]), float(g["l2"]), lr_decay=0.99)
    for step in range(3):
        batch = make_batch(500 + step, 4, 1000, review_net_only=True)
        _, loss = train_step(model, opt, batch, update=True)
        train_step(twin_model, twin, batch)
        assert abs(loss.item() - g["losses"][step]) < 1e-4
        assert opt.pending == 0 and opt.accum_arenas() is None and opt._acc is None
        if step == 0:
            opt.epoch_end()
            twin.epoch_end()
    for k, p in model.named_parameters():
        if "param/" + k in g:
            ref = torch.from_numpy(np.asarray(g["param/" + k]))
            assert torch.allclose(p.detach().cpu(), ref, atol=2e-5, rtol=1e-4), k
    assert _same(_snap(opt), _snap(twin))
