"""`--sparse_embedding True` on the GPU: umpr_embed_grad_rows against umpr_embed_grad (bit-equal run sums, -1 / +0.0 everywhere else),
umpr_sparse_adam_rows against the float64 row update of tests/sparse_adam_reference.py, the model with the option on against the
dense model, four train_steps against the oracle with torch.optim.SparseAdam on the table, the checkpoint round trip, the refusals
and the CLI.

Conventions of tests/test_gpu_embed_grad.py: every output is prefilled with a sentinel and followed by a guard band that must come
back untouched, the workspace is exactly the queried size behind a guard band, and the gate is the project's own
(coattn_decisions.gate: a HIP tensor may be K = 4 x as far from float64 as the float32 CPU evaluation of the same formula, floor 2^-22).
"""
import ctypes
import os
import shutil
import sys

import numpy as np
import pytest
import torch

import embed_grad_reference as EG
import sparse_adam_reference as SA
from test_gpu_embed_grad import (GUARD, SENTINEL, VOCAB, _calls, _chunk, _make, _model, _scatter, _sentinel, _small_batches,
                                 _trajectory_check, log)
from test_gpu_parity import L, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

ID_SENTINEL = -0x123456789ABCDEF
ES = [1, 49, 50, 300]


def _sizes(L):
    c = _chunk(L)
    return [0, 1, c - 1, c, c + 1, 2 * c, 2 * c + 77]


# ------------------------------------------------------------------------------------------------ umpr_embed_grad_rows
def _rows(L, dev, sources, vocab, E, stream=None):
    """umpr_embed_grad_rows on the device, as test_gpu_embed_grad._scatter calls umpr_embed_grad: row_id / row_grad are
    sentinel-filled with guard bands, the workspace is exactly umpr_embed_grad_rows_ws_bytes long, NaN bytes, with a guard band.
    Returns (row_id int64 [T], row_grad int32 bits [T][E]) on the CPU."""
    ids = [torch.from_numpy(np.ascontiguousarray(i, dtype=np.int64)).to(dev) for i, _ in sources]
    dxs = [torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).reshape(-1, E).to(dev) for _, d in sources]
    T = sum(int(i.numel()) for i in ids)
    pos = torch.sort(torch.cat(ids), stable=True).indices.to(torch.int32) if T else torch.zeros(1, dtype=torch.int32, device=dev)
    row_id = torch.full((T + GUARD,), ID_SENTINEL, dtype=torch.int64, device=dev)
    bits, row_grad = _sentinel(dev, T * E)
    wsb = L.size("umpr_embed_grad_rows_ws_bytes", T, E)
    ws = torch.full((wsb + 4 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    k = max(len(ids), 1)
    iarr = (ctypes.c_void_p * k)(*[t.data_ptr() for t in ids])
    darr = (ctypes.c_void_p * k)(*[t.data_ptr() for t in dxs])
    counts = (ctypes.c_long * k)(*[int(t.numel()) for t in ids])
    args = (ctypes.addressof(iarr), ctypes.addressof(darr), ctypes.addressof(counts), len(ids), E, vocab, pos, row_id, row_grad, ws,
            wsb)
    if stream is None:
        L.call("umpr_embed_grad_rows", *args, st())
    else:
        with torch.cuda.stream(stream):
            L.call("umpr_embed_grad_rows", *args, stream.cuda_stream)
    torch.cuda.synchronize()
    assert bool((bits[T * E:] == SENTINEL).all()) and bool((row_id[T:] == ID_SENTINEL).all()), "written behind row_grad / row_id"
    assert bool((ws[wsb:] == 0xFF).all()), "written behind ws_bytes"
    return row_id[:T].cpu(), bits[:T * E].cpu().view(T, E)


def _judge_rows(tag, L, dev, sources, vocab, E):
    """every run start carries its id and the dense table's row to the bit; every other position -1 and +0.0; no sentinel left"""
    row_id, bits = _rows(L, dev, sources, vocab, E)
    dense = _scatter(L, dev, sources, vocab, E)
    flat = np.concatenate([np.asarray(i, dtype=np.int64).reshape(-1) for i, _ in sources]) if sources else np.zeros(0, np.int64)
    keys = flat[EG.sorted_positions([i for i, _ in sources])]
    T = keys.size
    begins = np.ones(T, dtype=bool)
    begins[1:] = keys[1:] != keys[:-1]
    begins &= (keys >= 0) & (keys < vocab)
    want_id = torch.from_numpy(np.where(begins, keys, -1))
    assert torch.equal(row_id, want_id), (tag, "row_id")
    b = torch.from_numpy(begins)
    assert bool((bits[~b] == 0).all()), (tag, "a position that begins no run of a table row is not +0.0 in every column")
    assert torch.equal(bits[b], dense[want_id[b]]), (tag, "a run's sum is not bit-equal to the dense table's row")
    assert want_id[b].tolist() == SA.named_rows([i for i, _ in sources], vocab).tolist(), tag
    return row_id, bits


@pytest.mark.parametrize("E", ES)
@pytest.mark.parametrize("pattern", EG.PATTERNS)
def test_rows_vs_dense_table(L, dev, pattern, E):
    for T in _sizes(L):
        ids, dx = _make(pattern, T, E)
        _judge_rows(f"{pattern} T{T} E{E}", L, dev, [(ids, dx)], VOCAB, E)


def test_rows_long_runs_at_every_offset(L, dev):
    """the run lists of test_gpu_embed_grad.test_long_runs_at_every_offset: runs longer than a window that begin anywhere in one"""
    c = _chunk(L)
    for lens in ([c + 1, 3, 2 * c, 2 * c + 5, 1, c, c + 2], [5, 3 * c + 1, c + 1, c + 1, 7], [c - 1, c + 1, c + 1], [4 * c + 3]):
        ids = np.concatenate([np.full(n, 11 * k + (k % 2) * 500, dtype=np.int64) for k, n in enumerate(lens)])
        rng = np.random.default_rng(sum(lens))
        ids = ids[rng.permutation(ids.size)]
        dx = rng.standard_normal((ids.size, 50)).astype(np.float32)
        for E in (50, 300):
            _judge_rows(f"runs {lens} E{E}", L, dev, [(ids, np.ascontiguousarray(np.resize(dx, (ids.size, E))))], VOCAB, E)


@pytest.mark.parametrize("counts", [(1,), (200, 389), (300, 0, 289), (17, 250, 1, 321)], ids=lambda c: "-".join(map(str, c)))
def test_rows_one_to_four_sources_of_unequal_length(L, dev, counts):
    T = sum(counts)
    ids, dx = _make("zipf", T, 50, seed=len(counts))
    row_id, bits = _judge_rows(f"sources {counts}", L, dev, EG.split_sources(ids, dx, counts), VOCAB, 50)
    one_id, one_bits = _rows(L, dev, [(ids, dx)], VOCAB, 50)
    assert torch.equal(row_id, one_id) and torch.equal(bits, one_bits)


def test_rows_ids_outside_the_table(L, dev):
    c = _chunk(L)
    ids, dx = _make("zipf", 600, 50)
    ids[::7] = -5
    ids[2::17] = -2 ** 40
    ids[3::7] = VOCAB
    ids[5::11] = 2 ** 40
    ids[6::13] = VOCAB + 7
    _judge_rows("ids outside", L, dev, [(ids, dx)], VOCAB, 50)
    ids = np.concatenate([np.full(c + 5, -3), np.full(2 * c + 1, VOCAB + 1), np.full(c + 9, 4)]).astype(np.int64)   # long runs outside
    dx = np.random.default_rng(9).standard_normal((ids.size, 300)).astype(np.float32)
    _judge_rows("long runs outside", L, dev, [(ids, dx)], VOCAB, 300)


def test_rows_are_deterministic(L, dev):
    c = _chunk(L)
    ids, dx = _make("zipf", 4 * c + 9, 50)
    src = EG.split_sources(ids, dx, (c, 3 * c + 9))
    first = _rows(L, dev, src, VOCAB, 50)
    side = torch.cuda.Stream(dev)
    a = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            a = a @ a * 1e-3                                      # keeps the stream busy while the call is enqueued behind it
    second = _rows(L, dev, src, VOCAB, 50, stream=side)
    assert torch.equal(first[0], second[0]) and torch.equal(first[1], second[1])


# ------------------------------------------------------------------------------------------------ umpr_sparse_adam_rows
def _one_sign_case(T, E, vocab=VOCAB):
    """ids ("ends": rows 0 and vocab - 1 among them) and dx with ONE sign per (id, column): no row sum cancels"""
    rng = np.random.default_rng(7000 + 10 * T + E)
    ids = EG.make_ids("ends", T, vocab, rng)
    sign = rng.choice(np.array([-1.0, 1.0], dtype=np.float32), size=(vocab, E))
    dx = (np.abs(rng.standard_normal((T, E))) + 0.1).astype(np.float32) * sign[ids]
    src = [(ids, dx)]
    if T:
        total, mags = EG.scatter_reference(src, vocab, E), EG.scatter_reference([(ids, np.abs(dx))], vocab, E)
        rows = SA.named_rows([ids], vocab)
        assert bool((np.abs(total[rows]) > 1e-3 * mags[rows]).all()) and bool((mags[rows] > 0).all())
    return ids, dx


def _row_inputs(L, dev, ids, dx, vocab, E):
    """(rows, their gradient, row_id [T], row_grad [T][E]) built on the HOST from the table umpr_embed_grad writes (which
    tests/test_gpu_embed_grad.py pins) - never from umpr_embed_grad_rows"""
    table = _scatter(L, dev, [(ids, dx)], vocab, E).view(torch.float32).numpy()
    keys = ids[EG.sorted_positions([ids])]
    begins = np.ones(keys.size, dtype=bool)
    begins[1:] = keys[1:] != keys[:-1]
    row_id = np.where(begins, keys, -1).astype(np.int64)
    row_grad = np.zeros((keys.size, E), dtype=np.float32)
    row_grad[begins] = table[keys[begins]]
    return keys[begins], table[keys[begins]], row_id, row_grad


def _banded(dev, values, off):
    """a device copy of `values` based `off` floats into a sentinel-filled allocation with a guard band behind it"""
    n = values.size
    bits, view = _sentinel(dev, n, off)
    view.copy_(torch.from_numpy(np.ascontiguousarray(values, dtype=np.float32)).reshape(-1).to(dev))
    return bits, view


def _adam(L, dev, state0, offs, row_id, row_grad, vocab, E, step, grad_scale, clip=None, T=None):
    """umpr_sparse_adam_rows on fresh banded copies of state0 = (p, m, v); returns the three tables' int32 bits (CPU)"""
    bufs = [_banded(dev, a, o) for a, o in zip(state0, offs)]
    rid = torch.from_numpy(row_id).to(dev) if row_id.size else torch.zeros(1, dtype=torch.int64, device=dev)
    rg = torch.from_numpy(row_grad).to(dev) if row_grad.size else torch.zeros(1, dtype=torch.float32, device=dev)
    cs = None if clip is None else torch.tensor(list(clip) + [0.0] * (8 - len(clip)), dtype=torch.float32, device=dev)
    L.call("umpr_sparse_adam_rows", bufs[0][1], bufs[1][1], bufs[2][1], vocab, E, rid, rg, row_id.size if T is None else T, 1e-3,
           0.9, 0.999, 1e-8, step, grad_scale, cs, st())
    torch.cuda.synchronize()
    out = []
    for (bits, _), o in zip(bufs, offs):
        assert bool((bits[:o] == SENTINEL).all()) and bool((bits[o + vocab * E:] == SENTINEL).all()), "written outside a table"
        out.append(bits[o:o + vocab * E].cpu().view(vocab, E))
    return out


@pytest.mark.parametrize("grad_scale", [1.0, 0.5])
@pytest.mark.parametrize("step", [1, 7])
@pytest.mark.parametrize("E", ES)
def test_sparse_adam_rows_vs_float64(L, dev, E, step, grad_scale):
    for k, T in enumerate(_sizes(L)):
        ids, dx = _one_sign_case(T, E)
        rng = np.random.default_rng(100 * T + E + step)
        state0 = [rng.standard_normal((VOCAB, E)).astype(np.float32), rng.standard_normal((VOCAB, E)).astype(np.float32),
                  rng.random((VOCAB, E)).astype(np.float32)]
        offs = [(0, 1, 3)[(k + i) % 3] for i in range(3)]
        tag = f"adam rows T{T} E{E} step{step} scale{grad_scale} offs{offs}"
        if T == 0:
            got = _adam(L, dev, state0, offs, np.zeros(0, np.int64), np.zeros((0, E), np.float32), VOCAB, E, step, grad_scale)
            assert all(np.array_equal(g.view(torch.float32).numpy(), a) for g, a in zip(got, state0)), tag
            continue
        rows, grad, row_id, row_grad = _row_inputs(L, dev, ids, dx, VOCAB, E)
        if T >= 2:
            assert rows[0] == 0 and rows[-1] == VOCAB - 1
        got = _adam(L, dev, state0, offs, row_id, row_grad, VOCAB, E, step, grad_scale)
        ref = SA.row_update(*state0, rows, grad, step, 1e-3, grad_scale=grad_scale)
        ref32 = SA.row_update(*state0, rows, grad, step, 1e-3, grad_scale=grad_scale, dtype=np.float32)
        out = np.setdiff1d(np.arange(VOCAB), rows)
        for g, a in zip(got, state0):
            assert np.array_equal(g.numpy()[out], a.view(np.int32)[out]), (tag, "a row no position names changed")
        ok, res = EG.gate([g.view(torch.float32)[rows] for g in got], [EG.as_tensor(r[rows]) for r in ref],
                          [EG.as_tensor(r[rows]) for r in ref32], names=["p", "m", "v"], K=EG.K, log=log, tag=tag)
        assert ok, (tag, res)


def test_sparse_adam_rows_clip_state(L, dev):
    """COEF = 1 is bit-equal to NULL, COEF = 0.25 to the call whose grad_scale is the float product, FINITE = 0 changes no byte,
    T = 0 is a no-op"""
    c = _chunk(L)
    E, T = 50, 2 * c + 77
    ids, dx = _one_sign_case(T, E)
    rng = np.random.default_rng(3)
    state0 = [rng.standard_normal((VOCAB, E)).astype(np.float32), rng.standard_normal((VOCAB, E)).astype(np.float32),
              rng.random((VOCAB, E)).astype(np.float32)]
    offs = (1, 0, 3)
    _, _, row_id, row_grad = _row_inputs(L, dev, ids, dx, VOCAB, E)
    run = lambda gs, clip=None, T=None: _adam(L, dev, state0, offs, row_id, row_grad, VOCAB, E, 3, gs, clip, T)   # noqa: E731
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))                                             # noqa: E731
    start = [torch.from_numpy(a.view(np.int32)) for a in state0]
    plain = run(0.3)
    assert not same(plain, start)
    assert same(plain, run(0.3, clip=(1.0, 2.0, 1.0)))
    product = float(np.float32(0.3) * np.float32(0.25))
    quarter = run(0.3, clip=(0.25, 2.0, 1.0))
    assert same(quarter, run(product)) and not same(quarter, plain)
    assert same(start, run(0.3, clip=(0.25, float("inf"), 0.0)))
    assert same(start, run(0.3, T=0))


# ------------------------------------------------------------------------------------------------ the model
MODEL_CASES = {"umpr_r": dict(ronly=True, B=3, kw={}), "full_frozen_vgg_B2": dict(ronly=False, B=2, kw=dict(freeze_vgg=True))}


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_model_sparse_vs_dense(L, dev, name, monkeypatch):
    """pred, loss and every other gradient bit-equal to the dense (train_embedding) model's; sparse_table_grad() has exactly the ids
    the batch names and its rows are the dense gradient's to the bit; embedding.weight.grad stays None; one train_step calls
    umpr_embed_grad_rows once, umpr_sparse_adam_rows once and umpr_embed_grad never.  S = 5, L <= 6."""
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_batch, make_param_state
    from umpr_amd.train import train_step
    mc = MODEL_CASES[name]
    ronly = mc["ronly"]
    P = make_param_state(81, 50, 600, 1, ronly, m_scale=0.05)
    batch = make_batch(82, mc["B"], 600, 1, max_sent_count=5, min_sent_count=5, max_ui_sent_count=2, max_sent_length=6,
                       review_net_only=ronly)
    kw = dict(review_net_only=ronly, views=["unknown"], train_embedding=True, **mc["kw"])
    res = {}
    for sparse in (False, True):
        m = _model(dev, P, sparse_embedding=sparse, **kw).eval()
        assert m.sparse_embedding is sparse and m.embedding.weight.requires_grad
        pred, loss = m(*batch)
        loss.backward()
        torch.cuda.synchronize()
        res[sparse] = (pred.detach().cpu(), loss.detach().cpu(), {k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None},
                       m)
    dense, sp = res[False], res[True]
    assert torch.equal(dense[0], sp[0]) and torch.equal(dense[1], sp[1])
    assert set(dense[2]) == set(sp[2]) | {"embedding.weight"} and sp[3].embedding.weight.grad is None
    for k, g in sp[2].items():
        assert torch.equal(g, dense[2][k]), k
    named = SA.named_rows([t.numpy() for t in (batch[:2] if ronly else batch[:3])], 600)
    grad = sp[3].sparse_table_grad()
    assert grad.is_sparse and grad.is_coalesced() and tuple(grad.shape) == (600, 50)
    assert grad.indices().cpu()[0].tolist() == named.tolist()
    table = dense[2]["embedding.weight"]
    assert torch.equal(grad.values().cpu().view(torch.int32), table[torch.from_numpy(named)].view(torch.int32))
    assert float(table.abs().max()) > 0
    # one optimiser step: the calls, the rows that move
    m = sp[3]
    opt = FusedAdam(m, 1e-3, 1e-3)
    before = m.embedding.weight.detach().cpu().clone()
    names = []
    monkeypatch.setattr(L, "call", _calls(L, names))
    train_step(m, opt, batch)
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert names.count("umpr_embed_grad_rows") == 1 and names.count("umpr_sparse_adam_rows") == 1 and "umpr_embed_grad" not in names
    assert names.index("umpr_sparse_adam_rows") > max(i for i, n in enumerate(names) if n == "umpr_adam_step")
    moved = (m.embedding.weight.detach().cpu() != before).any(1)
    assert moved.any() and set(torch.nonzero(moved).reshape(-1).tolist()) <= set(named.tolist()) and m.embedding.weight.grad is None
    # zero_grad drops the gradient; a step whose backward never reached the table updates no row
    opt.zero_grad()
    assert m.sparse_table_grad() is None
    after = m.embedding.weight.detach().cpu().clone()
    names.clear()
    monkeypatch.setattr(L, "call", _calls(L, names))
    opt.step()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert "umpr_sparse_adam_rows" not in names and torch.equal(m.embedding.weight.detach().cpu(), after)


# ------------------------------------------------------------------------------------------------ Adam steps vs the oracle
def _oracle_steps(P, batches, lr, l2, max_norm=None):
    """n steps of the oracle: torch.optim.Adam in the reference's two groups on everything but the table, torch.optim.SparseAdam on
    the table, fed the oracle's dense table gradient restricted to the ids the batch names as a COO tensor; clip_grad_norm_ over
    all of it when asked (applied while the table's gradient is still dense: the rows left out are exactly zero).  Returns what
    test_gpu_embed_grad._oracle_steps returns."""
    from oracle import umpr_ref as R
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    table = Pr["embedding.weight"]
    opt = R.adam_reference({k: v for k, v in Pr.items() if k != "embedding.weight"}, lr, l2)
    sopt = torch.optim.SparseAdam([table], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    mask = {k: torch.ones_like(v, dtype=torch.bool) for k, v in Pr.items()}
    norms, norms_wo = [], []
    touched = torch.zeros(table.shape[0], dtype=torch.bool)
    for b in batches:
        _, loss = R.umpr_forward(Pr, b, review_net_only=True, aten=True, train=True)
        for p in Pr.values():
            p.grad = None
        loss.backward()
        named = torch.from_numpy(SA.named_rows([b[0].numpy(), b[1].numpy()], table.shape[0]))
        rest = torch.ones(table.shape[0], dtype=torch.bool)
        rest[named] = False
        assert not bool(table.grad[rest].any())
        for k, p in Pr.items():
            big = p.grad.abs() > 1e-4 * p.grad.abs().max()
            if k == "embedding.weight":     # a row with an exactly zero gradient (PAD, or not named) carries no rounding noise
                big |= (p.grad == 0).all(1, keepdim=True).expand_as(big)
            mask[k] &= big
        sq = {k: float(p.grad.double().pow(2).sum()) for k, p in Pr.items()}
        norms.append(sum(sq.values()) ** 0.5)
        norms_wo.append((sum(sq.values()) - sq["embedding.weight"]) ** 0.5)
        touched[named] = True
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(list(Pr.values()), max_norm)
        table.grad = torch.sparse_coo_tensor(named.unsqueeze(0), table.grad[named], tuple(table.shape))
        opt.step()
        sopt.step()
    return {k: v.detach() for k, v in Pr.items()}, mask, norms, norms_wo, touched


@pytest.mark.parametrize("clip", [False, True])
def test_four_train_steps_vs_oracle_with_sparse_adam(dev, clip):
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_param_state
    from umpr_amd.train import train_step
    lr, l2 = 1e-3, 1e-3
    P = make_param_state(31, 50, 1000, 1, True, m_scale=0.05)
    batches = _small_batches(4)
    _, _, free_norms, _, _ = _oracle_steps(P, batches[:1], lr, l2)
    max_norm = 0.5 * free_norms[0] if clip else None            # half the first step's float64 norm: that step clips for certain
    ref, mask, norms, norms_wo, touched = _oracle_steps(P, batches, lr, l2, max_norm)
    model = _model(dev, P, review_net_only=True, train_embedding=True, sparse_embedding=True)
    opt = FusedAdam(model, lr, l2, max_grad_norm=max_norm or 0.0)
    assert all("embedding.weight" not in g.names for g in opt.groups)
    for s, b in enumerate(batches):
        train_step(model, opt, b)
        if clip:
            stats = opt.clip_stats()
            log(f"sparse clip step {s + 1}: norm {stats['norm']:.6f} float64 {norms[s]:.6f} (without the table {norms_wo[s]:.6f})")
            assert abs(stats["norm"] - norms[s]) <= 1e-3 * norms[s], (s, stats, norms[s])
            assert abs(stats["norm"] - norms[s]) < abs(stats["norm"] - norms_wo[s]), "the table's gradient is not in the norm"
            assert (stats["coef"] < 1.0) == (norms[s] > max_norm)
    if clip:
        assert stats["clipped"] >= 1 and stats["skipped"] == 0 and stats["seen"] == 4
    _trajectory_check(model, ref, mask)
    # rows no step named: every byte of the value as it was, moments exactly zero (the dense path moves them by its L2)
    table = model.embedding.weight.detach().cpu()
    _, _, m, v = opt.sparse
    assert (~touched).sum() > 100
    assert torch.equal(table[~touched].view(torch.int32), P["embedding.weight"][~touched].view(torch.int32))
    assert not bool(m.cpu()[~touched].any()) and not bool(v.cpu()[~touched].any())
    assert bool((table[touched] != P["embedding.weight"][touched]).any()) and bool(m.cpu()[touched].any())


def test_checkpoint_round_trip_and_refusal_under_the_other_setting(dev, tmp_path):
    """save after 2 steps, resume, step: bit-equal to 3 uninterrupted steps (parameters and moments, the table's among them);
    resuming under the other --sparse_embedding setting raises before anything is loaded, both ways"""
    from umpr_amd.checkpoint import load_checkpoint, save_checkpoint
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_param_state
    from umpr_amd.train import train_step
    P = make_param_state(101, 50, 500, 1, True, m_scale=0.05)
    batches = _small_batches(3, vocab=500)

    def fresh(sparse=True):
        m = _model(dev, P, review_net_only=True, train_embedding=True, sparse_embedding=sparse)
        return m, FusedAdam(m, 1e-3, 1e-3, lr_decay=0.99)

    m1, o1 = fresh()
    for b in batches:
        train_step(m1, o1, b)
    m2, o2 = fresh()
    for b in batches[:2]:
        train_step(m2, o2, b)
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, m2, o2, epoch=0, batch_counter=2)
    m3, o3 = fresh()
    assert load_checkpoint(path, m3, o3, map_location=dev)["batch_counter"] == 2
    assert torch.equal(o3.sparse[2], o2.sparse[2]) and bool(o3.sparse[3].any())
    train_step(m3, o3, batches[2])
    assert not torch.equal(m1.embedding.weight.cpu(), P["embedding.weight"])
    for (k, a), (_, c) in zip(m1.state_dict().items(), m3.state_dict().items()):
        assert torch.equal(a, c), k
    for ga, gc in zip(o1.groups, o3.groups):
        assert torch.equal(ga.m, gc.m) and torch.equal(ga.v, gc.v)
    assert torch.equal(o1.sparse[2], o3.sparse[2]) and torch.equal(o1.sparse[3], o3.sparse[3])
    m4, o4 = fresh(sparse=False)
    before = {k: v.clone() for k, v in m4.state_dict().items()}
    with pytest.raises(ValueError, match="written with --sparse_embedding True, this run has --sparse_embedding False"):
        load_checkpoint(path, m4, o4, map_location=dev)
    assert all(torch.equal(v, before[k]) for k, v in m4.state_dict().items()) and o4.step_count == 0
    train_step(m4, o4, batches[0])
    dense_path = str(tmp_path / "dense.pt")
    save_checkpoint(dense_path, m4, o4, epoch=0, batch_counter=1)
    m5, o5 = fresh()
    with pytest.raises(ValueError, match="written with --sparse_embedding False, this run has --sparse_embedding True"):
        load_checkpoint(dense_path, m5, o5, map_location=dev)
    assert torch.equal(m5.embedding.weight.cpu(), P["embedding.weight"]) and o5.step_count == 0 and not bool(o5.sparse[2].any())


# ------------------------------------------------------------------------------------------------ refusals, CLI
def test_refusals(dev):
    from umpr_amd.graphs import GraphedTrainStep
    from umpr_amd.optim import FusedAdam
    from umpr_amd.parallel import GradReducer
    from umpr_amd.pretrain import PretrainRNet
    from umpr_amd.synthetic import make_param_state
    from umpr_amd.train import train_step
    P = make_param_state(5, 50, 300, 1, True, m_scale=0.05)
    model = _model(dev, P, review_net_only=True, train_embedding=True, sparse_embedding=True)
    opt = FusedAdam(model, 1e-3, 1e-3)
    batch = _small_batches(1, vocab=300)[0]
    with pytest.raises(NotImplementedError, match="--sparse_embedding runs on one rank only"):
        GradReducer(opt)
    with pytest.raises(NotImplementedError, match="--sparse_embedding runs on one rank only"):
        train_step(model, opt, batch, world=2)
    with pytest.raises(NotImplementedError, match="trainable embedding table"):
        GraphedTrainStep(model, opt, batch)
    assert opt.step_count == 0 and torch.equal(model.embedding.weight.cpu(), P["embedding.weight"])
    w2v = type("W", (), {"embedding": P["embedding.weight"].numpy(), "word_dim": 50})()
    pre = PretrainRNet(w2v, 64)                                   # the pre-training model keeps its table frozen
    assert not pre.embedding.weight.requires_grad and FusedAdam(pre, 1e-3, 1e-3).sparse is None


def test_main_cli_with_both_flags(tmp_path, capsys, monkeypatch):
    """main.py --train_embedding True --sparse_embedding True on the tiny CSV corpus, in-process as tests/test_gpu_e2e.py runs the
    CLI; --sparse_embedding True alone is refused at start-up"""
    import importlib
    corpus = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_corpus")
    d = tmp_path / "music"
    d.mkdir()
    for split in ("train", "valid", "test"):
        shutil.copy(os.path.join(corpus, "train.csv"), d / f"{split}.csv")
    shutil.copy(os.path.join(corpus, "photos.json"), d / "photos.json")
    (d / "photos").mkdir()
    argv = ["main.py", "--data_dir", str(d), "--word2vec_file", os.path.join(corpus, "glove.txt"), "--review_net_only", "True",
            "--train_epochs", "1", "--batch_size", "4", "--max_sent_count", "6", "--min_sent_count", "2", "--max_ui_sent_count", "3",
            "--max_sent_length", "10", "--views", "food", "--learning_rate", "1e-3", "--model_path", str(tmp_path / "m.pt"),
            "--sparse_embedding", "True"]
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main")
    monkeypatch.setattr(sys, "argv", argv)
    with pytest.raises(SystemExit, match="--sparse_embedding needs --train_embedding True"):
        main.main()
    monkeypatch.setattr(sys, "argv", argv + ["--train_embedding", "True"])
    main.main()
    out = capsys.readouterr().out
    assert "Initial validation mse is" in out and "Test end, test mse is" in out, out[-2000:]
    mse = float(out.strip().split("test mse is")[-1])
    assert mse == mse and mse < 100.0
