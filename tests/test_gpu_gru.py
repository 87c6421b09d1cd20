"""Embedding + bidirectional GRU through the stage-level C ABI (umpr_embed_gru_bidir_fwd / _bwd / _bwd_acc) against the float64
recurrence of tests/gru_reference.py.

The GRU takes no discrete decision, so the output, the gate records `saved` and all eight parameter gradients are held
directly to K x the distance the float32 CPU evaluation of the same formulas has from float64 (G.K = 4, never above 14; floor
2^-22) - three to four orders of magnitude below what one lost (sequence, step, unit) element moves
(test_gate_catches_one_dropped_dout_element).  The cases (G.CASES) are the smallest at which the 16-sequence tiles, the padded
embedding pitch and the split-K dW_ih product can go wrong.  Every call runs on NaN-filled out / saved / gradient buffers and a
NaN-filled workspace, and the upstream gradient is NaN past each sequence's length: whatever the kernels read there shows.
Every distance is logged to gru.log beside the parity tests' log.
"""
import os
from types import SimpleNamespace

import pytest
import torch

import gru_reference as G
from test_gpu_parity import LOG as PARITY_LOG
from test_gpu_parity import L, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "gru.log")
H = G.H
_CASES = {}
_ids = lambda s: "-".join(map(str, s))      # noqa: E731


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _i32(t, dev):
    return t.to(torch.int32).to(dev).contiguous()


def _ws(L, dev, case):
    wsb = L.size("umpr_embed_gru_bidir_ws_bytes", case.N, case.L, case.E)
    return _nan(dev, wsb // 4 + 64), wsb


def _hip_forward(L, dev, case, order, dst_row, small_ws=False):
    """umpr_embed_gru_bidir_fwd on NaN-filled out / saved and a NaN-filled workspace.  small_ws: ws_bytes is exactly the gx
    area N * L * 384 floats and saved = NULL (the inference callers' form).  Returns (out, saved) on the device."""
    N, Lm, E = case.N, case.L, case.E
    out = _nan(dev, N, Lm, 2 * H)
    saved = None if small_ws else _nan(dev, 2, N, Lm, 4, H)
    ws, wsb = _ws(L, dev, case)
    if small_ws:
        wsb = N * Lm * 384 * 4
        assert wsb < L.size("umpr_embed_gru_bidir_ws_bytes", N, Lm, E)
    L.call("umpr_embed_gru_bidir_fwd", case.ids.to(dev), case.emb.to(dev), E, *[p.to(dev) for p in case.w],
           _i32(case.lengths, dev), _i32(order, dev), _i32(dst_row, dev), N, Lm, out, saved, ws, wsb, st())
    torch.cuda.synchronize()
    return out, saved


def _hip_backward(L, dev, case, fwd, order, dst_row, dout=None, entry="umpr_embed_gru_bidir_bwd_acc", prefill=None):
    """The backward entry on the HIP forward's own out / saved (NaN past each length).  dout [N][L][128] is given by input row;
    it is handed over at the output rows (row dst_row[n] = dout[n]) with NaN past each length.  The eight gradient buffers are
    NaN-filled, or hold `prefill` with accumulate = 1; the workspace is NaN-filled.  Returns the eight gradients on the CPU."""
    N, Lm, E = case.N, case.L, case.E
    out, saved = fwd
    d = (case.dout if dout is None else dout).clone()
    d[~G.valid(case)] = float("nan")
    dout_hip = _nan(dev, N, Lm, 2 * H)
    dout_hip[dst_row.long().to(dev)] = d.to(dev)
    if prefill is None:
        g = [_nan(dev, *p.shape) for p in case.w]
    else:
        g = [p.to(dev).contiguous() for p in prefill]
    ws, wsb = _ws(L, dev, case)
    head = (case.ids.to(dev), case.emb.to(dev), E, case.w[1].to(dev), case.w[5].to(dev), _i32(case.lengths, dev),
            _i32(order, dev), _i32(dst_row, dev), N, Lm, dout_hip, out, saved, *g)
    if entry == "umpr_embed_gru_bidir_bwd":
        assert prefill is None
        L.call(entry, *head, ws, wsb, st())
    else:
        L.call(entry, *head, 0 if prefill is None else 1, ws, wsb, st())
    torch.cuda.synchronize()
    return [t.cpu() for t in g]


def _case(L, dev, shape, case=None):
    """One case: its float64 reference and float32 yardstick, and the HIP forward with order = dst_row = sorted_indices.
    Computed once per shape and shared by the tests; nothing in it is modified afterwards."""
    if shape in _CASES:
        return _CASES[shape]
    from umpr_amd.model import UMPR
    case = G.make_case(*shape) if case is None else case
    c = SimpleNamespace(case=case, tag=case.tag, ref=G.reference(case), ref32=G.reference(case, torch.float32), g0=None)
    _, order = UMPR._host_perm(case.lengths, dev)
    c.order = order.cpu().long()
    assert torch.equal(c.order, G.sorted_order(case))
    c.fwd = _hip_forward(L, dev, case, c.order, c.order)
    c.out, c.saved = c.fwd[0].cpu(), c.fwd[1].cpu()
    c.rows = c.out[c.order]                              # rows[n] = out[order[n]] = sequence n
    _CASES[shape] = c
    return c


def _g0(L, dev, c):
    """the eight gradients of _bwd_acc(accumulate = 0) on the case's forward, once"""
    if c.g0 is None:
        c.g0 = _hip_backward(L, dev, c.case, c.fwd, c.order, c.order)
    return c.g0


def _grads(ref):
    return [ref.grads[n] for n in G.GRADS]


def _assert_gate(c, tag, got, ref, ref32, names=G.GRADS):
    ok, rows = G.gate(got, ref, ref32, names=names, K=G.K, log=log, tag=f"{c.tag} {tag}")
    assert ok, [(r["name"], r["d_max"], r["d_l2"], r["r_max"], r["r_l2"], r["ratio"]) for r in rows if not r["ok"]]


def _assert_out(c, tag, rows, ref=None, ref32=None):
    """rows [N][L][128] in input-row order: nothing NaN, exactly 0.0 at t >= min(len, L), under the gate as max abs distance"""
    assert not bool(torch.isnan(rows).any()), f"{c.tag} {tag}: NaN in out"
    m = G.valid(c.case)
    assert bool((rows[~m] == 0).all()), f"{c.tag} {tag}: out is not zero past a length"
    row = G.gate_abs(rows, c.ref.out if ref is None else ref, c.ref32.out if ref32 is None else ref32, "out", K=G.K, log=log,
                     tag=f"{c.tag} {tag}")
    assert row["ok"], row


@pytest.mark.parametrize("shape", G.CASES, ids=_ids)
def test_forward(L, dev, shape):
    """order = dst_row = sorted_indices (UMPR._host_perm): out[order[n]] is sequence n under the gate, exactly zero at every
    t >= min(len, L) - a length of 0 gives an all-zero row, a length above L counts as L - and nothing is left NaN."""
    c = _case(L, dev, shape)
    _assert_out(c, "forward", c.rows)


@pytest.mark.parametrize("shape", G.CASES, ids=_ids)
def test_gate_records(L, dev, shape):
    """saved[d][n][t] (r, z, n, W_hn h + b_hn), indexed by INPUT row n, against the reference's records at t < min(len, L),
    per direction and component.  Positions past the length are not inspected (they still hold the NaN prefill)."""
    c = _case(L, dev, shape)
    m = G.valid(c.case)
    names = [f"saved {q}{s}" for s in ("_f", "_r") for q in ("r", "z", "n", "hn")]
    pick = lambda t: [t[d][m][:, q] for d in range(2) for q in range(4)]      # noqa: E731
    got = pick(c.saved)
    if not bool(m.any()):
        pytest.fail("case without a valid position")
    assert all(bool(torch.isfinite(g).all()) for g in got)
    _assert_gate(c, "records", got, pick(c.ref.gates), pick(c.ref32.gates), names=names)


@pytest.mark.parametrize("shape", G.CASES, ids=_ids)
def test_backward(L, dev, shape):
    """accumulate = 0 on the HIP forward's own out / saved, which still hold NaN past each length: all eight gradients finite
    and under the gate against backward64; dW_hh exactly zero where no sequence has a second step; and
    umpr_embed_gru_bidir_bwd bit-equal to _bwd_acc(accumulate = 0)."""
    c = _case(L, dev, shape)
    assert bool(torch.isnan(c.saved[:, ~G.valid(c.case)]).all())
    g0 = _g0(L, dev, c)
    for name, g in zip(G.GRADS, g0):
        assert bool(torch.isfinite(g).all()), (c.tag, name)
    _assert_gate(c, "backward", g0, _grads(c.ref), _grads(c.ref32))
    if G.whh_is_zero(c.case):
        for i in (1, 5):
            assert float(c.ref.grads[G.GRADS[i]].abs().max()) == 0 and bool((g0[i] == 0).all()), G.GRADS[i]
    else:
        assert all(float(t.abs().max()) > 0 for t in _grads(c.ref))
    plain = _hip_backward(L, dev, c.case, c.fwd, c.order, c.order, entry="umpr_embed_gru_bidir_bwd")
    for name, a, b in zip(G.GRADS, plain, g0):
        assert torch.equal(a, b), (c.tag, name)


@pytest.mark.parametrize("shape", G.CASES, ids=_ids)
def test_accumulate(L, dev, shape):
    """accumulate = 1 onto a seeded finite prefill p (randn) of the eight buffers: bit-equal to the float32 sum p + g0 with g0
    of test_backward - both reduction epilogues (colsum_rows_kernel, unstack_dwih_kernel) compute dst + v with the same v."""
    c = _case(L, dev, shape)
    g0 = _g0(L, dev, c)
    g = torch.Generator().manual_seed(4242 + c.case.N)
    pre = [torch.randn(p.shape, generator=g) for p in c.case.w]
    got = _hip_backward(L, dev, c.case, c.fwd, c.order, c.order, prefill=pre)
    for name, a, p, v in zip(G.GRADS, got, pre, g0):
        assert torch.equal(a, p + v), (c.tag, name, float((a - (p + v)).abs().max()))


@pytest.mark.parametrize("combo", ["sorted_to_identity", "identity_to_random"])
@pytest.mark.parametrize("shape", [(17, 6, 7, "zeros"), (33, 9, 50, "tail1")], ids=_ids)
def test_permutations(L, dev, shape, combo):
    """dst_row distinct from order.  sorted_to_identity: order = sorted_indices, dst_row = identity.  identity_to_random:
    order = identity (tiles of unsorted lengths), dst_row = a seeded random permutation.  Row dst_row[n] of out - and the
    records saved[:, n] - are bit-equal to sequence n of test_forward (a sequence does not depend on its tile's grouping),
    and the gradients are under the gate: dout is read at dst_row."""
    c = _case(L, dev, shape)
    N = c.case.N
    ident = torch.arange(N)
    if combo == "sorted_to_identity":
        order, dst = c.order, ident
    else:
        order, dst = ident, torch.randperm(N, generator=torch.Generator().manual_seed(N))
        assert not torch.equal(dst, ident) and not torch.equal(dst, c.order)
    fwd = _hip_forward(L, dev, c.case, order, dst)
    rows = fwd[0].cpu()[dst]
    assert torch.equal(rows, c.rows), f"{c.tag} {combo}: out depends on order / dst_row"
    m = G.valid(c.case)
    assert torch.equal(fwd[1].cpu()[:, m], c.saved[:, m]), f"{c.tag} {combo}: saved depends on order / dst_row"
    got = _hip_backward(L, dev, c.case, fwd, order, dst)
    _assert_gate(c, combo, got, _grads(c.ref), _grads(c.ref32))


def test_pair_form(L, dev):
    """Two review tensors of 9 sequences on one GRU as ONE batch of 18 (UMPR._pair): lengths and sorted indices per half, the
    item half's order offset by N.  The forward is bit-equal to the two separate calls; the gradients are under the gate
    against the float64 sum of both halves' gradients."""
    n, Lm, E = 9, 6, 7
    a = G.make_case(n, Lm, E, "rand", seed=61)
    b = G.make_case(n, Lm, E, "tail1", seed=62)
    b.emb, b.w = a.emb, a.w
    b.x = torch.nn.functional.embedding(b.ids, b.emb)
    ca, cb = _case(L, dev, ("pair u",), a), _case(L, dev, ("pair i",), b)
    both = SimpleNamespace(N=2 * n, L=Lm, E=E, emb=a.emb, w=a.w, ids=torch.cat([a.ids, b.ids]), tag="pair 2x9 L6 E7",
                           lengths=torch.cat([a.lengths, b.lengths]), dout=torch.cat([a.dout, b.dout]))
    order = torch.cat([ca.order, cb.order + n])
    fwd = _hip_forward(L, dev, both, order, order)
    out = fwd[0].cpu()
    assert torch.equal(out[:n], ca.out) and torch.equal(out[n:], cb.out), "the pair's forward differs from two separate calls"
    assert not bool(torch.isnan(out).any())
    got = _hip_backward(L, dev, both, fwd, order, order)
    ref = [x + y for x, y in zip(_grads(ca.ref), _grads(cb.ref))]
    ref32 = [x + y for x, y in zip(_grads(ca.ref32), _grads(cb.ref32))]
    _assert_gate(SimpleNamespace(tag=both.tag), "pair", got, ref, ref32)


@pytest.mark.parametrize("shape", [(17, 6, 7, "zeros"), (15, 5, 3, "rand")], ids=_ids)
def test_small_workspace_forward(L, dev, shape):
    """ws_bytes = N * L * 384 * 4 exactly and saved = NULL: one gather-GEMM per direction with an unpadded K = E, on a
    NaN-filled workspace.  Held to float64 like the stacked path, not bit-compared with it."""
    c = _case(L, dev, shape)
    out, saved = _hip_forward(L, dev, c.case, c.order, c.order, small_ws=True)
    assert saved is None
    _assert_out(c, "small workspace", out.cpu()[c.order])


def test_gate_catches_one_dropped_dout_element(L, dev):
    """(33, 9, 50): ONE element of dout - last sequence (length 1, alone in the third tile), t = 0, one reverse-direction unit -
    is zeroed and the HIP backward runs on it: the gate against the unaltered reference fails, at 10x the bound or more; the
    forward direction's four gradients, which that element cannot reach, stay bit-equal."""
    c = _case(L, dev, (33, 9, 50, "tail1"))
    g0 = _g0(L, dev, c)
    n, t, col = G.dropped_dout_element(c.case)
    assert col >= H and abs(float(c.case.dout[n, t, col])) >= 0.5
    dout = c.case.dout.clone()
    dout[n, t, col] = 0
    got = _hip_backward(L, dev, c.case, c.fwd, c.order, c.order, dout=dout)
    ok, rows = G.gate(got, _grads(c.ref), _grads(c.ref32), names=G.GRADS, K=G.K, log=log,
                      tag=f"{c.tag} dout[{n}][{t}][{col}] dropped")
    log(f"{c.tag} one dropped dout element: distance / bound = " + ", ".join(f"{r['name']} {r['over']:.1f}x" for r in rows))
    assert not ok
    assert max(r["over"] for r in rows) >= 10, [(r["name"], r["over"]) for r in rows]
    for name, x, y in zip(G.GRADS[:4], got[:4], g0[:4]):
        assert torch.equal(x, y), name
