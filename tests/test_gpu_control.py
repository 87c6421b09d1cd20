"""The control network through the stage-level C ABI (umpr_cnet_head_fwd / _bwd, umpr_control_gate_fwd / _bwd, umpr_snet_fwd /
_bwd) and the fused entries umpr_control_net_fwd / _bwd, against the decision-conditioned float64 reference of
tests/control_decisions.py.

Every saved tensor of the head forward (Y, cmax, argl, sp, view_p) and every decision it and the gate take - the first argmax
over the Lout valid conv positions, cmax > 0, the 0.35 threshold, the side of 0.5 - is checked against float64
(C.check_decisions): index work bit-exact, values within the a-priori rounding of a float32 evaluation, thresholds without
exception (the inputs keep every float64 value 1e-4 away from them).  Outputs and gradients are recomputed in float64 FROM the
HIP decisions and held to K x the distance the float32 CPU evaluation of the same formula has from float64 (C.gate, K = 14,
see control_decisions.K) - three to four orders of magnitude below what one wrong route moves
(test_gate_catches_one_wrong_route).
All outputs and workspaces are NaN-filled before each call, argl is filled with -7.  Every distance is logged to control.log
beside the parity tests' log.
"""
import os
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import control_decisions as C
from test_gpu_parity import LOG as PARITY_LOG
from test_gpu_parity import L, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "control.log")
D, AT = C.D, C.AT
_CASES = {}


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _ws(L, dev, name, *dims):
    wsb = L.size(name, *dims)
    return _nan(dev, wsb // 4 + 64), wsb


def _hip_head_forward(L, dev, x, entry="fp32", thr=C.THR32):
    """umpr_cnet_head_fwd on NaN-filled outputs and a NaN-filled workspace, argl filled with -7, Y allocated [B][S][L][KC];
    entry b16 sets umpr_set_gemm_bf16(1) around this one call."""
    B, S, Lm, V, KS, KC = x["dims"]
    d = {k: x[k].to(dev).contiguous() for k in ("X", "Wc", "bc", "Wl", "bl")}
    o = SimpleNamespace(Y=_nan(dev, B, S, Lm, KC), cmax=_nan(dev, B, S, KC), sp=_nan(dev, B, S, V), view_p=_nan(dev, B, S, V),
                        final=_nan(dev, B, V), argl=torch.full((B, S, KC), -7, dtype=torch.int32, device=dev), **d)
    ws, wsb = _ws(L, dev, "umpr_cnet_head_fwd_ws_bytes", B, S, Lm, KS)
    if entry == "b16":
        L.fn["umpr_set_gemm_bf16"](1)
    try:
        L.call("umpr_cnet_head_fwd", o.X, o.Wc, o.bc, o.Wl, o.bl, float(thr), B, S, Lm, KC, KS, V, o.Y, o.cmax, o.argl, o.sp,
               o.view_p, o.final, ws, wsb, st())
    finally:
        if entry == "b16":
            L.fn["umpr_set_gemm_bf16"](0)
    torch.cuda.synchronize()
    return o


def _hip_head_backward(L, dev, c, d_final=True, d_view_p=True, pre_dX=None, pre_w=None, argl=None):
    """umpr_cnet_head_bwd on the HIP forward's saved tensors; the five gradients are NaN-filled unless prefilled for
    accumulate_dX / accumulate_w, and so is the workspace.  Returns CPU copies (dX, dWc, dbc, dWl, dbl)."""
    o, x = c.hip, c.x
    B, S, Lm, V, KS, KC = x["dims"]
    dX = pre_dX.to(dev).contiguous() if pre_dX is not None else _nan(dev, B * S, Lm, D)
    shapes = ((KC, D, KS), (KC,), (V, KC), (V,))
    w = [t.to(dev).contiguous() for t in pre_w] if pre_w is not None else [_nan(dev, *s) for s in shapes]
    ws, wsb = _ws(L, dev, "umpr_cnet_head_bwd_ws_bytes", B, S, Lm, KC, KS, V)
    L.call("umpr_cnet_head_bwd", o.X, o.Wc, o.Wl, o.cmax, o.argl if argl is None else argl, o.sp, o.view_p,
           x["d_final"].to(dev).contiguous() if d_final else None, x["d_view_p"].to(dev).contiguous() if d_view_p else None,
           B, S, Lm, KC, KS, V, dX, 1 if pre_dX is not None else 0, 1 if pre_w is not None else 0, *w, ws, wsb, st())
    torch.cuda.synchronize()
    return (dX.cpu(), *[t.cpu() for t in w])


def _hip_snet_forward(L, dev, X, Ms, Ws, word_soft, dims, ld_senti=D, senti_off=0):
    """umpr_snet_fwd on NaN-filled outputs; senti rows land at column senti_off of a NaN-filled [B][ld_senti] buffer"""
    B, S, Lm, wl = dims
    o = SimpleNamespace(X=X.to(dev).contiguous(), Ms=Ms.to(dev).contiguous(), Ws=Ws.to(dev).contiguous(),
                        word_soft=word_soft.to(dev).contiguous(), U=_nan(dev, B * S, Lm, AT), P=_nan(dev, B * S, Lm),
                        wsum=_nan(dev, B, S), self_atte=_nan(dev, B, S, D), senti_buf=_nan(dev, B, ld_senti))
    L.call("umpr_snet_fwd", o.X, o.Ms, o.Ws, o.word_soft, wl, B, S, Lm, o.U, o.P, o.wsum, o.self_atte,
           o.senti_buf.data_ptr() + 4 * senti_off, ld_senti, st())
    torch.cuda.synchronize()
    return o


def _hip_gate_forward(L, dev, x, sa, view_p, c_out):
    B, S, Lm, V, KS, KC = x["dims"]
    o = SimpleNamespace(w=x["ssW"].to(dev).contiguous(), bias=x["ssb"].to(dev).contiguous(), senti=_nan(dev, B, S),
                        vs=_nan(dev, B, V), pp=_nan(dev, B, V), pn=_nan(dev, B, V))
    L.call("umpr_control_gate_fwd", sa, o.w, o.bias, view_p, c_out, B, S, V, o.senti, o.vs, o.pp, o.pn, st())
    torch.cuda.synchronize()
    return o


def _case(L, dev, shape, entry="fp32"):
    """HIP head forward of one shape through `entry`, the control S-Net and the gate behind it (fp32), every decision judged
    by float64, and - once the indices are inside their range - the float64 forward and its float32 yardstick conditioned on
    the HIP decisions.  Computed once per (shape, entry) and shared by the tests; nothing in it is modified afterwards."""
    if (shape, entry) in _CASES:
        return _CASES[shape, entry]
    B, S, Lm, V, KS, KC = shape
    x = C.make_inputs(*shape)
    c = SimpleNamespace(x=x, ops=C.bf16_operands(x) if entry == "b16" else x, entry=entry, tag=f"{shape} {entry}", refs={})
    c.hip = o = _hip_head_forward(L, dev, x, entry)
    c.sn = _hip_snet_forward(L, dev, x["X"], x["Ms"], x["Ws"], o.view_p, (B, S, Lm, V))
    c.g = _hip_gate_forward(L, dev, x, c.sn.self_atte, o.view_p, o.final)
    c.fails, c.stats = C.check_decisions(c.ops, o.Y, o.cmax, o.argl, o.sp, o.view_p, c.g.vs)
    log(f"{c.tag} decisions: " + " ".join(f"{k}={v:.3e}" for k, v in c.stats.items()) + (f" FAILS {c.fails}" if c.fails else ""))
    c.argl = o.argl.cpu().long().view(B * S, KC)
    c.in_range = bool(((c.argl >= 0) & (c.argl < C.lout(Lm, KS))).all())
    c.alive, c.kept = o.cmax.cpu().view(B * S, KC) > 0, o.view_p.cpu().view(B * S, V) > 0
    if c.in_range:
        c.f64 = C.forward64(c.ops, c.argl, c.kept)
        c.f32 = C.forward64(c.ops, c.argl, c.kept, dtype=torch.float32)
    _CASES[shape, entry] = c
    return c


def _refs(c, d_final=True, d_view_p=True):
    """(float64 reference, float32 yardstick, parts) of the head backward conditioned on the HIP decisions; cached"""
    key = (d_final, d_view_p)
    if key not in c.refs:
        up = (c.x["d_final"] if d_final else None, c.x["d_view_p"] if d_view_p else None)
        parts = {}
        ref = C.backward64(c.x, c.argl, c.alive, c.kept, *up, parts=parts)
        c.refs[key] = (ref, C.backward64(c.x, c.argl, c.alive, c.kept, *up, dtype=torch.float32), parts)
    return c.refs[key]


def _assert_gate(tag, names, got, ref, ref32):
    ok, rows = C.gate(got, ref, ref32, names=names, K=C.K, log=log, tag=tag)
    assert ok, [(r["name"], r["d_max"], r["d_l2"], r["r_max"], r["r_l2"], r["ratio"]) for r in rows if not r["ok"]]


@pytest.mark.parametrize("entry", ["fp32", "b16"])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_head_forward(L, dev, shape, entry):
    """Every saved tensor and decision of umpr_cnet_head_fwd against float64 (C.check_decisions: no failure), and sp, view_p,
    final through C.gate against forward64 recomputed from the HIP decisions.  b16: umpr_set_gemm_bf16(1) around the forward
    call only; the reference multiplies the bf16-rounded X and Wc.  Forward and decisions only - the bf16 gradients keep their
    bounds in tests/test_gpu_bf16.py."""
    c = _case(L, dev, shape, entry)
    assert not c.fails, c.fails
    o, B, S, V = c.hip, shape[0], shape[1], shape[3]
    _assert_gate(f"{c.tag} forward", ("sp", "view_p", "final"), (o.sp.cpu().view(B * S, V), o.view_p.cpu().view(B * S, V), o.final.cpu()),
                 (c.f64.sp, c.f64.view_p, c.f64.final), (c.f32.sp, c.f32.view_p, c.f32.final))


@pytest.mark.parametrize("variant", ["plain", "no_d_view_p", "no_d_final", "accumulate_dX", "accumulate_w"])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_head_backward(L, dev, shape, variant):
    """umpr_cnet_head_bwd (fp32) on the HIP forward's saved tensors: dX, dWc, dbc, dWl, dbl through C.gate against the float64
    backward conditioned on the HIP decisions.  no_d_view_p / no_d_final: that pointer NULL, the reference with zeros.
    accumulate_dX: dX prefilled with randn scaled to max |reference dX| and accumulate_dX = 1 (the weight gradients NaN-filled,
    overwritten); accumulate_w: the four weight gradients prefilled the same way and accumulate_w = 1 (dX NaN-filled,
    overwritten).  Prefill + gradient goes through the same gate, the float32 yardstick summed the same way."""
    c = _case(L, dev, shape)
    assert c.in_range, c.fails
    tag = f"{c.tag} {variant}"
    if variant in ("plain", "no_d_view_p", "no_d_final"):
        df, dv = variant != "no_d_final", variant != "no_d_view_p"
        ref, ref32, _ = _refs(c, df, dv)
        _assert_gate(tag, C.HEAD_GRADS, _hip_head_backward(L, dev, c, df, dv), ref, ref32)
        return
    ref, ref32, _ = _refs(c)
    g = torch.Generator().manual_seed(77 + sum(shape))
    pre = [torch.randn(r.shape, generator=g) for r in ref]
    pre = [p * (float(r.abs().max()) / float(p.abs().max())) for p, r in zip(pre, ref)]
    which = [0] if variant == "accumulate_dX" else [1, 2, 3, 4]
    got = _hip_head_backward(L, dev, c, pre_dX=pre[0] if variant == "accumulate_dX" else None,
                             pre_w=pre[1:] if variant == "accumulate_w" else None)
    _assert_gate(tag, C.HEAD_GRADS, got, [r + pre[i].double() if i in which else r for i, r in enumerate(ref)],
                 [r + pre[i] if i in which else r for i, r in enumerate(ref32)])


@pytest.mark.parametrize("shape", [(3, 5, 20, 1, 3, 120), (2, 7, 65, 4, 3, 120)])
def test_gate_catches_one_wrong_route(L, dev, shape):
    """umpr_cnet_head_bwd is handed the HIP argl with ONE entry - the live (sentence, filter) with the median |dc| - moved to
    the next valid position (a wrong argument value, in range): the gate against the unaltered reference fails, with dX and
    dWc both at least 10x outside."""
    c = _case(L, dev, shape)
    assert not c.fails, c.fails
    ref, ref32, parts = _refs(c)
    (n, k), _ = C.median_and_least_route(parts, c.alive, c.argl, C.lout(shape[2], shape[4]))
    wrong = c.hip.argl.clone()
    wrong.view(-1, shape[5])[n, k] += 1
    got = _hip_head_backward(L, dev, c, argl=wrong)
    ok, rows = C.gate(got, ref, ref32, names=C.HEAD_GRADS, K=C.K, log=log,
                      tag=f"{c.tag} sentence {n} filter {k} routed to position {int(c.argl[n, k]) + 1} instead of {int(c.argl[n, k])}")
    over = {r["name"]: r["over"] for r in rows}
    log(f"{c.tag} one wrong route: distance / bound = " + ", ".join(f"{k_} {v:.1f}x" for k_, v in over.items()))
    assert not ok
    assert over["dX"] >= 10 and over["dWc"] >= 10, over


@pytest.mark.parametrize("entry", ["fp32", "b16"])
@pytest.mark.parametrize("shape", [s for s in C.SHAPES if s[2] >= 8])
def test_exact_ties_take_the_first_index(L, dev, shape, entry):
    """Past each sentence's length X is zero, so many windows of X are bit-identical (all-zero ones give exactly relu(bc[k])).
    For every (sentence, filter) whose float64 maximum is attained inside a group of bit-identical windows, Y is bit-equal
    across the group and argl names the group's FIRST position - `y > m`, never `y >= m`.  (A maximum that leads the other
    windows by less than the two a-priori deltas may legitimately sit elsewhere in float32; such cases are counted, there are
    none in the fp32 runs recorded.)  Each shape holds at least one such live group."""
    c = _case(L, dev, shape, entry)
    assert c.in_range, c.fails
    B, S, Lm, V, KS, KC = shape
    N, Lo, pad = B * S, C.lout(Lm, KS), (KS - 1) // 2
    X = c.ops["X"]
    win = F.pad(X, (0, 0, pad, KS - 1 - pad)).unfold(1, KS, 1)[:, :Lo].reshape(N, Lo, -1)
    pre64 = C.conv64(X, c.ops["Wc"], c.ops["bc"], KS)
    delta = C.rounding_delta(X, c.ops["Wc"], c.ops["bc"], KS)
    Yh = c.hip.Y.cpu().view(N, Lm, KC)[:, :Lo]
    groups = excused = 0
    for n in range(N):
        _, inv, counts = torch.unique(win[n], dim=0, return_inverse=True, return_counts=True)
        first = torch.full((len(counts),), Lo).scatter_reduce(0, inv, torch.arange(Lo), "amin")
        amax = pre64[n].argmax(0)                                  # [KC] a position of the float64 maximum
        gid = inv[amax]                                            # its group
        member = inv.view(Lo, 1) == gid.view(1, KC)                # [Lo][KC]
        tied = (counts[gid] > 1) & (pre64[n].max(0).values > delta[n].max(0).values)      # live beyond rounding
        y_first = Yh[n].gather(0, first[gid].view(1, KC)).squeeze(0)
        same = ((Yh[n] == y_first.view(1, KC)) | ~member).all(0)
        assert bool(same[tied].all()), (n, torch.nonzero(tied & ~same).flatten().tolist())
        outside = torch.where(member, torch.full_like(pre64[n], -float("inf")), pre64[n])
        lead = pre64[n].max(0).values - outside.max(0).values
        decisive = lead > 2 * delta[n].max(0).values
        wrong = tied & (c.argl[n] != first[gid])
        assert not bool((wrong & decisive).any()), (n, [(int(k), int(c.argl[n, k]), int(first[gid[k]])) for k in torch.nonzero(wrong & decisive).flatten()])
        groups += int(tied.sum())
        excused += int((wrong & ~decisive).sum())
    log(f"{c.tag} exact ties: {groups} live maxima inside a group of bit-identical windows, {excused} within rounding of another window")
    assert groups >= 1


def test_threshold_edge(L, dev):
    """`sg < thr ? 0 : sg` at the edge: with thr equal to one sp value t that entry is kept (t < t is false), with thr =
    nextafter(t, +inf) it is zero and so is its contribution to final; sp itself does not move, and every entry of view_p is
    bit-exactly where(sp < thr, 0, sp) at both thresholds."""
    shape = (2, 3, 11, 4, 2, 120)
    B, S, Lm, V, KS, KC = shape
    c = _case(L, dev, shape)
    sp = c.hip.sp.cpu().view(B * S, V)
    n, v = [int(i) for i in torch.nonzero(sp >= C.THR32)[0]]
    t = sp[n, v]
    b = n // S
    finals = []
    for thr, kept in ((t, True), (torch.nextafter(t, torch.tensor(float("inf"))), False)):
        o = _hip_head_forward(L, dev, c.x, thr=float(thr))
        sp2, vp = o.sp.cpu().view(B * S, V), o.view_p.cpu().view(B * S, V)
        assert torch.equal(sp2, sp)
        assert torch.equal(vp, torch.where(sp < thr, torch.zeros_like(sp), sp))
        assert float(vp[n, v]) == (float(t) if kept else 0.0)
        want = (vp.double() ** 2).view(B, S, V).sum(1)
        fin = o.final.cpu().double()
        assert bool(((fin - want).abs() <= S * 2.0 ** -23 * want).all()), (fin, want)
        finals.append(float(fin[b, v]))
    log(f"{c.tag} threshold edge: sp[{n}][{v}] = {float(t)!r}, final[{b}][{v}] {finals[0]!r} kept, {finals[1]!r} dropped")
    assert abs(finals[0] - finals[1] - float(t) ** 2) <= 1e-6


@pytest.mark.parametrize("shape", C.SHAPES)
def test_control_gate(L, dev, shape):
    """umpr_control_gate_fwd / _bwd on the head's own view_p and final and the control S-Net's self_atte: senti, view_score,
    prefer_pos, prefer_neg and the five gradients through C.gate against the float64 gate with the HIP side of 0.5 given.  A
    view column that is zero for every sentence (den = 1e-4 exactly) gets exactly zero d_view_p."""
    c = _case(L, dev, shape)
    assert not c.fails, c.fails
    B, S, Lm, V, KS, KC = shape
    x, o, g = c.x, c.hip, c.g
    sa, vp, co = c.sn.self_atte.cpu(), o.view_p.cpu(), o.final.cpu()
    side = g.vs.cpu() > 0.5
    f64 = C.gate_forward64(sa, x["ssW"], x["ssb"], vp, co, side)
    f32 = C.gate_forward64(sa, x["ssW"], x["ssb"], vp, co, side, dtype=torch.float32)
    pick = lambda f: (f.senti, f.vs, f.prefer_pos, f.prefer_neg)
    _assert_gate(f"{c.tag} gate forward", ("senti", "view_score", "prefer_pos", "prefer_neg"),
                 (g.senti.cpu(), g.vs.cpu(), g.pp.cpu(), g.pn.cpu()), pick(f64), pick(f32))
    outs = [_nan(dev, B, S, D), _nan(dev, B, S, V), _nan(dev, B, V), _nan(dev, D), _nan(dev, 1)]
    ws, wsb = _ws(L, dev, "umpr_control_gate_bwd_ws_bytes", B)
    L.call("umpr_control_gate_bwd", c.sn.self_atte, g.w, o.view_p, o.final, g.senti, g.vs, x["d_prefer_pos"].to(dev),
           x["d_prefer_neg"].to(dev), B, S, V, *outs, ws, wsb, st())
    torch.cuda.synchronize()
    got = [t.cpu() for t in outs]
    up = (x["d_prefer_pos"], x["d_prefer_neg"])
    _assert_gate(f"{c.tag} gate backward", C.GATE_GRADS, got, C.gate_backward64(sa, x["ssW"], x["ssb"], vp, co, side, *up),
                 C.gate_backward64(sa, x["ssW"], x["ssb"], vp, co, side, *up, dtype=torch.float32))
    zero_col = (vp == 0).all(1)                                    # [B][V]
    assert torch.equal(zero_col, (C.decisions64(x).f.view_p.view(B, S, V) == 0).all(1))
    assert bool((got[1].transpose(1, 2)[zero_col] == 0).all())
    log(f"{c.tag} gate: {int(zero_col.sum())} all-zero view columns, sides {int(side.sum())} above / {int((~side).sum())} below 0.5")


@pytest.mark.parametrize("form", ["review", "control"])
@pytest.mark.parametrize("B,S,Lm", C.SNET_SHAPES)
def test_snet_stage(L, dev, B, S, Lm, form):
    """umpr_snet_fwd / _bwd at the stage level, all outputs (U, P, wsum, self_atte, senti) and gradients through C.gate against
    float64 autograd of the oracle's s_net.  review form (as the ReviewNet calls it): wl = L, senti and d_senti are the upper
    halves of [B][256] rows (ld = 256; the lower halves stay NaN), d_self_atte = NULL, d_word_soft given.  control form (as the
    ControlNet calls it): wl = V = 3, d_senti zero, d_self_atte given, d_word_soft = NULL.  L = 64 / 65 and 128 / 130 / 200
    straddle the one-, two- and four-slot kernels."""
    wl = Lm if form == "review" else 3
    x = C.make_snet_inputs(B, S, Lm, wl)
    ld, off = (2 * D, D) if form == "review" else (D, 0)
    o = _hip_snet_forward(L, dev, x["X"], x["Ms"], x["Ws"], x["word_soft"], (B, S, Lm, wl), ld, off)
    up = (x["d_senti"], None) if form == "review" else (None, x["d_self_atte"])
    out64, g64 = C.snet64(x, *up)
    out32, g32 = C.snet64(x, *up, dtype=torch.float32)
    tag = f"snet B{B} S{S} L{Lm} {form}"
    senti = o.senti_buf.cpu()
    assert bool(torch.isnan(senti[:, :off]).all()) and bool(torch.isnan(senti[:, off + D:]).all()), "senti written outside its 128 columns"
    _assert_gate(tag, C.SNET_OUT, (o.U.cpu(), o.P.cpu(), o.wsum.cpu(), o.self_atte.cpu(), senti[:, off:off + D]), out64, out32)
    ds = _nan(dev, B, ld)
    ds[:, off:off + D] = x["d_senti"].to(dev) if form == "review" else 0.0
    dsa = x["d_self_atte"].to(dev).contiguous() if form == "control" else None
    dX, dMs, dWs = _nan(dev, B * S, Lm, D), _nan(dev, AT, D), _nan(dev, AT)
    dws = _nan(dev, B, S, wl) if form == "review" else None
    ws, wsb = _ws(L, dev, "umpr_snet_bwd_ws_bytes", B, S, Lm)
    L.call("umpr_snet_bwd", o.X, o.Ms, o.Ws, o.U, o.P, o.wsum, o.self_atte, ds.data_ptr() + 4 * off, ld, dsa, B, S, Lm, wl, dX, dMs,
           dWs, dws, ws, wsb, st())
    torch.cuda.synchronize()
    n = 4 if form == "review" else 3
    names = ("dX", "dMs", "dWs", "d_word_soft")[:n]
    got = [t.cpu() for t in (dX, dMs, dWs, dws)[:n]]
    _assert_gate(tag, names, got, g64[:n], g32[:n])


def _ragged_ids(g, n, Lm, vocab):
    lengths = torch.randint(1, Lm + 1, (n,), generator=g)
    lengths[0] = Lm
    ids = torch.randint(3, vocab, (n, Lm), generator=g)
    ids = ids * (torch.arange(Lm).view(1, Lm) < lengths.view(n, 1))
    return ids, lengths


@pytest.mark.parametrize("shape", [(2, 3, 11, 4, 2, 120), (2, 7, 65, 4, 3, 120)])
def test_fused_entry_equals_the_stages(L, dev, shape):
    """umpr_control_net_fwd / _bwd - what training calls (_ControlNetF) - against the chain csrc/text_path.hip issues through
    the stage-level entry points: umpr_embed_gru_bidir_fwd twice, three heads, S-Net, gate; then gate, S-Net, three heads with
    the same accumulate flags, and the GRU backward twice.  Ragged lengths; the user / item pair has one sentence more and two
    tokens fewer than the ui reviews.  The header promises the same kernels and the same arithmetic: the four outputs and all
    16 gradients are torch.equal."""
    from umpr_amd.model import UMPR
    from umpr_amd.synthetic import make_param_state
    B, S_ui, L_ui, V, KS, KC = shape
    S, Lm, E, vocab = S_ui + 1, L_ui - 2, 50, 500
    Nui, N = B * S_ui, B * S
    x = C.make_inputs(*shape)
    P = make_param_state(13, E, vocab, V, False, with_vgg=False, m_scale=0.3, kernel_size=KS, kernel_count=KC)
    g = torch.Generator().manual_seed(31 + sum(shape))
    emb = P["embedding.weight"].to(dev).contiguous()
    gp = "control_net.c_net.gru.module."
    gru = [P[gp + n + s] for s in ("", "_reverse") for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    params = [t.to(dev).contiguous() for t in gru + [x[k] for k in ("Wc", "bc", "Wl", "bl", "Ms", "Ws", "ssW", "ssb")]]
    ids_ui, len_ui = _ragged_ids(g, Nui, L_ui, vocab)
    ids_u, len_u = _ragged_ids(g, N, Lm, vocab)
    ids_i, len_i = _ragged_ids(g, N, Lm, vocab)
    lens_ui, ord_ui = UMPR._host_perm(len_ui, dev)
    (lu, ou), (li, oi) = UMPR._host_perm(len_u, dev), UMPR._host_perm(len_i, dev)
    lens_pair, ord_pair = torch.cat([lu, li]).contiguous(), torch.cat([ou, oi + N]).contiguous()
    ids_ui, ids_pair = ids_ui.to(dev).contiguous(), torch.cat([ids_u, ids_i]).to(dev).contiguous()
    ups = [torch.randn(B, V, generator=g).to(dev) for _ in range(4)]              # d_cu, d_ci, d_pp, d_pn
    ptrs = lambda ts: torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64)   # a host array of device pointers

    # ---- the fused entries
    arena = _nan(dev, L.size("umpr_control_net_arena_bytes", B, S_ui, L_ui, S, Lm, KC, V) // 4 + 64)
    ws, wsb = _ws(L, dev, "umpr_control_net_ws_bytes", B, S_ui, L_ui, S, Lm, E, KC, KS, V)
    fused_out = [_nan(dev, B, V) for _ in range(4)]
    parr = ptrs(params)
    L.call("umpr_control_net_fwd", ids_ui, ids_pair, emb, E, parr.data_ptr(), lens_ui, ord_ui, lens_pair, ord_pair, B, S_ui, L_ui, S,
           Lm, KC, KS, V, float(C.THR32), 0, 1, arena, *fused_out, ws, wsb, st())
    fused_g = [_nan(dev, *p.shape) for p in params]
    garr = ptrs(fused_g)
    ws.fill_(float("nan"))
    L.call("umpr_control_net_bwd", ids_ui, ids_pair, emb, E, parr.data_ptr(), lens_ui, ord_ui, lens_pair, ord_pair, B, S_ui, L_ui, S,
           Lm, KC, KS, V, 0, arena, *ups, garr.data_ptr(), ws, wsb, st())
    torch.cuda.synchronize()

    # ---- the same chain through the stage-level entry points
    def gru_fwd(ids, lens, order, n, l):
        out, saved = _nan(dev, n, l, D), _nan(dev, 2, n, l, 4, 64)
        w, wb = _ws(L, dev, "umpr_embed_gru_bidir_ws_bytes", n, l, E)
        L.call("umpr_embed_gru_bidir_fwd", ids, emb, E, *params[:8], lens, order, order, n, l, out, saved, w, wb, st())
        return out, saved
    gru_ui, saved_ui = gru_fwd(ids_ui, lens_ui, ord_ui, Nui, L_ui)
    gru_pair, saved_pair = gru_fwd(ids_pair, lens_pair, ord_pair, 2 * N, Lm)
    Xs = (gru_ui, gru_pair[:N], gru_pair[N:])
    dims = ((S_ui, L_ui), (S, Lm), (S, Lm))
    Wc, bc, Wl, bl, Ms, Ws, ssW, ssb = params[8:]
    heads = []
    for X, (s, l) in zip(Xs, dims):
        h = SimpleNamespace(Y=_nan(dev, B, s, l, KC), cmax=_nan(dev, B, s, KC), sp=_nan(dev, B, s, V), vp=_nan(dev, B, s, V),
                            fin=_nan(dev, B, V), argl=torch.full((B, s, KC), -7, dtype=torch.int32, device=dev))
        w, wb = _ws(L, dev, "umpr_cnet_head_fwd_ws_bytes", B, s, l, KS)
        L.call("umpr_cnet_head_fwd", X, Wc, bc, Wl, bl, float(C.THR32), B, s, l, KC, KS, V, h.Y, h.cmax, h.argl, h.sp, h.vp, h.fin,
               w, wb, st())
        heads.append(h)
    sn = SimpleNamespace(U=_nan(dev, Nui, L_ui, AT), P=_nan(dev, Nui, L_ui), wsum=_nan(dev, B, S_ui), sa=_nan(dev, B, S_ui, D))
    L.call("umpr_snet_fwd", gru_ui, Ms, Ws, heads[0].vp, V, B, S_ui, L_ui, sn.U, sn.P, sn.wsum, sn.sa, _nan(dev, B, D), D, st())
    senti, vs, pp, pn = _nan(dev, B, S_ui), _nan(dev, B, V), _nan(dev, B, V), _nan(dev, B, V)
    L.call("umpr_control_gate_fwd", sn.sa, ssW, ssb, heads[0].vp, heads[0].fin, B, S_ui, V, senti, vs, pp, pn, st())
    stage_out = [heads[1].fin, heads[2].fin, pp, pn]
    G = [_nan(dev, *p.shape) for p in params]
    d_sa, d_vp, d_cout = _nan(dev, B, S_ui, D), _nan(dev, B, S_ui, V), _nan(dev, B, V)
    w, wb = _ws(L, dev, "umpr_control_gate_bwd_ws_bytes", B)
    L.call("umpr_control_gate_bwd", sn.sa, ssW, heads[0].vp, heads[0].fin, senti, vs, ups[2], ups[3], B, S_ui, V, d_sa, d_vp, d_cout,
           G[14], G[15], w, wb, st())
    dX_ui, dX_pair = _nan(dev, Nui, L_ui, D), _nan(dev, 2 * N, Lm, D)
    w, wb = _ws(L, dev, "umpr_snet_bwd_ws_bytes", B, S_ui, L_ui)
    L.call("umpr_snet_bwd", gru_ui, Ms, Ws, sn.U, sn.P, sn.wsum, sn.sa, torch.zeros(B, D, device=dev), D, d_sa, B, S_ui, L_ui, V, dX_ui,
           G[12], G[13], None, w, wb, st())
    dXs = (dX_ui, dX_pair[:N], dX_pair[N:])
    for q, (X, (s, l), h, dX, dfin, dvp) in enumerate(zip(Xs, dims, heads, dXs, (d_cout, ups[0], ups[1]), (d_vp, None, None))):
        w, wb = _ws(L, dev, "umpr_cnet_head_bwd_ws_bytes", B, s, l, KC, KS, V)
        L.call("umpr_cnet_head_bwd", X, Wc, Wl, h.cmax, h.argl, h.sp, h.vp, dfin, dvp, B, s, l, KC, KS, V, dX, 1 if q == 0 else 0,
               0 if q == 0 else 1, G[8], G[9], G[10], G[11], w, wb, st())
    for ids, lens, order, n, l, dout, out, saved, acc in ((ids_ui, lens_ui, ord_ui, Nui, L_ui, dX_ui, gru_ui, saved_ui, 0),
                                                          (ids_pair, lens_pair, ord_pair, 2 * N, Lm, dX_pair, gru_pair, saved_pair, 1)):
        w, wb = _ws(L, dev, "umpr_embed_gru_bidir_ws_bytes", n, l, E)
        L.call("umpr_embed_gru_bidir_bwd_acc", ids, emb, E, params[1], params[5], lens, order, order, n, l, dout, out, saved, *G[:8],
               acc, w, wb, st())
    torch.cuda.synchronize()

    names = ["c_u", "c_i", "prefer_pos", "prefer_neg"] + [f"grad[{i}]" for i in range(16)]
    differing = []
    for name, a, b in zip(names, fused_out + fused_g, stage_out + G):
        assert bool(torch.isfinite(a).all()) and bool(torch.isfinite(b).all()), name
        if not torch.equal(a, b):
            differing.append((name, float((a - b).abs().max()), float(b.abs().max())))
    log(f"{shape} fused entry against the stages: {len(names) - len(differing)} of {len(names)} tensors bit-equal" +
        (f", differing {differing}" if differing else ""))
    assert not differing, differing
