"""CPU tests of the decision-conditioned control-network reference (tests/control_decisions.py) that the GPU gates of
tests/test_gpu_control.py compare the HIP kernels with.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import control_decisions as C

_X = {}


def _inputs(shape):
    if shape not in _X:
        _X[shape] = C.make_inputs(*shape)
    return _X[shape]


def _close(name, got, want, rel=1e-12):
    got, want = got.detach().double(), want.detach().double()
    assert got.shape == want.shape, (name, got.shape, want.shape)
    scale = float(want.abs().max())
    assert float((got - want).abs().max()) <= rel * max(scale, 1e-300), (name, float((got - want).abs().max()), scale)
    return scale


@pytest.mark.parametrize("form", ["both", "no_d_view_p", "no_d_final"])
@pytest.mark.parametrize("shape", C.SHAPES)
def test_backward64_equals_autograd(shape, form):
    """The oracle's head formula (oracle/umpr_ref.py: c_net, src/model.py:118-125) under float64 autograd, and backward64 given
    the decisions autograd itself took (the index its max returned, cmax > 0, view_p > 0): forward values and all five
    gradients agree to 1e-12 of each tensor's maximum, in both optional-gradient forms and with both.  Where a maximum is
    attained once, autograd's index is the first index."""
    B, S, L, V, KS, KC = shape
    x = _inputs(shape)
    X, Wc, bc, Wl, bl = (x[k].double().requires_grad_(True) for k in ("X", "Wc", "bc", "Wl", "bl"))
    y = F.relu(F.conv1d(X.transpose(-1, -2), Wc, bc, padding=(KS - 1) // 2))
    cm, idx = y.max(dim=-1)
    sp = torch.sigmoid(F.linear(cm, Wl, bl))
    vp = torch.where(sp < C.THR32, torch.zeros_like(sp), sp)
    fin = (vp.view(B, S, V) ** 2).sum(-2)
    d_final = None if form == "no_d_final" else x["d_final"]
    d_view_p = None if form == "no_d_view_p" else x["d_view_p"]
    outs = [o for o, u in ((fin, d_final), (vp.view(B, S, V), d_view_p)) if u is not None]
    torch.autograd.backward(outs, [u.double() for u in (d_final, d_view_p) if u is not None])
    yd = y.detach().transpose(1, 2)
    m, first = C.first_argmax(yd)
    once = (yd == m.unsqueeze(1)).sum(1) == 1
    assert bool((idx[once] == first[once]).all())
    f = C.forward64(x, idx, vp.detach() > 0)
    for name, got, want in (("cmax", f.cmax, cm), ("sp", f.sp, sp), ("view_p", f.view_p, vp), ("final", f.final, fin)):
        _close(name, got, want)
    got = C.backward64(x, idx, cm.detach() > 0, vp.detach() > 0, d_final, d_view_p)
    for name, g, w in zip(C.HEAD_GRADS, got, (X.grad, Wc.grad, bc.grad, Wl.grad, bl.grad)):
        assert _close(name, g, w) > 0, name


@pytest.mark.parametrize("shape", C.SHAPES)
def test_gate_backward64_equals_autograd(shape):
    """The gate formulas of src/model.py:186-197 under float64 autograd against gate_forward64 / gate_backward64 with the side
    autograd's own view_score falls on, on the reference's view_p and final as independent inputs."""
    B, S, L, V, KS, KC = shape
    x = _inputs(shape)
    d = C.decisions64(x)
    _, _, sa0 = C.self_atte(x["X"].double(), x["Ms"].double(), x["Ws"].double())
    sa, w, b, vp, co = (t.double().clone().requires_grad_(True) for t in
                        (sa0.view(B, S, C.D), x["ssW"], x["ssb"], d.f.view_p.view(B, S, V), d.f.final))
    senti = torch.sigmoid(F.linear(sa, w.view(1, -1), b)).expand(-1, -1, V)
    vs = (senti * vp ** 2).sum(-2) / ((vp ** 2).sum(-2) + 1e-4)
    q_p = (vs > 0.5).double()
    q_pos = torch.where(vs < 0.5, torch.zeros_like(vs), 4 * (vs - 0.5) ** 2)
    q_neg = torch.where(vs > 0.5, torch.zeros_like(vs), 4 * (0.5 - vs) ** 2)
    pp, pn = co * q_p * q_pos, co * (1 - q_p) * q_neg
    torch.autograd.backward([pp, pn], [x["d_prefer_pos"].double(), x["d_prefer_neg"].double()])
    side = vs.detach() > 0.5
    f = C.gate_forward64(sa.detach(), w.detach(), b.detach(), vp.detach(), co.detach(), side)
    for name, got, want in (("senti", f.senti, senti[..., 0]), ("vs", f.vs, vs), ("prefer_pos", f.prefer_pos, pp),
                            ("prefer_neg", f.prefer_neg, pn)):
        _close(name, got, want)
    got = C.gate_backward64(sa.detach(), w.detach(), b.detach(), vp.detach(), co.detach(), side, x["d_prefer_pos"], x["d_prefer_neg"])
    for name, g, want in zip(C.GATE_GRADS, got, (sa.grad, vp.grad, co.grad, w.grad, b.grad)):
        _close(name, g, want, rel=1e-11)


@pytest.mark.parametrize("B,S,L", C.SNET_SHAPES)
def test_snet64_is_consistent(B, S, L):
    """snet64 is float64 autograd of the oracle's s_net; the U and P it reports beside it reproduce the oracle's self_atte,
    and the gradient of the word weights is d_senti . self_atte for every word of a sentence."""
    x = C.make_snet_inputs(B, S, L, L)
    (U, P, wsum, sa, senti), (dX, dMs, dWs, dws) = C.snet64(x, x["d_senti"], None)
    _close("self_atte", (P.unsqueeze(-1) * x["X"].double()).sum(1).view(B, S, C.D), sa)
    _close("senti", (wsum.unsqueeze(-1) * sa).sum(1), senti)
    _close("d_word_soft", dws, (sa * x["d_senti"].double().unsqueeze(1)).sum(-1, keepdim=True).expand(B, S, L))
    assert float(U.abs().max()) < 0.99          # tanh not saturated: 1 - U^2 carries no cancellation
    assert float(dX.abs().max()) > 0
    if L > 1:
        assert float(dMs.abs().max()) > 0 and float(dWs.abs().max()) > 0
    else:       # one position: the softmax is the constant 1 (C.distances then demands exact zeros of the kernel)
        assert float(dMs.abs().max()) == 0 and float(dWs.abs().max()) == 0


def test_conditions():
    """What the issue demands of the inputs, asserted on the float64 reference alone (seeds in C.SEEDS chosen so that they
    hold): no sigmoid within 1e-4 of the threshold and no view_score within 1e-4 of 0.5, so that no threshold or gate decision
    is excused; across the shapes with L >= 8 at least 5 % dead filters, live maxima tied at more than one position and
    argmaxes at padded positions; in each even-KS shape the excluded position L - 1 beats every valid one somewhere; in each
    V > 1 shape view_score on both sides of 0.5; and a view column that is zero for every sentence (den = 1e-4 exactly)."""
    dead, cells, tied, padded, zero_cols = 0.0, 0, 0, 0, 0
    for shape in C.SHAPES:
        B, S, L, V, KS, KC = shape
        c = C.conditions(_inputs(shape))
        print(shape, c)
        assert c["sp_margin"] >= C.MARGIN and c["vs_margin"] >= C.MARGIN, (shape, c)
        if KS % 2 == 0:
            assert c["n_excluded_wins"] >= 1, (shape, c)
        if V > 1:
            assert min(c["sides"]) >= 1, (shape, c)
        if L >= 8:
            assert c["dead"] >= 0.05, (shape, c)
            dead += c["dead"] * B * S * KC
            cells += B * S * KC
            tied += c["n_tied_live"]
            padded += c["n_padded"]
        zero_cols += c["n_zero_columns"]
    assert dead / cells >= 0.05 and tied >= 1 and padded >= 1 and zero_cols >= 1, (dead / cells, tied, padded, zero_cols)


@pytest.mark.parametrize("shape", C.SHAPES)
def test_check_decisions_accepts_float32_and_rejects_wrong_decisions(shape):
    """The float32 CPU evaluation's saved tensors pass, far inside the a-priori bound.  Rejected: a value 2 delta off; an index
    at Lout (for an even KS a position the GEMM did write) and a negative one; a clear loser; the LATER index of an exact tie
    with the right cmax; a kept entry whose sp lies below the threshold - both as view_p alone and as a consistent (sp,
    view_p) pair that float64 contradicts; a view_score on the wrong side of 0.5."""
    B, S, L, V, KS, KC = shape
    x = _inputs(shape)
    Lo = C.lout(L, KS)
    e = C.evaluate32(x)
    saved = lambda: dict(Y=e.Y.clone(), cmax=e.cmax.clone(), argl=e.argl.clone(), sp=e.sp.clone(), view_p=e.view_p.clone(),
                         view_score=e.view_score.clone())
    fails, stats = C.check_decisions(x, **saved())
    assert not fails, fails
    assert stats["y_over_delta"] < 0.1, stats
    delta = C.rounding_delta(x["X"], x["Wc"], x["bc"], KS)

    def rejected(key, **change):
        s = saved()
        s.update(change)
        fails = C.check_decisions(x, **s)[0]
        assert any(f.startswith(key) for f in fails), (key, fails)

    live = torch.nonzero(e.cmax > 0)
    n, k = [int(v) for v in live[0]]
    Y = e.Y.clone()
    Y[n, int(e.argl[n, k]), k] += 2 * float(delta[n, int(e.argl[n, k]), k])
    rejected("Y", Y=Y)
    for bad in (Lo, -1):
        a = e.argl.clone()
        a[n, k] = bad
        rejected("argl", argl=a)
    if Lo > 1:
        Yv = e.Y[:, :Lo]
        once = torch.nonzero(((Yv == e.cmax.unsqueeze(1)).sum(1) == 1) & (e.cmax > 0))
        n, k = [int(v) for v in once[0]]
        a, c = e.argl.clone(), e.cmax.clone()
        a[n, k] = (int(a[n, k]) + 1) % Lo
        c[n, k] = Yv[n, a[n, k], k]
        rejected("argl", argl=a, cmax=c)
        ties = torch.nonzero((Yv == e.cmax.unsqueeze(1)).sum(1) > 1)
        assert len(ties), "no tie in this shape"
        n, k = [int(v) for v in ties[-1]]
        later = torch.nonzero(Yv[n, :, k] == e.cmax[n, k]).flatten()
        assert int(later[0]) == int(e.argl[n, k])
        a = e.argl.clone()
        a[n, k] = int(later[1])
        rejected("argl", argl=a)                  # cmax is the same value at both positions: only the index is wrong
    below = torch.nonzero(e.sp < C.THR32)
    if len(below):
        n, v = [int(i) for i in below[0]]
        vp = e.view_p.clone()
        vp[n, v] = e.sp[n, v]
        rejected("view_p", view_p=vp)
        sp, vp = e.sp.clone(), e.view_p.clone()
        sp[n, v] = vp[n, v] = 0.36
        rejected("threshold", sp=sp, view_p=vp)
    vs = e.view_score.clone()
    vs[0, 0] = 1.0 - vs[0, 0]
    rejected("gate", view_score=vs)


@pytest.mark.parametrize("shape", [s for s in C.SHAPES if C.lout(s[2], s[4]) > 1])
def test_one_wrong_route_moves_dX_and_dWc_far_past_the_gate(shape):
    """A pure misroute in float64 - what the GPU test test_gate_catches_one_wrong_route hands umpr_cnet_head_bwd: the live
    (sentence, filter) entry with the MEDIAN |dc| sends its gradient to the next valid position while cmax, sp and view_p stay
    those of the right decisions.  dX and dWc then lie at least 10x outside the gate at its widest factor, 14.  The factor of
    the least visible entry (smallest non-zero |dc|) is printed."""
    B, S, L, V, KS, KC = shape
    x = _inputs(shape)
    d = C.decisions64(x)
    parts = {}
    ref = C.backward64(x, d.argl, d.alive, d.kept, x["d_final"], x["d_view_p"], parts=parts)
    ref32 = C.backward64(x, d.argl, d.alive, d.kept, x["d_final"], x["d_view_p"], dtype=torch.float32)
    ok, rows = C.gate(ref32, ref, ref32, names=C.HEAD_GRADS, K=1.0)
    assert ok, rows
    med, least = C.median_and_least_route(parts, d.alive, d.argl, C.lout(L, KS))
    assert med is not None
    over = {}
    for tag, (n, k) in (("median", med), ("least", least)):
        route = d.argl.clone()
        route[n, k] += 1
        moved = C.backward64(x, d.argl, d.alive, d.kept, x["d_final"], x["d_view_p"], route=route)
        ok, rows = C.gate(moved, ref, ref32, names=C.HEAD_GRADS, K=C.K_MAX)
        over[tag] = {r["name"]: r["over"] for r in rows}
        assert not ok or tag == "least"           # the least visible entry is logged, not asserted
        for name in ("dbc", "dWl", "dbl"):        # a route does not touch them
            assert over[tag][name] <= 1 / C.K_MAX, (tag, name, over[tag][name])
    print(f"{shape}: one wrong route, distance / (14 x floored ref32 distance): median |dc| entry dX {over['median']['dX']:.3g}x "
          f"dWc {over['median']['dWc']:.3g}x; least visible entry dX {over['least']['dX']:.3g}x dWc {over['least']['dWc']:.3g}x")
    assert over["median"]["dX"] >= 10 and over["median"]["dWc"] >= 10, over
