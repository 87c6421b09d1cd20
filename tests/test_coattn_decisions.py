"""CPU tests of the decision-conditioned co-attention reference (tests/coattn_decisions.py) that the GPU gates of
tests/test_gpu_coattn.py compare the HIP kernels with.  No GPU needed."""
import pytest
import torch

import coattn_decisions as C


def _scores(x):
    T64 = x["Gi"].double() @ x["M"].double()
    return T64, C.scores64(T64, x["Gu"])


def _refs(x, T64, A64, ac, ar):
    """(float64 reference, float32 yardstick) of the backward with the decisions (ac, ar)"""
    up = (x["d_atte_u"], x["d_atte_i"], x["d_soft_u"], x["d_soft_i"])
    ref = C.backward64(x["Gu"], x["Gi"], x["M"], T64, A64, ac, ar, *up)
    T32 = x["Gi"] @ x["M"]
    A32 = torch.tanh(T32 @ x["Gu"].transpose(-1, -2))
    return ref, C.backward64(x["Gu"], x["Gi"], x["M"], T32, A32, ac, ar, *up, dtype=torch.float32)


@pytest.mark.parametrize("B,SL", [(2, 1), (2, 7), (3, 65), (2, 130)])
@pytest.mark.parametrize("with_soft", [True, False])
def test_backward64_equals_autograd(B, SL, with_soft):
    """With its own float64 argmax, backward64 is the gradient of the oracle's formula (oracle/umpr_ref.py: r_net,
    src/model.py:50-55) as float64 autograd computes it: 1e-12 of each tensor's maximum."""
    x = C.make_inputs(B, SL)
    Gu, Gi, M = (x[k].double().requires_grad_(True) for k in ("Gu", "Gi", "M"))
    A = torch.tanh(Gi @ M @ Gu.transpose(-1, -2))
    soft_u = torch.softmax(torch.max(A, dim=-2).values, dim=-1)
    soft_i = torch.softmax(torch.max(A, dim=-1).values, dim=-1)
    atte_u = (Gu.transpose(-1, -2) @ soft_u.unsqueeze(-1)).squeeze(-1)
    atte_i = (Gi.transpose(-1, -2) @ soft_i.unsqueeze(-1)).squeeze(-1)
    outs, ups = [atte_u, atte_i], [x["d_atte_u"].double(), x["d_atte_i"].double()]
    if with_soft:
        outs += [soft_u, soft_i]
        ups += [x["d_soft_u"].double(), x["d_soft_i"].double()]
    torch.autograd.backward(outs, ups)
    Ad = A.detach()
    ac, ar = Ad.argmax(1), Ad.argmax(2)
    cm, rm, su, si, au, ai = C.forward64(x["Gu"], x["Gi"], Ad, ac, ar)
    for got, want in ((su, soft_u), (si, soft_i), (au, atte_u), (ai, atte_i)):
        assert float((got - want.detach()).abs().max()) <= 1e-12
    got = C.backward64(x["Gu"], x["Gi"], x["M"], (Gi @ M).detach(), Ad, ac, ar, x["d_atte_u"], x["d_atte_i"],
                       x["d_soft_u"] if with_soft else None, x["d_soft_i"] if with_soft else None)
    for name, g, want in zip(("dGu", "dGi", "dM"), got, (Gu.grad, Gi.grad, M.grad)):
        scale = float(want.abs().max())
        if SL == 1:
            assert name != "dM" or scale == 0.0          # one position: the softmax is the constant 1
        else:
            assert scale > 0, name
        assert float((g - want).abs().max()) <= 1e-12 * scale, (name, float((g - want).abs().max()), scale)


@pytest.mark.parametrize("B,SL", [(3, 65), (3, 400)])
def test_one_wrong_route_moves_every_gradient_far_past_the_gate(B, SL):
    """A pure misroute - what the GPU test test_gate_catches_one_wrong_route hands umpr_coattention_bwd: EVERY column of
    sample 0 in turn has its ROUTE moved to the float64 runner-up row while the maxima, soft_* and the 1 - max^2 factors stay
    those of the right decisions (backward64's saved_at).  For every such move the gate's own figure - the worse of the two
    distances over the floored distance of the float32 yardstick - exceeds 10 x 14 on dGu, dGi and dM alike, so the gate,
    whose factor never exceeds 14, sits at least tenfold below one wrong route whichever route it is.  Measured weakest
    column (the one with the smallest |dS_col|): 400x / 496x / 757x (dM / dGi / dGu) at SL = 65, 701x and more at SL = 400.
    The BETTER of the two distances is logged in `both`: it exceeds 140x for all 400 columns at SL = 400 (weakest 274x) and
    for 64 of the 65 at SL = 65 - the column whose weight is 25x smaller than the next one's moves the relative L2 of dGu
    and dGi by 110x only.  (Letting the move change the maxima too, as a forward that picked the wrong index would, moves
    everything several times further.)"""
    x = C.make_inputs(B, SL)
    T64, A64 = _scores(x)
    ac, ar = A64.argmax(1), A64.argmax(2)
    ref, ref32 = _refs(x, T64, A64, ac, ar)
    floors = [tuple(max(d, C.FLOOR) for d in C.distances(r32, r)) for r32, r in zip(ref32, ref)]
    up = (x["d_atte_u"], x["d_atte_i"], x["d_soft_u"], x["d_soft_i"])
    worst, both, n_both = [float("inf")] * 3, [float("inf")] * 3, 0
    for k in range(SL):
        first, second = C.runner_up(A64, 0, k)
        assert first == int(ac[0, k])
        moved_ac = ac.clone()
        moved_ac[0, k] = second
        moved = C.backward64(x["Gu"], x["Gi"], x["M"], T64, A64, moved_ac, ar, *up, saved_at=(ac, ar))
        ok, rows = C.gate(moved, ref, ref32, K=C.K_MAX)
        assert not ok and all(r["over"] >= 10 for r in rows), (k, rows)
        col_both = []
        for t in range(3):
            d = C.distances(moved[t], ref[t])
            worst[t] = min(worst[t], max(d[0] / floors[t][0], d[1] / floors[t][1]))
            col_both.append(min(d[0] / floors[t][0], d[1] / floors[t][1]))
            both[t] = min(both[t], col_both[t])
        n_both += min(col_both) > 10 * C.K_MAX
    print(f"SL={SL}: weakest column, worse distance / floor {worst}, better distance / floor {both}; "
          f"{n_both} of {SL} columns beyond 140x in both distances")
    assert min(worst) > 10 * C.K_MAX, worst
    assert n_both >= SL - 1 and min(both) > 100, (n_both, both)
    # the same move with the maxima moved along is further away still, and the yardstick itself passes at K = 1
    moved_all = C.backward64(x["Gu"], x["Gi"], x["M"], T64, A64, moved_ac, ar, *up)
    assert all(C.distances(a, r)[1] >= C.distances(m, r)[1] for a, m, r in zip(moved_all, moved, ref))
    ok, rows = C.gate(ref32, ref, ref32, K=1.0)
    assert ok, rows


@pytest.mark.parametrize("B,SL", C.SHAPES)
def test_check_decisions_accepts_float32_argmax_and_rejects_a_clear_loser(B, SL):
    """The float32 CPU evaluation's argmax and maxima pass (inputs not saturated); an index whose float64 value lies
    5 delta below the maximum is rejected, one that lies delta / 2 below is accepted; an index outside [0, SL) and a saved
    maximum 2 delta off its score are rejected."""
    x = C.make_inputs(B, SL)
    T64, A64 = _scores(x)
    assert float(A64.max(1).values.abs().max()) <= 0.99 and float(A64.max(2).values.abs().max()) <= 0.99
    A32 = torch.tanh((x["Gi"] @ x["M"]) @ x["Gu"].transpose(-1, -2))
    saved = [A32.argmax(1).int(), A32.max(1).values, A32.argmax(2).int(), A32.max(2).values]
    fails, stats = C.check_decisions(A64, T64, x["Gu"], *saved)
    assert not fails, fails
    assert max(max(v) for v in stats.values()) < 0.1, stats         # float32 sits far inside the a-priori bound
    delta = C.rounding_delta(T64, x["Gu"])
    for side in (0, 1):                                             # 0: a column's decision, 1: a row's
        bad = [t.clone() for t in saved]
        bad[2 * side][B - 1, SL - 1] = SL
        assert C.check_decisions(A64, T64, x["Gu"], *bad)[0]
        bad = [t.clone() for t in saved]
        bad[2 * side][B - 1, 0] = -1
        assert C.check_decisions(A64, T64, x["Gu"], *bad)[0]
        bad = [t.clone() for t in saved]
        p = SL // 2
        w = int(saved[2 * side][0, p])
        d = float(delta[0, w, p] if side == 0 else delta[0, p, w])
        bad[2 * side + 1][0, p] += 2 * d
        assert C.check_decisions(A64, T64, x["Gu"], *bad)[0]
    if SL == 1:
        return
    # a second candidate placed a chosen distance below the winner of column / row p (delta does not depend on A64)
    for side in (0, 1):
        p = SL // 2
        w = int(A64[0, :, p].argmax() if side == 0 else A64[0, p, :].argmax())
        o = (w + 1) % SL
        at = (lambda q: (0, q, p)) if side == 0 else (lambda q: (0, p, q))
        d_hi, d_lo = max(float(delta[at(w)]), float(delta[at(o)])), min(float(delta[at(w)]), float(delta[at(o)]))
        for gap, accept in ((5 * d_hi, False), (0.5 * d_lo, True)):
            A = A64.clone()
            A[at(o)] = A[at(w)] - gap
            alt = [t.clone() for t in saved]
            alt[2 * side][0, p] = o
            alt[2 * side + 1][0, p] = float(A[at(o)])
            # the other side's maxima see the altered entry too: check this side only
            fails = [f for f in C.check_decisions(A, T64, x["Gu"], *alt)[0] if ("col" in f) == (side == 0)]
            assert bool(fails) != accept, (side, gap, fails)


def test_distances_and_gate_edges():
    """A reference that is identically zero is matched by exact zero only; NaN fails; K above 14 is refused."""
    z = torch.zeros(4, 4)
    assert C.distances(z, z) == (0.0, 0.0)
    assert C.distances(z + 1e-30, z)[0] == float("inf")
    r = torch.arange(16.0).reshape(4, 4).double()
    ok, rows = C.gate([r.float(), r.float(), z], [r, r, z.double()], [r.float(), r.float(), z])
    assert ok and all(row["ratio"] == 0 for row in rows)
    bad = r.float().clone()
    bad[0, 0] = float("nan")
    assert not C.gate([bad], [r], [r.float()], names=("x",))[0]
    assert not C.gate([r.float() * (1 + 8 * C.FLOOR)], [r], [r.float()], names=("x",))[0]
    assert C.gate([r.float() * (1 + 2 * C.FLOOR)], [r], [r.float()], names=("x",))[0]
    with pytest.raises(AssertionError):
        C.gate([r.float()], [r], [r.float()], names=("x",), K=15)
    assert C.K <= C.K_MAX
