"""R-Net co-attention through the stage-level C ABI (umpr_coattention_fwd, umpr_coattention_fwd_bf16, umpr_coattention_bwd)
against the decision-conditioned float64 reference of tests/coattn_decisions.py.

The forward's saved decisions (argcol / argrow with colmax / rowmax) are each checked against float64 scores within the
a-priori rounding of a float32 evaluation; the softmax and context outputs are recomputed in float64 FROM those decisions;
and the backward, which is smooth once the decisions are given, is held to K x the distance the float32 CPU evaluation of
the same formula has from float64 (C.gate, K = 4, never above 14) - two to three orders of magnitude below what one wrong
route moves (test_gate_catches_one_wrong_route).  Inputs are not saturated (|maximum| <= 0.99 is asserted), so the routed
term, which carries the factor 1 - max^2, is alive in every case but the one forward-only saturated case.  Every distance
is logged to coattn.log beside the parity tests' log.
"""
import os
from types import SimpleNamespace

import pytest
import torch

import coattn_decisions as C
from test_gpu_parity import LOG as PARITY_LOG
from test_gpu_parity import L, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "coattn.log")
D = C.D
ENTRY = {"fp32": "umpr_coattention_fwd", "bf16": "umpr_coattention_fwd_bf16"}
_CASES = {}


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _hip_forward(L, dev, x, entry):
    """The forward entry on NaN-filled outputs and a NaN-filled workspace; atte_u goes to columns 0..127 of a NaN-filled
    [B][256] buffer, atte_i to columns 128..255 of another (ld = 256, the concat layout of src/model.py:166-167)."""
    B, SL, _ = x["Gu"].shape
    d = {k: x[k].to(dev).contiguous() for k in ("Gu", "Gi", "M")}
    o = SimpleNamespace(T=_nan(dev, B, SL, D), soft_u=_nan(dev, B, SL), soft_i=_nan(dev, B, SL), colmax=_nan(dev, B, SL),
                        rowmax=_nan(dev, B, SL), rep_u=_nan(dev, B, 2 * D), rep_i=_nan(dev, B, 2 * D),
                        argcol=torch.full((B, SL), -7, dtype=torch.int32, device=dev),
                        argrow=torch.full((B, SL), -7, dtype=torch.int32, device=dev), **d)
    wsb = L.size("umpr_coattention_fwd_ws_bytes", B, SL)
    ws = _nan(dev, wsb // 4 + 64)
    L.call(ENTRY[entry], o.Gu, o.Gi, o.M, B, SL, o.T, o.soft_u, o.soft_i, o.rep_u, 2 * D, o.rep_i.data_ptr() + D * 4, 2 * D,
           o.colmax, o.argcol, o.rowmax, o.argrow, ws, wsb, st())
    torch.cuda.synchronize()
    return o


def _hip_backward(L, dev, c, with_soft=True, prefill=None, argcol=None):
    """umpr_coattention_bwd on the HIP forward's saved tensors.  The upstream context gradients sit in NaN-filled [B][256]
    buffers (ld = 256) at column offsets 0 and 128; dM and - unless prefilled for accumulate = 1 - dGu, dGi are NaN-filled,
    and so is the workspace.  Returns CPU copies (dGu, dGi, dM)."""
    o, x = c.hip, c.x
    B, SL, _ = x["Gu"].shape
    du, di = _nan(dev, B, 2 * D), _nan(dev, B, 2 * D)
    du[:, :D] = x["d_atte_u"].to(dev)
    di[:, D:] = x["d_atte_i"].to(dev)
    dsu = x["d_soft_u"].to(dev).contiguous() if with_soft else None
    dsi = x["d_soft_i"].to(dev).contiguous() if with_soft else None
    dGu = prefill[0].to(dev).contiguous() if prefill else _nan(dev, B, SL, D)
    dGi = prefill[1].to(dev).contiguous() if prefill else _nan(dev, B, SL, D)
    dM = _nan(dev, D, D)
    wsb = L.size("umpr_coattention_bwd_ws_bytes", B, SL)
    ws = _nan(dev, wsb // 4 + 64)
    L.call("umpr_coattention_bwd", o.Gu, o.Gi, o.M, o.T, o.soft_u, o.soft_i, o.colmax, o.argcol if argcol is None else argcol,
           o.rowmax, o.argrow, du, 2 * D, di.data_ptr() + D * 4, 2 * D, dsu, dsi, B, SL, dGu, dGi, dM, 1 if prefill else 0,
           ws, wsb, st())
    torch.cuda.synchronize()
    return dGu.cpu(), dGi.cpu(), dM.cpu()


def _case(L, dev, key, x, entry):
    """HIP forward of the inputs x through `entry`, the float64 scores its decisions are judged by, and - once the decisions
    are inside their range - the float64 reference and float32 yardstick of the backward conditioned on them.  Computed once
    per (key, entry) and shared by the tests; nothing in it is modified afterwards."""
    if (key, entry) in _CASES:
        return _CASES[key, entry]
    c = SimpleNamespace(x=x, entry=entry, tag=f"{key} {entry}")
    c.hip = o = _hip_forward(L, dev, x, entry)
    Gu, Gi, M = x["Gu"], x["Gi"], x["M"]
    c.T64 = Gi.double() @ M.double()
    T_hip = o.T.cpu()
    if entry == "fp32":
        # float64 from the inputs; the routed products use the same T
        c.T_scores, c.Gu_scores, c.T_route = c.T64, Gu, c.T64
        T32 = Gi @ M
        A32 = torch.tanh(T32 @ Gu.transpose(-1, -2))
    else:
        # the bf16-rounded values of the HIP T and of Gu: their products are exact in float32, only accumulation differs;
        # the routed products use the unrounded HIP T
        c.T_scores, c.Gu_scores, c.T_route = C.bf16_round(T_hip), C.bf16_round(Gu), T_hip.double()
        T32 = T_hip
        A32 = torch.tanh(c.T_scores @ c.Gu_scores.transpose(-1, -2))
    c.A64 = C.scores64(c.T_scores, c.Gu_scores)
    c.argcol, c.argrow, c.colmax, c.rowmax = o.argcol.cpu(), o.argrow.cpu(), o.colmax.cpu(), o.rowmax.cpu()
    c.fails, c.stats = C.check_decisions(c.A64, c.T_scores, c.Gu_scores, c.argcol, c.colmax, c.argrow, c.rowmax)
    log(f"{c.tag} decisions: " + " ".join(f"{s}: value error {v[0]:.3e} delta, argmax lead {v[1]:.3e} of the deltas"
                                          for s, v in c.stats.items()) + (f" FAILS {c.fails}" if c.fails else ""))
    SL = Gu.shape[1]
    c.in_range = bool(((c.argcol >= 0) & (c.argcol < SL) & (c.argrow >= 0) & (c.argrow < SL)).all())
    if c.in_range:
        up = (x["d_atte_u"], x["d_atte_i"])
        soft = (x["d_soft_u"], x["d_soft_i"])
        c.parts = {}
        c.ref = C.backward64(Gu, Gi, M, c.T_route, c.A64, c.argcol, c.argrow, *up, *soft, parts=c.parts)
        c.ref32 = C.backward64(Gu, Gi, M, T32, A32, c.argcol, c.argrow, *up, *soft, dtype=torch.float32)
        c.ref_nosoft = C.backward64(Gu, Gi, M, c.T_route, c.A64, c.argcol, c.argrow, *up)
        c.ref32_nosoft = C.backward64(Gu, Gi, M, T32, A32, c.argcol, c.argrow, *up, dtype=torch.float32)
    _CASES[key, entry] = c
    return c


def _shape_case(L, dev, B, SL, entry):
    return _case(L, dev, f"B{B} SL{SL}", C.make_inputs(B, SL), entry)


def _assert_gate(c, tag, got, ref, ref32):
    ok, rows = C.gate(got, ref, ref32, log=log, tag=f"{c.tag} {tag}")
    assert ok, [(r["name"], r["d_max"], r["d_l2"], r["r_max"], r["r_l2"], r["ratio"]) for r in rows if not r["ok"]]


def _assert_alive(c):
    """no maximum saturated, and - wherever the softmax has more than one position to weigh - a non-zero dM reference"""
    SL = c.x["Gu"].shape[1]
    for m in (c.A64.max(1).values, c.A64.max(2).values):
        assert float(m.abs().max()) <= 0.99, float(m.abs().max())
    assert c.in_range, c.fails
    if SL > 1:
        assert float(c.ref[2].abs().max()) > 0
    else:       # one position: soft = 1 whatever the score, so dS = 0 and dM = 0 exactly (C.distances then demands exact zero)
        assert float(c.ref[2].abs().max()) == 0


@pytest.mark.parametrize("entry", ["fp32", "bf16"])
@pytest.mark.parametrize("B,SL", C.SHAPES)
def test_forward(L, dev, B, SL, entry):
    """T against float64 G_i M at test_gemm's bound (1e-5 sqrt(K) absolute + 1e-5 relative, K = 128); every saved decision
    against the float64 scores (C.check_decisions); soft_* and atte_* against float64 recomputed from the HIP decisions at
    2e-6 absolute; atte_* land in their half of the [B][256] concat buffer and the other half stays NaN."""
    c = _shape_case(L, dev, B, SL, entry)
    o = c.hip
    _assert_alive(c)
    T = o.T.cpu().double()
    assert torch.isfinite(T).all()
    err = (T - c.T64).abs()
    log(f"{c.tag} T: max_err={float(err.max()):.3e} ref_max={float(c.T64.abs().max()):.3e}")
    assert bool((err <= 1e-5 * D ** 0.5 + 1e-5 * c.T64.abs()).all()), float(err.max())
    assert not c.fails, c.fails
    cm, rm, su, si, au, ai = C.forward64(c.x["Gu"], c.x["Gi"], c.A64, c.argcol, c.argrow)
    rep_u, rep_i = o.rep_u.cpu(), o.rep_i.cpu()
    assert bool(torch.isnan(rep_u[:, D:]).all()) and bool(torch.isnan(rep_i[:, :D]).all()), "written outside the 128 columns"
    for name, got, want in (("soft_u", o.soft_u.cpu(), su), ("soft_i", o.soft_i.cpu(), si), ("atte_u", rep_u[:, :D], au),
                            ("atte_i", rep_i[:, D:], ai)):
        assert torch.isfinite(got).all(), name
        e = float((got.double() - want).abs().max())
        log(f"{c.tag} {name}: max_err={e:.3e} ref_max={float(want.abs().max()):.3e}")
        assert e <= 2e-6, (name, e)


@pytest.mark.parametrize("variant", ["plain", "no_d_soft", "accumulate"])
@pytest.mark.parametrize("entry", ["fp32", "bf16"])
@pytest.mark.parametrize("B,SL", C.SHAPES)
def test_backward(L, dev, B, SL, entry, variant):
    """umpr_coattention_bwd on the HIP forward's saved tensors, dGu / dGi / dM through C.gate against the float64 backward
    conditioned on the HIP decisions.  plain: all four upstream gradients.  no_d_soft: d_soft_u = d_soft_i = NULL, the
    reference with zeros.  accumulate: accumulate = 1 onto pre-filled dGu / dGi (randn scaled so that max |prefill| equals
    max |reference gradient| of that tensor and shape: the sum's scale and rounding stay the gradient's own, and the
    variant is as sharp as the plain one): prefill + gradient through the same gate, with the float32 yardstick summed the
    same way, and dM overwritten (it was NaN)."""
    c = _shape_case(L, dev, B, SL, entry)
    _assert_alive(c)
    if variant == "plain":
        _assert_gate(c, variant, _hip_backward(L, dev, c), c.ref, c.ref32)
    elif variant == "no_d_soft":
        _assert_gate(c, variant, _hip_backward(L, dev, c, with_soft=False), c.ref_nosoft, c.ref32_nosoft)
    else:
        g = torch.Generator().manual_seed(77 + SL)
        pre = [torch.randn(B, SL, D, generator=g) for _ in range(2)]
        pre = [p * (float(r.abs().max()) / float(p.abs().max())) for p, r in zip(pre, c.ref)]
        got = _hip_backward(L, dev, c, prefill=pre)
        ref = (pre[0].double() + c.ref[0], pre[1].double() + c.ref[1], c.ref[2])
        ref32 = (pre[0] + c.ref32[0], pre[1] + c.ref32[1], c.ref32[2])
        _assert_gate(c, variant, got, ref, ref32)


@pytest.mark.parametrize("B,SL", [(3, 65), (3, 400)])
def test_gate_catches_one_wrong_route(L, dev, B, SL):
    """One argcol entry - of sample 0, the column whose routed weight |dS_col| is the SMALLEST, i.e. the least visible one -
    is replaced by the float64 runner-up row (in range) and umpr_coattention_bwd runs on it: the gate against the unaltered
    reference fails, at 10x the bound or more on at least two of the three tensors."""
    c = _shape_case(L, dev, B, SL, "fp32")
    _assert_alive(c)
    assert not c.fails, c.fails
    k = int(c.parts["dS_col"][0].abs().argmin())
    first, second = C.runner_up(c.A64, 0, k)
    assert int(c.argcol[0, k]) == first and 0 <= second < SL and second != first
    wrong = c.hip.argcol.clone()
    wrong[0, k] = second
    got = _hip_backward(L, dev, c, argcol=wrong)
    ok, rows = C.gate(got, c.ref, c.ref32, log=log, tag=f"{c.tag} column {k} routed to row {second} instead of {first}")
    log(f"{c.tag} one wrong route: distance / bound = " + ", ".join(f"{r['name']} {r['over']:.1f}x" for r in rows))
    assert not ok
    assert sum(r["over"] >= 10 for r in rows) >= 2, [(r["name"], r["over"]) for r in rows]


@pytest.mark.parametrize("entry", ["fp32", "bf16"])
def test_ties_take_the_first_index(L, dev, entry):
    """(2, 130) with rows 3 and 70 of Gi identical and rows 5 and 129 of Gu identical (different 64-wide tiles): T rows 3 and
    70 are bit-identical, and wherever the float64 column maximum is attained at the duplicated rows argcol is 3, never 70;
    argrow is 5, never 129, for the duplicated columns - the first-occurrence rule of the header and better_first.  At least
    one column and one row have such a tie (seed chosen on the CPU), and the gate still passes."""
    B, SL = 2, 130
    x = C.make_inputs(B, SL, seed=7000)
    x["Gi"][:, 70] = x["Gi"][:, 3]
    x["Gu"][:, 129] = x["Gu"][:, 5]
    c = _case(L, dev, "ties B2 SL130", x, entry)
    T = c.hip.T.cpu()
    assert torch.equal(T[:, 3], T[:, 70])
    # identical operands: make the float64 scores identical to the bit, whatever the CPU matmul's blocking does
    assert float((c.A64[:, 70, :] - c.A64[:, 3, :]).abs().max()) <= 1e-13 and float((c.A64[:, :, 129] - c.A64[:, :, 5]).abs().max()) <= 1e-13
    A = c.A64.clone()
    A[:, 70, :] = A[:, 3, :]
    A[:, :, 129] = A[:, :, 5]
    col_tie = A[:, 3, :] == A.max(1).values
    row_tie = A[:, :, 5] == A.max(2).values
    log(f"{c.tag}: {int(col_tie.sum())} columns and {int(row_tie.sum())} rows have their maximum at the duplicated positions")
    assert int(col_tie.sum()) >= 1 and int(row_tie.sum()) >= 1
    assert not c.fails, c.fails
    assert bool((c.argcol[col_tie] == 3).all()) and bool((c.argcol != 70).all()), c.argcol[col_tie]
    assert bool((c.argrow[row_tie] == 5).all()) and bool((c.argrow != 129).all()), c.argrow[row_tie]
    _assert_alive(c)
    _assert_gate(c, "plain", _hip_backward(L, dev, c), c.ref, c.ref32)


@pytest.mark.parametrize("entry", ["fp32", "bf16"])
def test_saturated_forward(L, dev, entry):
    """(3, 400) with M = randn, the m_scale = 1.0 regime of test_review_head: most of A is +-1 in float32.  Forward only -
    every decision still passes C.check_decisions and every output is finite; no gradient claim, 1 - max^2 is 0 there."""
    x = C.make_inputs(3, 400, seed=99, m_scale=1.0)
    c = _case(L, dev, "saturated B3 SL400", x, entry)
    o = c.hip
    share = float((c.A64.abs() >= 1 - C.EPS32).double().mean())
    tied = float((torch.cat([c.colmax, c.rowmax]).abs() == 1).double().mean())
    log(f"{c.tag}: {share:.1%} of A saturated in float32, {tied:.1%} of the saved maxima exactly +-1")
    assert share > 0.5
    assert not c.fails, c.fails
    for name, t in (("T", o.T), ("soft_u", o.soft_u), ("soft_i", o.soft_i), ("colmax", o.colmax), ("rowmax", o.rowmax),
                    ("atte_u", o.rep_u[:, :D]), ("atte_i", o.rep_i[:, D:])):
        assert bool(torch.isfinite(t).all()), name
    assert bool(torch.isnan(o.rep_u[:, D:]).all()) and bool(torch.isnan(o.rep_i[:, :D]).all())
