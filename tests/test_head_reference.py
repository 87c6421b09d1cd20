"""tests/head_reference.py on the CPU: the hand-written float64 forward and backward of the visual head, the review merge and the
BCE head against float64 autograd of the formulas tests/test_gpu_parity.py states (test_head, test_review_merge,
test_bce_head_kernel), the margins of every case, and the gate against five deliberately wrong variants.  No GPU."""
from types import SimpleNamespace

import pytest
import torch
import torch.nn.functional as F

import head_reference as HR

_ids = lambda s: "-".join(map(str, s)) if isinstance(s, tuple) else str(s)      # noqa: E731
_REFS = {}


def _refs(shape):
    """(case, float64 forward, float32 forward) of one head case, computed once; both take their own decisions"""
    if shape not in _REFS:
        case = HR.make_head_case(*shape)
        _REFS[shape] = (case, HR.head_forward64(case), HR.head_forward64(case, torch.float32))
    return _REFS[shape]


def _close(name, got, want, tol=1e-12):
    d = HR.distances(got, want)
    assert max(d) <= tol, (name, d)


def _head_autograd(case, d_loss, d_pred):
    """test_head's formulas in float64 on leaf copies: (outputs as a dict, the twelve gradients as a dict)"""
    B, V, P = case.B, case.V, case.P
    leaf = lambda t: t.double().requires_grad_(True)        # noqa: E731
    rr, fw, fb = leaf(case.rr), leaf(case.fus_w), leaf(case.fus_b)
    labels = case.labels.double()
    o = {}
    if V:
        c_u, c_i, pp, pn, vgg, pos_v, neg_v, lw, lb = [leaf(t) for t in (case.c_u, case.c_i, case.pp, case.pn, case.vgg, case.pos_v,
                                                                          case.neg_v, case.lin_w, case.lin_b)]
        lw2 = lw.unsqueeze(0)
        img = vgg.view(B, V, P, -1).mean(-2)
        ie = F.linear(img, lw2, lb).squeeze(-1)
        pe, ne = F.linear(pos_v, lw2, lb).squeeze(-1), F.linear(neg_v, lw2, lb).squeeze(-1)
        pm, nm = torch.tanh((pe - ie).abs()), torch.tanh((ne - ie).abs())
        feat = torch.cat([rr, c_u * c_i * (1 - pm), c_u * c_i * (1 - nm)], -1)
        z = F.linear(feat, fw.unsqueeze(0), fb).squeeze(-1)
        pred = F.relu(z)
        loss_r = F.mse_loss(pred, labels)
        loss_v = torch.mean(pp.transpose(-1, -2) @ pm + pn.transpose(-1, -2) @ nm)
        ins = dict(zip(HR.HEAD_GRADS, (rr, c_u, c_i, pp, pn, vgg, pos_v, neg_v, lw, lb, fw, fb)))
        o.update(img_emb=ie, pos_match=pm, neg_match=nm, posneg_emb=torch.stack([pe, ne]))
    else:
        z = F.linear(rr, fw.unsqueeze(0), fb).squeeze(-1)
        pred = F.relu(z)
        loss_r, loss_v = F.mse_loss(pred, labels), torch.zeros((), dtype=torch.float64)
        ins = dict(zip(HR.HEAD_GRADS_V0, (rr, fw, fb)))
    loss = loss_r + case.rate * loss_v
    o.update(z=z, pred=pred, loss=torch.stack([loss, loss_r, loss_v]))
    total = d_loss * loss
    if d_pred is not None:
        total = total + (d_pred.double() * pred).sum()
    total.backward()
    grads = {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in ins.items()}
    return {k: v.detach() for k, v in o.items()}, grads


# call forms: (d_loss, d_pred given)
FORMS = {"loss_only": (0.7, False), "loss_and_pred": (0.7, True), "pred_only": (0.0, True)}


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", HR.HEAD_CASES, ids=_ids)
def test_head_matches_autograd(shape, form):
    """Every output and all twelve gradients (three at V = 0) to 1e-12 of each tensor's maximum, for d_pred = NULL, d_pred given
    and d_pred given with d_loss = 0; the reference is handed autograd's own decisions."""
    case, f64, _ = _refs(shape)
    d_loss, with_pred = FORMS[form]
    d_pred = case.d_pred if with_pred else None
    outs, grads = _head_autograd(case, d_loss, d_pred)
    dec = HR.head_decisions(outs["z"], outs.get("posneg_emb"), outs.get("img_emb"))
    f = HR.head_forward64(case, torch.float64, dec)
    for name, want in outs.items():
        _close(f"{case.tag} {name}", getattr(f, name), want)
    got = HR.head_backward64(case, dec, d_loss, d_pred, fwd=f)
    names = HR.head_grad_names(case)
    assert [k for k in got if k != "_parts"] == list(names)
    for name in names:
        if name == "d_lin_b":          # exactly zero in exact arithmetic: a rounding residue on both sides
            bound = 1e-12 * float(got["_parts"].dimg.abs().sum() + 1)
            assert abs(float(got[name])) <= bound and abs(float(grads[name])) <= bound, (float(got[name]), float(grads[name]))
            continue
        assert got[name].shape == grads[name].reshape(got[name].shape).shape
        _close(f"{case.tag} {form} {name}", got[name], grads[name].reshape(got[name].shape))
    if case.V and d_loss == 0:
        assert float(got["d_pp"].abs().max()) == 0 and float(got["d_pn"].abs().max()) == 0


@pytest.mark.parametrize("shape", HR.HEAD_CASES, ids=_ids)
def test_head_margins(shape):
    """No float64 z, pos_emb - img_emb or neg_emb - img_emb within MARGIN of zero, so the GPU tests exclude no row and no element;
    the float32 evaluation takes the same decisions; z > 0 at B = 1, both signs from B = 3 on, and 30% - 55% of the rows negative
    from B = 33 on; d_pred has zero rows from B = 2 on and a non-zero row that the ReLU lets through everywhere."""
    case, f64, f32 = _refs(shape)
    mz, md = HR.head_margins(case, f64)
    neg = float((f64.z < 0).double().mean())
    print(f"{case.tag}: min |z| = {mz:.3e}, min |difference| = {md:.3e}, z < 0 in {neg:.0%} of the rows")
    assert mz > HR.MARGIN and md > HR.MARGIN, (mz, md)
    assert torch.equal(f64.decisions.zpos, f32.decisions.zpos)
    if case.V:
        assert torch.equal(f64.decisions.sgp, f32.decisions.sgp) and torch.equal(f64.decisions.sgn, f32.decisions.sgn)
        assert float(f64.decisions.sgp.abs().min()) == 1 and float(f64.decisions.sgn.abs().min()) == 1
        assert case.vgg.shape == (case.B * case.V * case.P, HR.F) and case.lin_w.shape == (HR.F,)
    if case.B == 1:
        assert neg == 0
    elif case.B >= 33:
        assert 0.30 <= neg <= 0.55, neg
    else:
        assert 0 < neg < 1, neg
    assert 1 <= float(case.labels.min()) and float(case.labels.max()) <= 5
    assert bool((f64.decisions.zpos & (case.d_pred != 0)).any()) and (case.B == 1 or bool((case.d_pred == 0).any()))


def test_head_cases_cover_the_lds_bound():
    """the last case is the largest B the ABI's LDS formula accepts at V = 4, computed from the formula"""
    B, V, P = HR.HEAD_CASES[-1]
    assert (V, P) == (4, 1) and B == HR.largest_b(4)
    assert HR.head_lds_bytes(B, V) <= HR.LDS_LIMIT < HR.head_lds_bytes(B + 1, V)
    assert len(HR.HEAD_CASES) == 13


def _gate_all(case, tag, got_f, got_g, f64, g64, f32, g32, lines):
    """every output and gradient of a (forward, backward) pair through the gates the GPU tests use: (all passed, worst distance /
    bound)"""
    rows = []
    for name in ("z", "pred", "loss") + (("img_emb", "posneg_emb") if case.V else ()):
        rows += HR.gate([getattr(got_f, name)], [getattr(f64, name)], [getattr(f32, name)], names=[name], K=HR.k_of(name),
                        log=lines.append, tag=tag)[1]
    for name in (("pos_match", "neg_match") if case.V else ()):
        rows.append(HR.gate_abs(getattr(got_f, name), getattr(f64, name), getattr(f32, name), name, K=HR.k_of(name),
                                log=lines.append, tag=tag))
    for name in HR.head_grad_names(case):
        if name == "d_lin_b":
            rows.append(HR.gate_lin_b(got_g[name], g32[name], g64["_parts"], K=HR.k_of(name), log=lines.append, tag=tag))
        else:
            rows += HR.gate([got_g[name]], [g64[name]], [g32[name]], names=[name], K=HR.k_of(name), log=lines.append, tag=tag)[1]
    return all(r["ok"] for r in rows), max(r["over"] for r in rows), rows


@pytest.mark.parametrize("shape", HR.HEAD_CASES, ids=_ids)
def test_float32_yardstick_is_inside_the_starting_gate(shape):
    """On every case the float32 evaluation passes its own gate (ratio <= 1 by construction) and its distances are of float32
    rounding size: what the yardstick credits is rounding, nothing else."""
    case, f64, f32 = _refs(shape)
    g64 = HR.head_backward64(case, f64.decisions, case.d_loss, case.d_pred, fwd=f64)
    g32 = HR.head_backward64(case, f32.decisions, case.d_loss, case.d_pred, torch.float32, fwd=f32)
    lines = []
    ok, worst, rows = _gate_all(case, case.tag, f32, g32, f64, g64, f32, g32, lines)
    print("\n".join(lines))
    assert ok and all(r["ratio"] <= 1 for r in rows)
    for r in rows:
        if r["name"] != "d_lin_b":
            assert r["r_max"] <= 1e-5, r


VARIANTS = ("relu_flip", "abs_sign_flip", "mean_p_minus_1", "d_pred_row_dropped", "dfw_one_row_short")


@pytest.mark.parametrize("variant,shape", [
    ("relu_flip", (33, 0, 0)), ("relu_flip", (64, 4, 2)), ("relu_flip", (1153, 4, 1)),
    ("abs_sign_flip", (5, 3, 1)), ("abs_sign_flip", (64, 4, 2)), ("abs_sign_flip", (1153, 4, 1)),
    ("mean_p_minus_1", (3, 4, 2)), ("mean_p_minus_1", (4, 1, 3)), ("mean_p_minus_1", (64, 4, 2)),
    ("d_pred_row_dropped", (33, 0, 0)), ("d_pred_row_dropped", (257, 2, 1)), ("d_pred_row_dropped", (1153, 4, 1)),
    ("dfw_one_row_short", (257, 0, 0)), ("dfw_one_row_short", (64, 4, 2)), ("dfw_one_row_short", (1153, 4, 1))])
def test_gate_rejects_wrong_variants(variant, shape):
    """Each error, evaluated in float64 from the reference alone (no rounding of its own), is outside the gate at the GPU tests' K
    by a factor of at least 10: one flipped z > 0 (the row with the smallest |z|: the likeliest wrong decision), one flipped sign
    under the abs (the element with the smallest difference), a mean over P that divides by P - 1, one dropped d_pred row, d_fus_w
    summed over one row less."""
    assert shape in HR.HEAD_CASES
    case, f64, f32 = _refs(shape)
    dec = f64.decisions
    g64 = HR.head_backward64(case, dec, case.d_loss, case.d_pred, fwd=f64)
    g32 = HR.head_backward64(case, f32.decisions, case.d_loss, case.d_pred, torch.float32, fwd=f32)
    wf, kw, wdec, d_pred = f64, {}, dec, case.d_pred
    if variant == "relu_flip":
        b = int(f64.z.abs().argmin())
        zpos = dec.zpos.clone()
        zpos[b] = ~zpos[b]
        wdec = SimpleNamespace(zpos=zpos, sgp=dec.sgp, sgn=dec.sgn)          # the backward's mask alone: the forward is right
    elif variant == "abs_sign_flip":
        dp = (f64.posneg_emb[0] - f64.img_emb).abs()
        b, v = divmod(int(dp.argmin()), case.V)
        sgp = dec.sgp.clone()
        sgp[b, v] = -sgp[b, v]
        wdec = SimpleNamespace(zpos=dec.zpos, sgp=sgp, sgn=dec.sgn)          # the backward's sign alone
    elif variant == "mean_p_minus_1":
        assert case.P >= 2
        wf = HR.head_forward64(case, torch.float64, dec, wrong=variant)
    elif variant == "d_pred_row_dropped":
        live = torch.nonzero(dec.zpos & (case.d_pred != 0)).reshape(-1)
        d_pred = case.d_pred.clone()
        d_pred[int(live[-1])] = 0
    else:
        kw = {"wrong": variant}
    wg = HR.head_backward64(case, wdec, case.d_loss, d_pred, fwd=wf, **kw)
    lines = []
    ok, worst, rows = _gate_all(case, f"{case.tag} {variant}", wf, wg, f64, g64, f32, g32, lines)
    print("\n".join(l for l in lines if l.endswith("OUTSIDE")))
    print(f"{case.tag} {variant}: worst distance / bound = {worst:.1f}x")
    assert not ok
    assert worst >= 10, worst


# ------------------------------------------------------------------------------------------------------- review merge
@pytest.mark.parametrize("B", HR.MERGE_CASES)
def test_merge_matches_autograd(B):
    """tanh(linear_u(repr_u) + linear_i(repr_i)) of test_review_merge in float64: forward and four gradients to 1e-12"""
    case = HR.make_merge_case(B)
    leaves = [t.double().requires_grad_(True) for t in (case.ru, case.ri, case.Wu, case.Wi)]
    out = torch.tanh(F.linear(leaves[0], leaves[2]) + F.linear(leaves[1], leaves[3]))
    out.backward(case.d_out.double())
    ref = HR.merge_forward64(case)
    _close(f"{case.tag} out", ref, out.detach())
    for name, got, leaf in zip(HR.MERGE_GRADS, HR.merge_backward64(case, case.d_out, out=ref), leaves):
        _close(f"{case.tag} {name}", got, leaf.grad)
    ref32 = HR.merge_forward64(case, torch.float32)
    assert ref32.dtype == torch.float32 and float((ref32.double() - ref).abs().max()) <= 5e-6   # 512-term float32 sums


# ------------------------------------------------------------------------------------------------------- BCE head
@pytest.mark.parametrize("with_d_result", [False, True], ids=["d_result_null", "d_result_given"])
@pytest.mark.parametrize("shape", HR.BCE_CASES, ids=_ids)
def test_bce_matches_autograd(shape, with_d_result):
    """sigmoid(Linear(K -> 1)) + BCELoss(mean) of test_bce_head_kernel in float64.  The reference rounds p to float32 where the
    kernel stores it, so autograd is cut at that point: torch's binary_cross_entropy (with its -100 clamp and its 1e-12
    denominator) is differentiated with respect to the rounded p, sigmoid's derivative p (1 - p) is taken at the rounded p, and
    autograd carries dz through the linear layer.  Everything to 1e-12."""
    case = HR.make_bce_case(*shape)
    res, loss, z = HR.bce_forward64(case)
    att, w, b = [t.double().requires_grad_(True) for t in (case.att, case.w, case.b)]
    z_ag = att @ w + b
    _close(f"{case.tag} z", z, z_ag.detach())
    p = torch.sigmoid(z_ag).detach().float().double().requires_grad_(True)
    assert torch.equal(p.detach().float(), res)
    loss_ag = F.binary_cross_entropy(p, case.target.double())
    _close(f"{case.tag} loss", loss, loss_ag.detach())
    total = case.d_loss * loss_ag
    d_result = case.d_result if with_d_result else None
    if with_d_result:
        total = total + (case.d_result.double() * p).sum()
    total.backward()
    z_ag.backward(p.grad * p.detach() * (1 - p.detach()))
    got = HR.bce_backward64(case, res, case.d_loss, d_result)
    for name, g, want in zip(HR.BCE_GRADS, got, (att.grad, w.grad, b.grad)):
        _close(f"{case.tag} {name}", g, want)


@pytest.mark.parametrize("shape", HR.BCE_CASES, ids=_ids)
def test_bce_cases(shape):
    """Every row at |z| < 10 or |z| > 30; from B = 3 on one row with p == 1.0f and one towards 0 whose p (1 - p) is under the 1e-12
    denominator, from B = 5 on one with p == 0.0f; the float32 evaluation saturates the same rows; binary and soft targets both
    occur among the cases; on the unsaturated rows the rounded-p reference is within float32 rounding of plain float64 autograd."""
    case = HR.make_bce_case(*shape)
    res, loss, z = HR.bce_forward64(case)
    res32, loss32, z32 = HR.bce_forward64(case, torch.float32)
    az = z.abs()
    assert bool(((az < 10) | (az > 30)).all())
    sat = az > 30
    assert int(sat.sum()) == case.n_sat
    assert torch.equal(sat, z32.abs() > 30)
    if case.B >= 3:
        assert float(res[0]) == 1.0 and 0 < float(res[1]) < 1e-12 and float(res32[0]) == 1.0 and 0 < float(res32[1]) < 1e-12
    if case.B >= 5:
        assert float(res[2]) == 0.0 and float(res32[2]) == 0.0
    assert bool(torch.isfinite(loss)) and bool(torch.isfinite(loss32))
    if case.binary:
        assert bool(((case.target == 0) | (case.target == 1)).all())
    else:
        assert bool(((case.target >= 0) & (case.target <= 1)).all()) and (case.B < 3 or bool(((case.target > 0) & (case.target < 1)).any()))
    kinds = {HR.make_bce_case(*s).binary for s in HR.BCE_CASES}
    assert kinds == {True, False}
    att = case.att.double().requires_grad_(True)
    p = torch.sigmoid(att @ case.w.double() + case.b.double())
    (case.d_loss * F.binary_cross_entropy(p, case.target.double())).backward()
    got = HR.bce_backward64(case, res, case.d_loss)[0]
    live = ~sat
    assert float((got[live] - att.grad[live]).abs().max()) <= 1e-5 * float(att.grad[live].abs().max())


# ------------------------------------------------------------------------------------------------------- evaluation accumulator
@pytest.mark.parametrize("n", HR.SQ_ERR_CASES)
def test_sq_err_reference(n):
    """the float64 sum of the float32 squares is what mse_loss(reduction='sum') adds up, batch after batch, on top of the preload"""
    case = HR.make_sq_err_case(n)
    a0, a1 = HR.sq_err_reference(case)
    want = case.preload[0] + sum(float(F.mse_loss(p, l, reduction="none").double().sum()) for p, l in case.batches)
    assert abs(a0 - want) <= 1e-12 * want and a1 == case.preload[1] + 2 * n
    assert case.preload[0] != 0 and case.preload[1] != 0
