"""The stages behind the text and visual paths through the C ABI - the visual head with linear_fusion and the losses (umpr_head_fwd /
_bwd), the review merge (umpr_review_merge_fwd / _bwd), the pre-training BCE head (umpr_bce_head_fwd / _bwd) and the evaluation
accumulator (umpr_sq_err_accumulate) - against the float64 references of tests/head_reference.py.

The head's decisions (z > 0 and the signs under the two abs) are compared with the float64 ones on every row and element - every
case keeps them MARGIN = 1e-4 away from zero, tests/test_head_reference.py asserts that - and the reference then replays the HIP
decisions.  Every output, saved tensor and gradient is held to K x the distance the float32 CPU evaluation of the same formulas has
from float64 (HR.k_of: 4 unless head_reference.py states otherwise, never above 14; floor 2^-22), three to six orders of magnitude
below what one wrong decision, a wrong divisor or one lost row moves (test_head_reference.py::test_gate_rejects_wrong_variants).
The cases are the smallest at which each stride, tail and grid edge of the kernels can go wrong, up to the largest batch the LDS
bound of umpr_head_bwd accepts.  Every call runs on NaN-filled outputs, gradients and workspaces.  Every distance is logged to
head.log beside the parity tests' log before it is judged.
"""
import os
from types import SimpleNamespace

import pytest
import torch

import head_reference as HR
from test_gpu_parity import LOG as PARITY_LOG
from test_gpu_parity import L, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "head.log")
F = HR.F
_CASES = {}
_ids = lambda s: "-".join(map(str, s)) if isinstance(s, tuple) else str(s)      # noqa: E731
# call forms of umpr_head_bwd: (d_loss, d_pred given)
FORMS = {"loss_only": (None, False), "loss_and_pred": (None, True), "pred_only": (0.0, True)}
HEAD_IN = ("rr", "c_u", "c_i", "pp", "pn", "vgg", "pos_v", "neg_v", "lin_w")      # the first nine pointers of both entry points


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _to(t, dev):
    return None if t is None else t.to(dev).contiguous()


class _Rows:
    """gate rows of one test: every tensor is logged when it is added, all are judged at the end"""

    def __init__(self, tag):
        self.tag, self.rows = tag, []

    def gate(self, name, got, ref, ref32, absolute=False):
        got = got.detach().cpu().reshape(ref.shape)
        k = HR.k_of(name)
        if absolute:
            self.rows.append(HR.gate_abs(got, ref, ref32, name, K=k, log=log, tag=self.tag))
        else:
            self.rows += HR.gate([got], [ref], [ref32], names=[name], K=k, log=log, tag=self.tag)[1]

    def lin_b(self, got, ref32, parts64):
        self.rows.append(HR.gate_lin_b(got, ref32, parts64, K=HR.k_of("d_lin_b"), log=log, tag=self.tag))

    def judge(self):
        bad = [(r["name"], r["d_max"], r["r_max"], r["ratio"]) for r in self.rows if not r["ok"]]
        assert not bad, (self.tag, bad)


# ------------------------------------------------------------------------------------------------------- head
def _hip_head_forward(L, dev, case):
    """umpr_head_fwd on NaN-filled pred, loss and saved buffers (at V = 0 the four visual buffers have one column, as
    _Head.forward allocates them).  Returns a namespace of device tensors: the inputs `ins` and every output."""
    B, V, P = case.B, case.V, case.P
    nv = max(V, 1)
    h = SimpleNamespace(ins=[_to(getattr(case, n), dev) for n in HEAD_IN], lin_b=_to(case.lin_b, dev), fus_w=_to(case.fus_w, dev),
                        fus_b=_to(case.fus_b, dev), labels=_to(case.labels, dev))
    h.pred, h.loss, h.z = _nan(dev, B), _nan(dev, 3), _nan(dev, B)
    h.img_emb, h.pos_match, h.neg_match, h.posneg_emb = _nan(dev, B, nv), _nan(dev, B, nv), _nan(dev, B, nv), _nan(dev, 2, nv)
    L.call("umpr_head_fwd", *h.ins, h.lin_b, h.fus_w, h.fus_b, h.labels, float(case.rate), B, V, P, h.pred, h.loss, h.z, h.img_emb,
           h.pos_match, h.neg_match, h.posneg_emb, st())
    torch.cuda.synchronize()
    return h


def _grad_buffers(dev, B, V, P):
    """the twelve NaN-filled gradient buffers in the ABI's order; at V = 0 the nine the call must not touch have V = P = 1"""
    v, p = max(V, 1), max(P, 1)
    shapes = ((B, HR.D), (B, v), (B, v), (B, v), (B, v), (B * v * p, F), (v, F), (v, F), (F,), (1,), (HR.D + 2 * V,), (1,))
    return dict(zip(HR.HEAD_GRADS, (_nan(dev, *s) for s in shapes)))


def _hip_head_backward(L, dev, case, h, d_loss, d_pred):
    """umpr_head_bwd on the HIP forward's own saved tensors and NaN-filled gradient buffers; returns the twelve buffers on the CPU"""
    B, V, P = case.B, case.V, case.P
    g = _grad_buffers(dev, B, V, P)
    gl = torch.tensor([d_loss], dtype=torch.float32, device=dev)
    L.call("umpr_head_bwd", *h.ins, h.fus_w, h.labels, float(case.rate), B, V, P, h.pred, h.z, h.img_emb, h.pos_match, h.neg_match,
           h.posneg_emb, gl, _to(d_pred, dev), *g.values(), st())
    torch.cuda.synchronize()
    return {k: t.cpu() for k, t in g.items()}


def _head_case(L, dev, shape):
    """One case: the HIP forward, the decisions it took, and the float64 reference / float32 yardstick replaying them.  Computed
    once per shape and shared by the tests; nothing in it is modified afterwards."""
    if shape in _CASES:
        return _CASES[shape]
    case = HR.make_head_case(*shape)
    c = SimpleNamespace(case=case, tag=case.tag, own=HR.head_forward64(case), hip=_hip_head_forward(L, dev, case))
    h = c.hip
    c.out = SimpleNamespace(**{n: getattr(h, n).cpu() for n in HR.HEAD_OUT})
    if case.V:
        c.dec = HR.head_decisions(c.out.z, c.out.posneg_emb, c.out.img_emb)
    else:
        c.dec = HR.head_decisions(c.out.z)
    c.dec_ok = not bool(torch.isnan(c.out.z).any()) and (not case.V or (float(c.dec.sgp.abs().min()) == 1 and float(c.dec.sgn.abs().min()) == 1))
    c.ref = c.ref32 = None
    _CASES[shape] = c
    return c


def _refs(c):
    """the forward references under the HIP decisions, once (only after the decisions were found sane: no NaN, no zero sign)"""
    assert c.dec_ok, f"{c.tag}: the HIP forward left NaN in z or a zero difference: no decisions to replay"
    if c.ref is None:
        c.ref = HR.head_forward64(c.case, torch.float64, c.dec)
        c.ref32 = HR.head_forward64(c.case, torch.float32, c.dec)
    return c.ref, c.ref32


@pytest.mark.parametrize("shape", HR.HEAD_CASES, ids=_ids)
def test_head_forward(L, dev, shape):
    """Nothing the call writes is NaN; at V = 0 the four visual buffers are still NaN.  The sign of the saved z and the signs of the
    saved posneg_emb - img_emb equal the float64 ones on every row and element, pred == max(z, 0) bit for bit, and pred, the three
    loss values and the five saved tensors are inside the gate."""
    c = _head_case(L, dev, shape)
    case, o = c.case, c.out
    visual = ("img_emb", "pos_match", "neg_match", "posneg_emb")
    for n in HR.HEAD_OUT:
        t = getattr(o, n)
        if n in visual and not case.V:
            assert bool(torch.isnan(t).all()), f"{c.tag}: {n} was written at V = 0"
        else:
            assert not bool(torch.isnan(t).any()), f"{c.tag}: NaN in {n}"
    own = c.own.decisions
    assert torch.equal(c.dec.zpos, own.zpos), f"{c.tag}: z > 0 differs from float64 in rows {torch.nonzero(c.dec.zpos != own.zpos).reshape(-1).tolist()}"
    if case.V:
        assert torch.equal(c.dec.sgp, own.sgp), f"{c.tag}: sign(pos_emb - img_emb) differs at {torch.nonzero(c.dec.sgp != own.sgp).tolist()}"
        assert torch.equal(c.dec.sgn, own.sgn), f"{c.tag}: sign(neg_emb - img_emb) differs at {torch.nonzero(c.dec.sgn != own.sgn).tolist()}"
    assert torch.equal(o.pred, o.z.clamp_min(0)), f"{c.tag}: pred is not max(z, 0)"
    assert bool((o.pred[~c.dec.zpos] == 0).all()) and torch.equal(o.pred[c.dec.zpos], o.z[c.dec.zpos])
    ref, ref32 = _refs(c)
    rows = _Rows(f"{c.tag} forward")
    for n in ("z", "pred", "loss") + (("img_emb", "posneg_emb") if case.V else ()):
        rows.gate(n, getattr(o, n), getattr(ref, n), getattr(ref32, n))
    for n in (("pos_match", "neg_match") if case.V else ()):
        rows.gate(n, getattr(o, n), getattr(ref, n), getattr(ref32, n), absolute=True)
    if not case.V:
        assert float(o.loss[2]) == 0 and float(o.loss[0]) == float(o.loss[1])
    rows.judge()


def _check_head_grads(c, tag, got, d_loss, d_pred):
    """the gradients `got` (dict of CPU tensors) of one call form against backward64 under the HIP decisions"""
    case = c.case
    ref, ref32 = _refs(c)
    g64 = HR.head_backward64(case, c.dec, d_loss, d_pred, fwd=ref)
    g32 = HR.head_backward64(case, c.dec, d_loss, d_pred, torch.float32, fwd=ref32)
    rows = _Rows(f"{c.tag} {tag}")
    for n in HR.head_grad_names(case):
        assert not bool(torch.isnan(got[n]).any()), f"{c.tag} {tag}: NaN in {n}"
        if n == "d_lin_b":
            rows.lin_b(got[n], g32[n], g64["_parts"])
        else:
            rows.gate(n, got[n], g64[n], g32[n])
    rows.judge()
    return g64


@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("shape", HR.HEAD_CASES, ids=_ids)
def test_head_backward(L, dev, shape, form):
    """umpr_head_bwd on the HIP forward's saved tensors and NaN-filled gradient buffers, with d_pred = NULL, with d_pred given, and
    with d_pred given and d_loss = 0: all twelve gradients finite and inside the gate (d_lin_b, exactly zero, against the float32
    evaluation's own residue); at V = 0 only d_rr, d_fus_w and d_fus_b are written and the nine other buffers are still NaN; with
    d_loss = 0 d_prefer_pos / d_prefer_neg are exactly zero; rows with z <= 0 have an exactly zero d_rr."""
    c = _head_case(L, dev, shape)
    case = c.case
    d_loss, with_pred = FORMS[form]
    d_loss = case.d_loss if d_loss is None else d_loss
    d_pred = case.d_pred if with_pred else None
    got = _hip_head_backward(L, dev, case, c.hip, d_loss, d_pred)
    if not case.V:
        for n in HR.HEAD_GRADS:
            if n not in HR.HEAD_GRADS_V0:
                assert bool(torch.isnan(got[n]).all()), f"{c.tag} {form}: {n} was written at V = 0"
    g64 = _check_head_grads(c, form, got, d_loss, d_pred)
    assert bool((got["d_rr"][~c.dec.zpos] == 0).all()), f"{c.tag} {form}: a row with z <= 0 has a gradient"
    if case.V and d_loss == 0:
        assert float(g64["d_pp"].abs().max()) == 0 and bool((got["d_pp"] == 0).all()) and bool((got["d_pn"] == 0).all())
    if d_pred is not None:
        live = c.dec.zpos & (d_pred != 0)
        assert bool(live.any()) and bool((got["d_rr"][live].abs().amax(1) > 0).all())


@pytest.mark.parametrize("with_loss", [True, False], ids=["loss_and_pred", "pred_only"])
@pytest.mark.parametrize("shape", [(5, 3, 1), (33, 0, 0)], ids=_ids)
def test_head_apply_with_a_prediction_gradient(L, dev, shape, with_loss):
    """_Head.apply, loss + (w * pred).sum() back-propagated: d_loss = 1 and d_pred = w reach umpr_head_bwd together; and
    (w * pred).sum() alone: autograd hands _Head.backward d_loss = None, which it must turn into a zero scalar.  pred, loss, the two
    logged loss terms and every leaf's gradient against the same reference (the float64 decisions: test_head_forward shows that
    they are the kernel's)."""
    from umpr_amd.model import _Head
    case = HR.make_head_case(*shape)
    own = HR.head_forward64(case)
    dec = own.decisions
    ref32 = HR.head_forward64(case, torch.float32, dec)
    w = case.d_pred
    leaf = lambda t: None if t is None else t.to(dev).requires_grad_(True)       # noqa: E731
    two_d = lambda t: None if t is None else t.unsqueeze(0)                      # noqa: E731  (nn.Linear's [1][n] weights)
    ins = [leaf(t) for t in (case.rr, case.c_u, case.c_i, case.pp, case.pn, case.vgg, case.pos_v, case.neg_v, two_d(case.lin_w),
                             case.lin_b, two_d(case.fus_w), case.fus_b)]
    pred, loss, terms = _Head.apply(*ins, case.labels.to(dev), case.rate, case.V, case.P)
    d_loss = 1.0 if with_loss else 0.0
    ((loss if with_loss else 0) + (w.to(dev) * pred).sum()).backward()
    torch.cuda.synchronize()
    rows = _Rows(f"{case.tag} _Head.apply {'loss + w.pred' if with_loss else 'w.pred'}")
    rows.gate("pred", pred, own.pred, ref32.pred)
    rows.gate("loss", torch.cat([loss.detach().reshape(1), terms.detach()]), own.loss, ref32.loss)
    g64 = HR.head_backward64(case, dec, d_loss, w, fwd=own)
    g32 = HR.head_backward64(case, dec, d_loss, w, torch.float32, fwd=ref32)
    for n, t in zip(HR.HEAD_GRADS, ins):
        if t is None:
            assert n not in g64
            continue
        assert t.grad is not None and not bool(torch.isnan(t.grad).any()), (case.tag, n)
        if n == "d_lin_b":
            rows.lin_b(t.grad.cpu(), g32[n], g64["_parts"])
        else:
            rows.gate(n, t.grad, g64[n], g32[n])
    rows.judge()


def test_head_bwd_lds_bound(L, dev):
    """(B + 3 B V + 2 V) * 4 <= 60000 at V = 4: the largest B of that formula is a case of the tests above (it runs and passes the
    gates); B + 1 is refused with the library's error before anything is launched - the NaN-filled gradient buffers, sized for
    B + 1, are still all NaN."""
    from umpr_amd._lib import UmprHipError
    V, P = 4, 1
    B = HR.largest_b(V)
    assert (B, V, P) in HR.HEAD_CASES and HR.head_lds_bytes(B, V) <= HR.LDS_LIMIT < HR.head_lds_bytes(B + 1, V)
    B += 1
    z = lambda *s: torch.zeros(*s, device=dev)              # noqa: E731
    ins = [z(B, HR.D), z(B, V), z(B, V), z(B, V), z(B, V), z(B * V * P, F), z(V, F), z(V, F), z(F)]
    g = _grad_buffers(dev, B, V, P)
    with pytest.raises(UmprHipError, match="batch too large"):
        L.call("umpr_head_bwd", *ins, z(HR.D + 2 * V), z(B), 0.1, B, V, P, z(B), z(B), z(B, V), z(B, V), z(B, V), z(2, V), z(1), None,
               *g.values(), st())
    assert "head_bwd" in L.last_error()
    torch.cuda.synchronize()
    for n, t in g.items():
        assert bool(torch.isnan(t).all()), n


# ------------------------------------------------------------------------------------------------------- review merge
@pytest.mark.parametrize("B", HR.MERGE_CASES)
def test_review_merge(L, dev, B):
    """umpr_review_merge_fwd / _bwd on the default route, on NaN-filled out, gradients and workspace, at both sides of the row
    groups of 4 and 32, of the 128-row pass of the weight gradient, and of the B = 256 / 257 switch to the GEMM route: out as
    largest absolute distance, the four gradients (of the HIP forward's own out) through the gate."""
    case = HR.make_merge_case(B)
    d = [t.to(dev) for t in (case.ru, case.ri, case.Wu, case.Wi)]
    out = _nan(dev, B, HR.MD)
    L.call("umpr_review_merge_fwd", *d, B, out, st())
    wsb = L.size("umpr_review_merge_bwd_ws_bytes", B)
    ws = _nan(dev, wsb // 4 + 64)
    grads = [_nan(dev, *t.shape) for t in d]
    L.call("umpr_review_merge_bwd", *d, out, case.d_out.to(dev), B, *grads, ws, ws.numel() * 4, st())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(out).any())
    ref, ref32 = HR.merge_forward64(case), HR.merge_forward64(case, torch.float32)
    rows = _Rows(case.tag)
    rows.gate("merge out", out, ref, ref32, absolute=True)
    g64 = HR.merge_backward64(case, case.d_out, out=ref)
    g32 = HR.merge_backward64(case, case.d_out, torch.float32, out=ref32)
    for n, got, r, r32 in zip(HR.MERGE_GRADS, grads, g64, g32):
        assert not bool(torch.isnan(got).any()), (case.tag, n)
        rows.gate("merge " + n, got, r, r32)
    rows.judge()


# ------------------------------------------------------------------------------------------------------- BCE head
PAD_ATT, PAD_D = 3, 5
SENTINEL = -7.25


@pytest.mark.parametrize("with_d_result", [False, True], ids=["d_result_null", "d_result_given"])
@pytest.mark.parametrize("shape", HR.BCE_CASES, ids=_ids)
def test_bce_head(L, dev, shape, with_d_result):
    """umpr_bce_head_fwd / _bwd with ld = K + 3 (NaN in the padding columns of att) and ld_d = K + 5 (a sentinel in the padding of
    d_att that must survive bit for bit), d_result NULL and given, on NaN-filled result, loss, gradients and workspace; rows with
    p == 1.0f, p = 4e-18 and p == 0.0f among the unsaturated ones.  result as largest absolute distance; loss, d_att, dw and db
    through the gate; the rows saturated to exactly 0 or 1 have an exactly zero d_att."""
    case = HR.make_bce_case(*shape)
    B, K = case.B, case.K
    att = _nan(dev, B, K + PAD_ATT)
    att[:, :K] = case.att.to(dev)
    w, b, tg = case.w.to(dev), case.b.to(dev), case.target.to(dev)
    res, loss, ws = _nan(dev, B), _nan(dev, 1), _nan(dev, B)
    L.call("umpr_bce_head_fwd", att, K + PAD_ATT, w, b, tg, B, K, res, loss, ws, B * 4, st())
    d_att = torch.full((B, K + PAD_D), SENTINEL, device=dev)
    d_att[:, :K] = float("nan")
    dw, db, ws2 = _nan(dev, K), _nan(dev, 1), _nan(dev, B)
    d_result = case.d_result if with_d_result else None
    gl = torch.tensor([case.d_loss], dtype=torch.float32, device=dev)
    L.call("umpr_bce_head_bwd", att, K + PAD_ATT, w, res, tg, _to(d_result, dev), gl, B, K, d_att, K + PAD_D, dw, db, ws2, B * 4, st())
    torch.cuda.synchronize()
    r64, l64, _ = HR.bce_forward64(case)
    r32, l32, _ = HR.bce_forward64(case, torch.float32)
    tag = f"{case.tag} {'d_result' if with_d_result else 'd_result=NULL'}"
    rows = _Rows(tag)
    assert not bool(torch.isnan(res).any()) and not bool(torch.isnan(loss).any())
    rows.gate("bce result", res, r64.double(), r32, absolute=True)
    rows.gate("bce loss", loss, l64.reshape(1), l32.reshape(1))
    exact = (r64 == 0) | (r64 == 1)
    assert torch.equal(res.cpu()[exact], r64[exact]), f"{tag}: a saturated row is not exactly 0 or 1"
    assert bool((d_att[:, K:] == SENTINEL).all()), f"{tag}: the padding of d_att was written"
    g64 = HR.bce_backward64(case, r64, case.d_loss, d_result)
    g32 = HR.bce_backward64(case, r32, case.d_loss, d_result, torch.float32)
    for n, got, r, r32_ in zip(HR.BCE_GRADS, (d_att[:, :K], dw, db), g64, g32):
        assert not bool(torch.isnan(got).any()), (tag, n)
        rows.gate("bce " + n, got, r, r32_)
    assert bool((d_att.cpu()[exact][:, :K] == 0).all())
    rows.judge()


# ------------------------------------------------------------------------------------------------------- evaluation accumulator
@pytest.mark.parametrize("n", HR.SQ_ERR_CASES)
def test_sq_err_accumulate(L, dev, n):
    """Two calls in a row onto a pre-loaded accumulator: acc[0] is the preload plus the float64 sum of the float32 elements
    (pred - label)^2 of both batches to 1e-12 relative (only the order of a float64 sum differs), acc[1] is exactly preload + 2 n."""
    case = HR.make_sq_err_case(n)
    acc = torch.tensor(case.preload, dtype=torch.float64, device=dev)
    for p, lab in case.batches:
        L.call("umpr_sq_err_accumulate", p.to(dev), lab.to(dev), n, acc, st())
    torch.cuda.synchronize()
    a0, a1 = HR.sq_err_reference(case)
    got = acc.cpu()
    log(f"sq_err n{n}: acc[0]={float(got[0]):.17g} ref={a0:.17g} rel={abs(float(got[0]) - a0) / a0:.3e} | acc[1]={float(got[1]):g} ref={a1:g}")
    assert abs(float(got[0]) - a0) <= 1e-12 * a0
    assert float(got[1]) == a1
