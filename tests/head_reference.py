"""Float64 references of the stages behind the text and visual paths (test helper, not a test module; CPU only): the visual head
with linear_fusion and the losses (umpr_head_fwd / _bwd), the review merge (umpr_review_merge_fwd / _bwd), the R-Net pre-training
BCE head (umpr_bce_head_fwd / _bwd) and the evaluation accumulator (umpr_sq_err_accumulate).

The head takes three kinds of decision: z > 0 (the ReLU on the prediction) and the signs of pos_emb - img_emb and neg_emb - img_emb
under the abs.  With the decisions given, every output is a smooth function of the inputs.  The functions here
  * build the seeded inputs of the GPU tests in the layout of the C ABI (make_head_case, make_merge_case, make_bce_case),
  * evaluate forward and backward by hand - no autograd: a second statement of the formulas next to oracle/umpr_ref.py - with the
    decisions as inputs, in float64 (the reference) or in float32 on the CPU (the yardstick), and
  * reuse the gate of tests/coattn_decisions.py and tests/gru_reference.py: a HIP tensor may be K x as far from float64 as the
    float32 CPU evaluation of the same formula with the same decisions is.
The review merge takes no decision.  The BCE head rounds p = sigmoid(z) to float32 in both precisions, as the kernel and torch do,
and applies the -100 clamp of the logarithms and the 1e-12 denominator to that rounded p: a saturated row (p == 1.0f or p == 0.0f)
then means the same thing in float64 and in float32.
tests/test_head_reference.py checks all of it against autograd on the CPU; tests/test_gpu_head.py uses it on the GPU.
"""
from types import SimpleNamespace

import torch

from coattn_decisions import FLOOR, K_MAX, K_START, distances, gate   # noqa: F401  (shared, not copied)
from gru_reference import gate_abs                                     # noqa: F401  (shared, not copied)

D = 128                     # width of the review representation: fus_w = [128 + 2V]
F = 1000                    # VGG16 feature width, fixed by the ABI
MD, MK = 128, 256           # review merge: out [B][128] = tanh(ru [B][256] Wu^T + ri Wi^T)
RATE = 0.1                  # loss_v_rate of the cases
MARGIN = 1e-4               # no float64 z, pos_emb - img_emb or neg_emb - img_emb of a case is this close to zero
LDS_LIMIT = 60000           # umpr_head_bwd: (B + 3 B V + 2 V) * 4 bytes of LDS must not exceed this

# The factor the GPU tests use, per tensor.  Worst measured ratio of a HIP distance to the floored float32 CPU distance: see
# profiles/r04_h_head_gates.txt - 2.95 (the scalar d_fus_b at (64, 4, 2) with d_loss = 0: 25 d_pred values of size 1 cancel to 7.7e-3,
# and the float32 CPU sum is itself 1e-5 off), 2.26 (d_neg_v at B = 1153: one serial float32 sum over 1153 rows), below 2 on everything
# else: every ratio is below 4, so K stays at its starting value for every tensor.  K_OF would hold the tensors whose factor had to
# leave it, each with its reason; it is empty.
K = K_START
K_OF = {}


def k_of(name):
    """the gate factor of one tensor: K unless K_OF raises it (never above K_MAX)"""
    k = K_OF.get(name, K)
    assert k <= K_MAX, (name, k)
    return k


def head_lds_bytes(B, V):
    """the dynamic LDS of head_bwd_kernel as the ABI's argument check states it: dz[B], dimg / ddp / ddn [B][V], dpos / dneg [V]"""
    return (B + 3 * B * V + 2 * V) * 4


def largest_b(V):
    """the largest B umpr_head_bwd accepts at V views, from head_lds_bytes"""
    B = (LDS_LIMIT // 4 - 2 * V) // (1 + 3 * V)
    assert head_lds_bytes(B, V) <= LDS_LIMIT < head_lds_bytes(B + 1, V)
    return B


# (B, V, P): the smallest at which each mechanism can fail - one row and three idle waves; UMPR-R (V = 0) off the 4-wave stride
# and on a second trip of the 256 strides; ndot = 2V + BV = 3 (a partial head_emb workgroup); P = 1, 2, 3 with ndot off and on
# the multiple of 4; the workload's batch and one row beyond it; B V and B beyond one 256-thread trip; V V = 289 > 256 in the loss
# loop; a second trip of the lane loop over V; the largest B the LDS bound accepts at V = 4
HEAD_CASES = ((1, 0, 0), (33, 0, 0), (257, 0, 0), (1, 1, 1), (3, 4, 2), (4, 1, 3), (5, 3, 1), (64, 4, 2), (65, 1, 1), (257, 2, 1),
              (3, 17, 1), (2, 65, 1), (largest_b(4), 4, 1))
MERGE_CASES = (1, 3, 4, 5, 31, 32, 33, 128, 129, 256, 257)
BCE_CASES = ((1, 1), (3, 63), (4, 64), (5, 65), (37, 256), (257, 256))
SQ_ERR_CASES = (1, 255, 256, 257, 1000)
HEAD_OUT = ("pred", "loss", "z", "img_emb", "pos_match", "neg_match", "posneg_emb")
HEAD_GRADS = ("d_rr", "d_cu", "d_ci", "d_pp", "d_pn", "d_vgg", "d_pos_v", "d_neg_v", "d_lin_w", "d_lin_b", "d_fus_w", "d_fus_b")
HEAD_GRADS_V0 = ("d_rr", "d_fus_w", "d_fus_b")          # all that V = 0 has
WRONG_HEAD_FWD = ("mean_p_minus_1",)
WRONG_HEAD_BWD = ("dfw_one_row_short",)

# seed = 1000003 B + 1009 V + P + HEAD_SEED_SHIFT.get(case, 0).  The shifts are the smallest for which the float64 reference keeps
# MARGIN (about one seed in two does at B = 1153: 9224 differences of spread 0.9), z has both signs from B = 3 on (z > 0 at
# B = 1, where a masked row would leave nothing to compare), and 30% to 55% of the rows have z < 0 from B = 33 on.
# tests/test_head_reference.py asserts all three for every case.
HEAD_SEED_SHIFT = {(3, 4, 2): 1, (5, 3, 1): 1, (3, 17, 1): 1, (largest_b(4), 4, 1): 2}


# ------------------------------------------------------------------------------------------------------- head
def make_head_case(B, V, P, seed=None):
    """Seeded float32 inputs in the layout of the C ABI.  rr [B][128] = randn and fus_w[:128] = randn / sqrt(128): z has a
    spread of about 1 around fus_b = 0.15, so that roughly 44% of the rows have z < 0; fus_w[128:] = 0.3 randn; labels in 1..5;
    c_u, c_i, prefer_pos, prefer_neg uniform in [0, 1); vgg [B V P][1000], pos_v, neg_v [V][1000] = randn; lin_w = 0.02 randn
    (the embeddings' differences have a spread of about 0.9: tanh is neither linear nor saturated), lin_b = 0.1;
    d_pred = randn with rows 1, 4, 7, ... zero; d_loss = 0.7."""
    shift = HEAD_SEED_SHIFT.get((B, V, P), 0)
    g = torch.Generator().manual_seed(1000003 * B + 1009 * V + P + shift if seed is None else seed)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    c = SimpleNamespace(B=B, V=V, P=P, rate=RATE, tag=f"B{B} V{V} P{P}")
    c.rr = rn(B, D)
    c.fus_w = torch.cat([rn(D) / D ** 0.5, 0.3 * rn(2 * V)])
    c.fus_b = torch.tensor([0.15])
    c.labels = torch.randint(1, 6, (B,), generator=g).float()
    c.d_pred = rn(B)
    c.d_pred[1::3] = 0
    c.d_loss = 0.7
    if V:
        c.c_u, c.c_i, c.pp, c.pn = (torch.rand(B, V, generator=g) for _ in range(4))
        c.vgg = rn(B * V * P, F)
        c.pos_v, c.neg_v = rn(V, F), rn(V, F)
        c.lin_w, c.lin_b = 0.02 * rn(F), torch.tensor([0.1])
    else:
        c.c_u = c.c_i = c.pp = c.pn = c.vgg = c.pos_v = c.neg_v = c.lin_w = c.lin_b = None
    return c


def head_decisions(z, posneg_emb=None, img_emb=None):
    """the decisions read off a forward's z [B], posneg_emb [2][V] and img_emb [B][V] (any dtype; a float32 subtraction keeps the
    sign of the exact difference): zpos [B] bool, sgp / sgn [B][V] in {-1, 0, +1} as float64 (None at V = 0)"""
    d = SimpleNamespace(zpos=z.detach().cpu() > 0, sgp=None, sgn=None)
    if posneg_emb is not None:
        pe, ie = posneg_emb.detach().cpu(), img_emb.detach().cpu()
        d.sgp, d.sgn = torch.sign(pe[0] - ie).double(), torch.sign(pe[1] - ie).double()
    return d


def head_forward64(case, dtype=torch.float64, decisions=None, wrong=None):
    """Every output of umpr_head_fwd in `dtype`, as a namespace, with the decisions given (None: the evaluation takes its own,
    and returns them as .decisions):
        img[b,v]   = mean_q vgg[b,v,q]                      img_emb[b,v] = img[b,v] . lin_w + lin_b
        pos_emb[v] = pos_v[v] . lin_w + lin_b               posneg_emb = (pos_emb, neg_emb)
        pos_match  = tanh(sgp (pos_emb - img_emb))          neg_match = tanh(sgn (neg_emb - img_emb))          (|x| = sign(x) x)
        feat       = (rr, c_u c_i (1 - pos_match), c_u c_i (1 - neg_match))      z = feat . fus_w + fus_b
        pred       = z where zpos, else 0
        loss_r     = mean (pred - labels)^2                 loss_v = mean over V x V of prefer_pos^T pos_match + prefer_neg^T neg_match
        loss       = (loss_r + rate loss_v, loss_r, loss_v)
    V = 0 has rr, z, pred and loss_r alone (loss_v = 0; the four visual tensors are None).  `wrong` names one of WRONG_HEAD_FWD."""
    assert wrong is None or wrong in WRONG_HEAD_FWD, wrong
    B, V, P = case.B, case.V, case.P
    t = lambda x: x.to(dtype)                              # noqa: E731
    o = SimpleNamespace(img_emb=None, pos_match=None, neg_match=None, posneg_emb=None, img=None)
    rr, fw, fb, labels = t(case.rr), t(case.fus_w), t(case.fus_b), t(case.labels)
    z = rr @ fw[:D] + fb
    own = None
    if V:
        lw, lb = t(case.lin_w), t(case.lin_b)
        div = P - 1 if wrong == "mean_p_minus_1" else P     # WRONG on purpose: the mean over the photos divides by P - 1
        o.img = t(case.vgg).view(B, V, P, F).sum(2) / div
        o.img_emb = o.img @ lw + lb
        o.posneg_emb = torch.stack([t(case.pos_v) @ lw + lb, t(case.neg_v) @ lw + lb])
        dp, dn = o.posneg_emb[0] - o.img_emb, o.posneg_emb[1] - o.img_emb
        own = (torch.sign(dp).double(), torch.sign(dn).double())
        sgp, sgn = own if decisions is None else (decisions.sgp, decisions.sgn)
        o.pos_match, o.neg_match = torch.tanh(t(sgp) * dp), torch.tanh(t(sgn) * dn)
        cc = t(case.c_u) * t(case.c_i)
        z = z + (cc * (1 - o.pos_match)) @ fw[D:D + V] + (cc * (1 - o.neg_match)) @ fw[D + V:]
    o.z = z
    zpos = (z > 0) if decisions is None else decisions.zpos
    o.pred = torch.where(zpos, z, torch.zeros_like(z))
    loss_r = ((o.pred - labels) ** 2).mean()
    loss_v = torch.zeros((), dtype=dtype)
    if V:
        loss_v = (t(case.pp).t() @ o.pos_match + t(case.pn).t() @ o.neg_match).mean()
    o.loss = torch.stack([loss_r + case.rate * loss_v, loss_r, loss_v])
    o.decisions = SimpleNamespace(zpos=z > 0, sgp=own and own[0], sgn=own and own[1]) if decisions is None else decisions
    return o


def head_backward64(case, decisions, d_loss, d_pred=None, dtype=torch.float64, fwd=None, wrong=None):
    """The twelve gradients of umpr_head_bwd in the ABI's order (a dict; at V = 0 only d_rr, d_fus_w, d_fus_b), by hand, in
    `dtype`, of d_loss * loss[0] + sum(d_pred * pred) with the decisions given.  `fwd` is the forward the saved tensors are taken
    from (default: head_forward64 in `dtype` with the same decisions).
        g      = d_loss 2 (pred - labels) / B + d_pred       dz = g where zpos, else 0
        d_fus_w = dz^T feat       d_fus_b = sum dz           d_rr = dz (x) fus_w[:128]
        sv     = d_loss rate / V^2                           dfp = dz (x) fus_w[128:128+V]       dfn = dz (x) fus_w[128+V:]
        d_cu   = (dfp (1 - pm) + dfn (1 - nm)) c_i           d_ci likewise with c_u
        d_pp[b,v] = sv sum_q pm[b,q]                         d_pn[b,v] = sv sum_q nm[b,q]
        dpm    = -dfp c_u c_i + sv sum_q pp[b,q]             ddp = dpm (1 - pm^2) sgp            (dnm, ddn likewise)
        dimg   = -(ddp + ddn)      dpos[v] = sum_b ddp       dneg[v] = sum_b ddn
        d_vgg[b,v,q] = dimg[b,v] lin_w / P                   d_pos_v = dpos (x) lin_w            d_neg_v = dneg (x) lin_w
        d_lin_w = dimg^T img + dpos^T pos_v + dneg^T neg_v   d_lin_b = sum dimg + sum dpos + sum dneg   (exactly 0: lin_b cancels)
    The key "_parts" of the result holds a namespace with dz, dimg, dpos, dneg.  `wrong` names one of WRONG_HEAD_BWD."""
    assert wrong is None or wrong in WRONG_HEAD_BWD, wrong
    B, V, P = case.B, case.V, case.P
    t = lambda x: x.to(dtype)                              # noqa: E731
    f = head_forward64(case, dtype, decisions) if fwd is None else fwd
    assert f.z.dtype == dtype, (f.z.dtype, dtype)
    fw, labels = t(case.fus_w), t(case.labels)
    g = d_loss * 2 * (f.pred - labels) / B
    if d_pred is not None:
        g = g + t(d_pred)
    dz = torch.where(decisions.zpos, g, torch.zeros_like(g))
    feat = t(case.rr)
    if V:
        cu, ci, pm, nm = t(case.c_u), t(case.c_i), f.pos_match, f.neg_match
        feat = torch.cat([feat, cu * ci * (1 - pm), cu * ci * (1 - nm)], 1)
    if wrong == "dfw_one_row_short":                        # WRONG on purpose: the last row with dz != 0 is left out of d_fus_w
        keep = torch.ones(B, dtype=torch.bool)
        keep[int(torch.nonzero(dz)[-1])] = False
        d_fw = dz[keep] @ feat[keep]
    else:
        d_fw = dz @ feat
    out = {"d_rr": dz.unsqueeze(1) * fw[:D].unsqueeze(0), "d_fus_w": d_fw, "d_fus_b": dz.sum().reshape(1),
           "_parts": SimpleNamespace(dz=dz, dimg=None, dpos=None, dneg=None)}
    if V == 0:
        return out
    sv = d_loss * case.rate / (V * V)
    pp, pn, lw = t(case.pp), t(case.pn), t(case.lin_w)
    dfp, dfn = dz.unsqueeze(1) * fw[D:D + V], dz.unsqueeze(1) * fw[D + V:]
    out["d_cu"] = (dfp * (1 - pm) + dfn * (1 - nm)) * ci
    out["d_ci"] = (dfp * (1 - pm) + dfn * (1 - nm)) * cu
    out["d_pp"] = (sv * pm.sum(1, keepdim=True)).expand(B, V).clone()
    out["d_pn"] = (sv * nm.sum(1, keepdim=True)).expand(B, V).clone()
    dpm = -dfp * cu * ci + sv * pp.sum(1, keepdim=True)
    dnm = -dfn * cu * ci + sv * pn.sum(1, keepdim=True)
    ddp, ddn = dpm * (1 - pm * pm) * t(decisions.sgp), dnm * (1 - nm * nm) * t(decisions.sgn)
    dimg, dpos, dneg = -(ddp + ddn), ddp.sum(0), ddn.sum(0)
    out["d_vgg"] = (dimg.reshape(B * V, 1, 1) * lw / P).expand(B * V, P, F).reshape(B * V * P, F).clone()
    out["d_pos_v"], out["d_neg_v"] = dpos.unsqueeze(1) * lw, dneg.unsqueeze(1) * lw
    out["d_lin_w"] = dimg.reshape(-1) @ f.img.reshape(B * V, F) + dpos @ t(case.pos_v) + dneg @ t(case.neg_v)
    out["d_lin_b"] = (dimg.sum() + dpos.sum() + dneg.sum()).reshape(1)
    out["_parts"] = SimpleNamespace(dz=dz, dimg=dimg, dpos=dpos, dneg=dneg)
    return {k: out[k] for k in HEAD_GRADS + ("_parts",)}


def head_grad_names(case):
    return HEAD_GRADS if case.V else HEAD_GRADS_V0


def head_margins(case, fwd):
    """(smallest |z|, smallest |pos_emb - img_emb| or |neg_emb - img_emb| - inf at V = 0) of a float64 forward"""
    mz = float(fwd.z.abs().min())
    if not case.V:
        return mz, float("inf")
    return mz, float(torch.minimum((fwd.posneg_emb[0] - fwd.img_emb).abs().min(), (fwd.posneg_emb[1] - fwd.img_emb).abs().min()))


def lin_b_floor(parts):
    """FLOOR x (sum |dimg| + sum |dpos| + sum |dneg|) of a float64 backward: the least residue the float32 yardstick of
    d_lin_b - a sum whose exact value is zero - is credited with"""
    return FLOOR * float(parts.dimg.abs().sum() + parts.dpos.abs().sum() + parts.dneg.abs().sum())


def gate_lin_b(got, ref32, parts64, K=K, log=None, tag=""):
    """|d_lin_b| of `got` within K x max(|d_lin_b| of the float32 CPU evaluation, lin_b_floor).  Logged before it is judged."""
    assert K <= K_MAX, K
    d, r, fl = abs(float(got)), abs(float(ref32)), lin_b_floor(parts64)
    finite = d == d and d != float("inf")
    if not finite:
        ratio = float("inf")
    elif d == 0:                                            # e.g. every live row masked by the ReLU: all three are exactly 0
        ratio = 0.0
    else:
        ratio = d / max(r, fl) if max(r, fl) > 0 else float("inf")
    row = {"name": "d_lin_b", "d_max": d, "r_max": r, "floor": fl, "ratio": ratio, "over": ratio / K, "ok": finite and ratio <= K}
    if log is not None:
        log(f"{tag} d_lin_b: abs={d:.3e} | ref32 abs={r:.3e} floor={fl:.3e} | ratio={ratio:.2f} K={K:g}{'' if row['ok'] else '  OUTSIDE'}")
    return row


# ------------------------------------------------------------------------------------------------------- review merge
MERGE_GRADS = ("d_repr_u", "d_repr_i", "dW_u", "dW_i")


def make_merge_case(B, seed=None):
    """ru, ri [B][256] = randn, Wu, Wi [128][256] = randn / 16 (the inputs of test_review_merge), d_out [B][128] = randn"""
    g = torch.Generator().manual_seed(7000 + B if seed is None else seed)
    rn = lambda *s: torch.randn(*s, generator=g)          # noqa: E731
    return SimpleNamespace(B=B, ru=rn(B, MK), ri=rn(B, MK), Wu=rn(MD, MK) / 16, Wi=rn(MD, MK) / 16, d_out=rn(B, MD), tag=f"merge B{B}")


def merge_forward64(case, dtype=torch.float64):
    """out [B][128] = tanh(ru Wu^T + ri Wi^T) in `dtype`"""
    t = lambda x: x.to(dtype)                              # noqa: E731
    return torch.tanh(t(case.ru) @ t(case.Wu).t() + t(case.ri) @ t(case.Wi).t())


def merge_backward64(case, d_out, dtype=torch.float64, out=None):
    """(d_repr_u, d_repr_i, dW_u, dW_i) by hand in `dtype`: dpre = d_out (1 - out^2), d_repr_s = dpre W_s, dW_s = dpre^T repr_s"""
    t = lambda x: x.to(dtype)                              # noqa: E731
    out = merge_forward64(case, dtype) if out is None else out
    dpre = t(d_out) * (1 - out * out)
    return dpre @ t(case.Wu), dpre @ t(case.Wi), dpre.t() @ t(case.ru), dpre.t() @ t(case.ri)


# ------------------------------------------------------------------------------------------------------- BCE head
BCE_GRADS = ("d_att", "dw", "db")
BCE_EPS = float(torch.tensor(1e-12, dtype=torch.float32))   # the denominator's floor is the FLOAT 1e-12f in ATen (in double too) and in the kernel


def make_bce_case(B, K_, seed=None):
    """att [B][K] = randn, w [K] = 2 randn / sqrt(K), b = 0.3.  Every row is then rescaled so that |att . w| <= 8 (|z| < 10);
    from B = 3 on, row 0 is rescaled to att . w = +40 (p == 1.0f) and row 1 to -40 (p = 4e-18, p (1 - p) under the 1e-12
    denominator); from B = 5 on, row 2 to -110 (p == 0.0f: the -100 clamp of log p).  B = 1 keeps its only row unsaturated.
    Targets: binary where the case's index in BCE_CASES is even (other shapes: where B is odd), uniform in [0, 1] otherwise.
    d_result [B] = randn, d_loss = 0.7."""
    g = torch.Generator().manual_seed(9000 + 1000 * B + K_ if seed is None else seed)
    att = torch.randn(B, K_, generator=g)
    w = 2 * torch.randn(K_, generator=g) / K_ ** 0.5
    w[w.abs() < 1e-2] = 0.05                                # K = 1: a weight that cannot be rescaled away
    b = torch.tensor([0.3])
    zc = att.double() @ w.double()
    scale = torch.clamp(8 / zc.abs(), max=1.0)
    if B >= 3:
        scale[0], scale[1] = 40 / zc[0], -40 / zc[1]
    if B >= 5:
        scale[2] = -110 / zc[2]
    att = (att.double() * scale.unsqueeze(1)).float()
    binary = (BCE_CASES.index((B, K_)) % 2 == 0) if (B, K_) in BCE_CASES else bool(B % 2)
    target = torch.randint(0, 2, (B,), generator=g).float() if binary else torch.rand(B, generator=g)
    c = SimpleNamespace(B=B, K=K_, att=att, w=w, b=b, target=target, binary=binary, d_result=torch.randn(B, generator=g), d_loss=0.7,
                        tag=f"bce B{B} K{K_} {'binary' if binary else 'soft'}")
    c.n_sat = 0 if B < 3 else (2 if B < 5 else 3)
    return c


def bce_forward64(case, dtype=torch.float64):
    """(result [B] float32, loss scalar in `dtype`, z [B] in `dtype`): z = att . w + b in `dtype`, p = sigmoid(z) ROUNDED TO
    FLOAT32 (what the kernel stores and what the backward reads), term = -(t max(log p, -100) + (1 - t) max(log(1 - p), -100))
    evaluated in `dtype` on that rounded p, loss = mean term"""
    t = lambda x: x.to(dtype)                              # noqa: E731
    z = t(case.att) @ t(case.w) + t(case.b)
    p32 = torch.sigmoid(z).float()
    p, tg = t(p32), t(case.target)
    terms = -(tg * torch.log(p).clamp_min(-100) + (1 - tg) * torch.log1p(-p).clamp_min(-100))
    return p32, terms.mean(), z


def bce_backward64(case, result, d_loss, d_result=None, dtype=torch.float64):
    """(d_att [B][K], dw [K], db [1]) by hand in `dtype` from the rounded `result` (ATen's binary_cross_entropy_backward and
    sigmoid_backward): g = d_loss / B (p - t) / max(p (1 - p), 1e-12f) + d_result, dz = g p (1 - p), d_att = dz (x) w,
    dw = dz^T att, db = sum dz"""
    t = lambda x: x.to(dtype)                              # noqa: E731
    p, tg = t(result), t(case.target)
    pq = p * (1 - p)
    g = d_loss / case.B * (p - tg) / pq.clamp_min(BCE_EPS)
    if d_result is not None:
        g = g + t(d_result)
    dz = g * pq
    return dz.unsqueeze(1) * t(case.w), dz @ t(case.att), dz.sum().reshape(1)


# ------------------------------------------------------------------------------------------------------- evaluation accumulator
def make_sq_err_case(n, seed=None):
    """two batches of (pred, label) [n]: pred = 3 + randn, labels in 1..5; acc preloaded with (3.25, 7)"""
    g = torch.Generator().manual_seed(500 + n if seed is None else seed)
    batches = [(3 + torch.randn(n, generator=g), torch.randint(1, 6, (n,), generator=g).float()) for _ in range(2)]
    return SimpleNamespace(n=n, batches=batches, preload=(3.25, 7.0))


def sq_err_reference(case):
    """(acc[0], acc[1]) after both batches: the preload plus the float64 sum of the FLOAT32 elements (pred - label)^2, and 2 n"""
    s = sum(float(((p - l) * (p - l)).double().sum()) for p, l in case.batches)
    return case.preload[0] + s, case.preload[1] + 2 * case.n
