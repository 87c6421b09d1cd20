"""Decision-conditioned reference of the control network (test helper, not a test module; CPU only).

The control network (umpr_amd/csrc/text_ops.hip: cnet_head_fwd_kernel / cnet_head_bwd_kernel, gate_fwd_kernel /
gate_bwd_kernel) takes four kinds of decision per step: the first argmax over the conv positions of every (sentence, filter),
ReLU's `cmax > 0`, the 0.35 threshold on the sigmoid, and the side of 0.5 that view_score falls on.  Once they are fixed the
head, the gate and the S-Net are smooth functions of every value.  The functions here
  * build the seeded inputs of the GPU tests (make_inputs: zero tails past each sentence's length, as the GRU leaves them, so
    that exact ties, dead filters and argmaxes at padded positions are in every case),
  * compute the pre-activation in float64 (conv64) and check every saved tensor and decision of the HIP forward against it
    within the a-priori rounding of a float32 evaluation (rounding_delta, check_decisions),
  * run the head, the gate and the S-Net forward and backward in float64 - or, for the yardstick, in float32 - with the
    decisions given (forward64 / backward64, gate_forward64 / gate_backward64, snet64), and
  * reuse the gate of tests/coattn_decisions.py: a HIP tensor may be K x as far from float64 as the float32 CPU evaluation of
    the same formula with the same decisions is.
tests/test_control_decisions.py checks them against autograd on the CPU; tests/test_gpu_control.py uses them on the GPU.
Layout: X [N = B*S][L][128], Y / pre-activations [N][positions][KC], cmax / argl [N][KC], sp / view_p [N][V], final [B][V].
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from coattn_decisions import FLOOR, K_MAX, K_START, bf16_round, distances, gate   # noqa: F401  (shared, not copied)

D = 128                     # 2 * gru_size, the only width the kernels are built for
AT = 64                     # self_atte_size of the S-Net kernels
EPS32 = 2.0 ** -24          # unit roundoff of float32
THR = 0.35                  # config.threshold
THR32 = float(torch.tensor(THR, dtype=torch.float32))     # what `sg < thr` compares with
MARGIN = 1e-4               # no reference sp within this of the threshold, no view_score within it of 0.5 (asserted)
# The factor the GPU tests use.  Worst measured ratio of a HIP distance to the floored float32 CPU distance, see
# profiles/r04_e_control_gates.txt: 7.75 (db of the gate backward at (2, 3, 9, 3, 4, 132), ONE number whose view_score lies 6e-3
# from 0.5, so that the rounding of view_score reaches vs - 0.5 amplified 80-fold, in the HIP and in the float32 CPU value
# alike, and the ratio compares two single draws); every other tensor is at 2.02 or below.  Twice the worst, rounded up, is 16:
# K takes the value it may never exceed.
K = K_MAX
# (B, S, L, V, KS, KC) of the GPU tests: the smallest case; even KS (the window GEMM also writes position L - 1, which must not
# win); KC = 132 needs a third lane trip; L = 65 is just above one wave; KS = L = 8; KC = 512 is the limit.  Sentence counts 1,
# 6, 9, 10, 14, 15 and S = 1, 2, 3, 5, 7, 9 reach the forward's wave tail and the backward's `on` tail; B*S*L runs from 1 to
# 1170, both sides of the GEMM's 64 and 128 row tiles.
SHAPES = ((1, 1, 1, 1, 1, 4), (3, 5, 20, 1, 3, 120), (2, 3, 11, 4, 2, 120), (2, 3, 9, 3, 4, 132), (2, 7, 65, 4, 3, 120),
          (5, 2, 8, 4, 8, 64), (1, 9, 130, 2, 5, 512), (2, 2, 70, 2, 3, 120))
# seeds at which every condition of tests/test_control_decisions.py::test_conditions holds; chosen on the CPU from the
# reference alone (float64), never from what a kernel returns
SEEDS = {(1, 9, 130, 2, 5, 512): 108, (2, 2, 70, 2, 3, 120): 1}     # every other shape: 0
SNET_SHAPES = ((2, 3, 1), (3, 5, 20), (1, 4, 64), (2, 3, 65), (2, 2, 130), (1, 3, 200))      # (B, S, L) of test_snet_stage


def lout(L, KS):
    """valid conv positions of nn.Conv1d(padding=(KS-1)//2): L for an odd KS, L - 1 for an even one"""
    return L + 2 * ((KS - 1) // 2) - KS + 1


def make_inputs(B, S, L, V, KS, KC, seed=None):
    """The seeded inputs of one shape: X = 0.7 randn with the rows at and past a per-sentence length zeroed (lengths uniform in
    1..L, sentence 0 full, sentence 1 of length 1); the C-Net / S-Net / SS-Net parameters of umpr_amd.synthetic with every
    eighth conv bias lowered by 1.5 (dead filters) and the next raised by 0.5 (filters whose maximum is the bias itself, at a
    padded position) and Wl doubled (sigmoids on both sides of the threshold); randn upstream gradients."""
    from umpr_amd.synthetic import make_param_state
    shape = (B, S, L, V, KS, KC)
    if seed is None:
        seed = SEEDS.get(shape, 0)
    g = torch.Generator().manual_seed(100003 * seed + 7919 * B + 1009 * S + 101 * L + 13 * V + 3 * KS + KC)
    rn = lambda *s: torch.randn(*s, generator=g)
    N = B * S
    X = 0.7 * rn(N, L, D)
    lengths = torch.randint(1, L + 1, (N,), generator=g)
    lengths[0] = L
    if N > 1:
        lengths[1] = 1
    X = X * (torch.arange(L).view(1, L, 1) < lengths.view(N, 1, 1))
    P = make_param_state(13, 50, 500, V, False, with_vgg=False, m_scale=0.3, kernel_size=KS, kernel_count=KC)
    pre = "control_net."
    bc = P[pre + "c_net.cnn.0.bias"].clone()
    bc[0::8] -= 1.5
    bc[1::8] += 0.5
    return {"dims": shape, "lengths": lengths, "X": X.contiguous(), "Wc": P[pre + "c_net.cnn.0.weight"].contiguous(), "bc": bc,
            "Wl": (2 * P[pre + "c_net.linear.0.weight"]).contiguous(), "bl": P[pre + "c_net.linear.0.bias"].clone(),
            "Ms": P[pre + "s_net.Ms"].contiguous(), "Ws": P[pre + "s_net.Ws"].reshape(-1).contiguous(),
            "ssW": P[pre + "ss_net.linear.0.weight"].reshape(-1).contiguous(), "ssb": P[pre + "ss_net.linear.0.bias"].clone(),
            "d_final": rn(B, V), "d_view_p": rn(B, S, V), "d_prefer_pos": rn(B, V), "d_prefer_neg": rn(B, V)}


def bf16_operands(x):
    """x with X and Wc rounded to bf16: what the window GEMM multiplies under umpr_set_gemm_bf16(1).  Products of two bf16
    values are exact in float32, so only the accumulation rounds and rounding_delta applies unchanged."""
    y = dict(x)
    y["X"], y["Wc"] = bf16_round(x["X"]), bf16_round(x["Wc"])
    y["X_snet"] = x["X"]           # the S-Net behind the gate still reads the unrounded X
    return y


def _conv(X, Wc, bc, KS, full=False):
    """[N][Lout][KC] in the operands' dtype (full: all L positions of the window GEMM - for an even KS the last one reads one
    zero past the sentence and is no output of nn.Conv1d)"""
    L, pad = X.shape[1], (KS - 1) // 2
    y = F.conv1d(F.pad(X.transpose(1, 2), (pad, KS - 1 - pad)), Wc, bc).transpose(1, 2)
    return y if full else y[:, :lout(L, KS)]


def conv64(X, Wc, bc, KS, full=False):
    """the pre-activation in float64"""
    return _conv(X.double(), Wc.double(), bc.double(), KS, full)


def rounding_delta(X, Wc, bc, KS, full=False):
    """delta[n][l][k] = (128 KS + 2) 2^-24 (sum |x| |w| + |bc|): the a-priori bound of a (128 KS)-term float32 dot product in
    any order, the bias add and ReLU (1-Lipschitz).  Derived, not measured."""
    return (D * KS + 2) * EPS32 * _conv(X.double().abs(), Wc.double().abs(), bc.double().abs(), KS, full)


def first_argmax(Y):
    """(values, first index) of the maximum over dim 1 of Y [N][positions][KC], by exact comparison"""
    m = Y.max(1).values
    pos = torch.arange(Y.shape[1]).view(1, -1, 1).expand_as(Y)
    first = torch.where(Y == m.unsqueeze(1), pos, torch.full_like(pos, Y.shape[1])).min(1).values
    return m, first


def self_atte(X, Ms, Ws):
    """S-Net pooling (src/model.py:71-78) of X [N][L][128] in the operands' dtype: (U [N][L][64], P [N][L], self_atte [N][128])"""
    U = torch.tanh(X @ Ms.t())
    Pr = torch.softmax(U @ Ws, -1)
    return U, Pr, (Pr.unsqueeze(-1) * X).sum(1)


def forward64(x, argl, kept=None, dtype=torch.float64, thr=THR32):
    """The head (src/model.py:118-125) with the maximum read at the given positions argl [N][KC] and - when given - the
    threshold decisions kept [N][V] (otherwise its own `sp >= thr`).  Returns pre, Y [N][Lout][KC], cmax, sp, view_p, final."""
    B, S, L, V, KS, KC = x["dims"]
    t = lambda k: x[k].to(dtype)
    pre = _conv(t("X"), t("Wc"), t("bc"), KS)
    Y = torch.relu(pre)
    cmax = Y.gather(1, argl.cpu().long().unsqueeze(1)).squeeze(1)
    sp = torch.sigmoid(cmax @ t("Wl").t() + t("bl"))
    kept = (sp >= thr) if kept is None else kept.cpu().bool()
    vp = torch.where(kept, sp, torch.zeros_like(sp))
    return SimpleNamespace(pre=pre, Y=Y, cmax=cmax, sp=sp, view_p=vp, final=(vp * vp).view(B, S, V).sum(1), kept=kept)


def decisions64(x, thr=THR32):
    """The reference's own decisions in float64: (argl, alive, kept, side, forward, gate forward)"""
    B, S, L, V, KS, KC = x["dims"]
    _, argl = first_argmax(torch.relu(conv64(x["X"], x["Wc"], x["bc"], KS)))
    f = forward64(x, argl, thr=thr)
    _, _, sa = self_atte(x["X"].double(), x["Ms"].double(), x["Ws"].double())
    gf = gate_forward64(sa.view(B, S, D), x["ssW"], x["ssb"], f.view_p.view(B, S, V), f.final)
    return SimpleNamespace(argl=argl, alive=f.cmax > 0, kept=f.kept, side=gf.side, f=f, gate=gf)


def backward64(x, argl, alive, kept, d_final=None, d_view_p=None, dtype=torch.float64, parts=None, route=None):
    """(dX, dWc, dbc, dWl, dbl) of the head with the decisions given, in `dtype` (float64: the reference; float32: the yardstick
    `ref32` of gate).
        g    = d_view_p + 2 view_p d_final            dsig = kept ? g sp (1 - sp) : 0
        dbl  = sum dsig        dWl = dsig^T cmax      dc = dsig Wl
        dY[argl] = alive ? dc : 0                     dbc, dWc, dX: the convolution's adjoints (autograd with dY held fixed)
    A dict passed as `parts` receives dsig, dc and dY.  `route` [N][KC] sends dc to OTHER positions than the ones cmax is read
    at: a backward that misroutes while the forward's saved cmax / sp / view_p are right - what umpr_cnet_head_bwd does when
    handed one altered index."""
    B, S, L, V, KS, KC = x["dims"]
    N, Lo = B * S, lout(L, KS)
    f = forward64(x, argl, kept, dtype)
    g = torch.zeros(N, V, dtype=dtype)
    if d_view_p is not None:
        g = g + d_view_p.to(dtype).reshape(N, V)
    if d_final is not None:
        g = g + 2 * f.view_p * d_final.to(dtype).repeat_interleave(S, 0)
    dsig = torch.where(f.kept, g * f.sp * (1 - f.sp), torch.zeros_like(g))
    dbl = dsig.sum(0)
    dWl = dsig.t() @ f.cmax
    dc = dsig @ x["Wl"].to(dtype)
    dcr = torch.where(alive.cpu().bool(), dc, torch.zeros_like(dc))
    dY = torch.zeros(N, Lo, KC, dtype=dtype)
    dY.scatter_(1, (argl if route is None else route).cpu().long().unsqueeze(1), dcr.unsqueeze(1))
    X = x["X"].detach().to(dtype).clone().requires_grad_(True)
    Wc = x["Wc"].detach().to(dtype).clone().requires_grad_(True)
    (_conv(X, Wc, None, KS) * dY).sum().backward()
    if parts is not None:
        parts.update(dsig=dsig, dc=dc, dY=dY)
    return X.grad, Wc.grad, dY.sum((0, 1)), dWl, dbl


HEAD_GRADS = ("dX", "dWc", "dbc", "dWl", "dbl")


def gate_forward64(sa, w, bias, view_p, c_out, side=None, dtype=torch.float64):
    """SS-Net and the preference gate (src/model.py:142-143, 186-197) on sa [B][S][128], view_p [B][S][V], c_out [B][V], with
    the side of 0.5 given as `side` [B][V] (True: view_score > 0.5; otherwise its own).  Returns senti [B][S], vs, prefer_pos,
    prefer_neg, side, num, den."""
    sa, w, bias, vp, co = (t.to(dtype) for t in (sa, w, bias, view_p, c_out))
    senti = torch.sigmoid(sa @ w + bias)
    num = (senti.unsqueeze(-1) * vp * vp).sum(1)
    den = (vp * vp).sum(1) + 1e-4
    vs = num / den
    side = (vs > 0.5) if side is None else side.cpu().bool()
    zero = torch.zeros_like(vs)
    pp = torch.where(side, co * 4 * (vs - 0.5) ** 2, zero)
    pn = torch.where(side, zero, co * 4 * (0.5 - vs) ** 2)
    return SimpleNamespace(senti=senti, vs=vs, prefer_pos=pp, prefer_neg=pn, side=side, num=num, den=den)


GATE_GRADS = ("d_self_atte", "d_view_p", "d_c_out", "dw", "db")


def gate_backward64(sa, w, bias, view_p, c_out, side, d_pp, d_pn, dtype=torch.float64):
    """(d_self_atte, d_view_p, d_c_out, dw, db) of the gate with the side given (view_p and c_out are independent inputs here,
    as they are for umpr_control_gate_bwd)."""
    f = gate_forward64(sa, w, bias, view_p, c_out, side, dtype)
    sa, w, vp, co, gpp, gpn = (t.to(dtype) for t in (sa, w, view_p, c_out, d_pp, d_pn))
    d_co =torch.where(f.side, gpp * 4 * (f.vs - 0.5) ** 2, gpn * 4 * (0.5 - f.vs) ** 2)
    dvs = torch.where(f.side, gpp * co * 8 * (f.vs - 0.5), gpn * co * -8 * (0.5 - f.vs))
    dnum = dvs / f.den
    dden = -dvs * f.num / (f.den * f.den)
    d_vp = 2 * vp * (f.senti.unsqueeze(-1) * dnum.unsqueeze(1) + dden.unsqueeze(1))
    dse = (dnum.unsqueeze(1) * vp * vp).sum(-1)
    dpre = dse * f.senti * (1 - f.senti)
    return dpre.unsqueeze(-1) * w, d_vp, d_co, (dpre.unsqueeze(-1) * sa).sum((0, 1)), dpre.sum().reshape(1)


def make_snet_inputs(B, S, L, wl, seed=0):
    """X as make_inputs builds it; Ms, Ws = 0.05 randn (|X Ms^T| stays around 0.4: tanh is not saturated, so the routed factor
    1 - U^2 is alive and carries no cancellation); word_soft uniform in [0, 1); randn upstream gradients."""
    g = torch.Generator().manual_seed(5000 + 97 * seed + 1000 * B + 100 * S + L + 7 * wl)
    rn = lambda *s: torch.randn(*s, generator=g)
    N = B * S
    X = 0.7 * rn(N, L, D)
    lengths = torch.randint(1, L + 1, (N,), generator=g)
    lengths[0] = L
    if N > 1:
        lengths[1] = 1
    X = X * (torch.arange(L).view(1, L, 1) < lengths.view(N, 1, 1))
    return {"dims": (B, S, L, wl), "X": X.contiguous(), "Ms": 0.05 * rn(AT, D), "Ws": 0.05 * rn(AT),
            "word_soft": torch.rand(B, S, wl, generator=g), "d_senti": rn(B, D), "d_self_atte": rn(B, S, D)}


SNET_OUT = ("U", "P", "wsum", "self_atte", "senti")


def snet64(x, d_senti=None, d_self_atte=None, dtype=torch.float64):
    """The S-Net (no decisions) in `dtype`: autograd of oracle.umpr_ref.s_net.  Returns ((U, P, wsum, self_atte [B][S][128],
    senti [B][128]), (dX [N][L][128], dMs, dWs, d_word_soft [B][S][wl])); an upstream gradient left None counts as zero."""
    from oracle import umpr_ref as R
    B, S, L, wl = x["dims"]
    leaf = lambda t: t.detach().to(dtype).clone().requires_grad_(True)
    X = leaf(x["X"])
    P = {"Ms": leaf(x["Ms"]), "Ws": leaf(x["Ws"].view(1, AT))}
    wsoft = leaf(x["word_soft"])
    sa, senti = R.s_net(X.view(B, S * L, D), wsoft.view(B, S * wl), L, P, "")
    outs, ups = [], []
    for o, u in ((senti, d_senti), (sa, d_self_atte)):
        if u is not None:
            outs.append(o)
            ups.append(u.to(dtype).reshape(o.shape))
    torch.autograd.backward(outs, ups)
    with torch.no_grad():
        U, Pr, _ = self_atte(X, P["Ms"], P["Ws"].view(AT))
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad
    return ((U, Pr, wsoft.detach().sum(-1), sa.detach(), senti.detach()),
            (zero(X), zero(P["Ms"]), zero(P["Ws"]).view(AT), zero(wsoft)))


def check_decisions(x, Y, cmax, argl, sp, view_p, view_score=None, thr=THR32):
    """Every saved tensor and decision of the HIP head forward (and, when view_score is given, of the gate) against float64.
    x holds the operands the GEMM multiplied (bf16_operands(x) for the bf16 entry).  Y [N][L][KC] as the kernel wrote it:
      * the first Lout positions are within rounding_delta of relu(conv64);
      * argl lies in [0, Lout), and argl / cmax are bit-exactly the first index and the value of the maximum of the HIP Y over
        l < Lout - index work bit-exact;
      * view_p is bit-exactly where(sp < float32(thr), 0, sp) of the HIP sp;
      * with sp64 recomputed in float64 from the HIP argl, every threshold decision agrees with sp64 >= thr;
      * with view_score recomputed in float64 from the HIP argl and threshold decisions, every gate side agrees with > 0.5.
    Returns (list of failure strings, stats); stats records the largest |Y - Y64| / delta for a later tightening, the
    smallest distances of the float64 values from the two thresholds, and the share of ties, dead filters and padded
    argmaxes among the HIP decisions."""
    B, S, L, V, KS, KC = x["dims"]
    N, Lo = B * S, lout(L, KS)
    Y, cmax, sp, view_p = (t.detach().cpu().float() for t in (Y, cmax, sp, view_p))
    Y, cmax, sp, view_p = Y.reshape(N, L, KC), cmax.reshape(N, KC), sp.reshape(N, V), view_p.reshape(N, V)
    argl = argl.detach().cpu().long().reshape(N, KC)
    fails, stats = [], {}
    Yv = Y[:, :Lo]
    for name, t in (("Y", Yv), ("cmax", cmax), ("sp", sp), ("view_p", view_p)):
        if not bool(torch.isfinite(t).all()):
            fails.append(f"{name}: not finite ({int((~torch.isfinite(t)).sum())} entries)")
    Y64 = torch.relu(conv64(x["X"], x["Wc"], x["bc"], KS))
    delta = rounding_delta(x["X"], x["Wc"], x["bc"], KS)
    err = (Yv.double() - Y64).abs()
    over = torch.where(delta > 0, err / delta.clamp_min(1e-300), torch.where(err > 0, float("inf"), 0.0).double())
    over = torch.nan_to_num(over, nan=float("inf"))
    stats["y_over_delta"] = float(over.max())
    if stats["y_over_delta"] > 1:
        n, l, k = [int(v) for v in torch.nonzero(over > 1)[0]]
        fails.append(f"Y: {int((over > 1).sum())} entries further than delta from relu(conv64), worst {stats['y_over_delta']:.2f} "
                     f"delta, first [{n}][{l}][{k}] = {float(Yv[n, l, k])!r} against {float(Y64[n, l, k])!r}")
    inside = (argl >= 0) & (argl < Lo)
    if not bool(inside.all()):
        n, k = [int(v) for v in torch.nonzero(~inside)[0]]
        fails.append(f"argl: {int((~inside).sum())} indices outside [0, {Lo}), first [{n}][{k}] = {int(argl[n, k])}")
        return fails, stats
    m, first = first_argmax(Yv)
    wrong = argl != first
    if bool(wrong.any()):
        n, k = [int(v) for v in torch.nonzero(wrong)[0]]
        fails.append(f"argl: {int(wrong.sum())} entries are not the first index of the maximum of Y over l < {Lo}, first "
                     f"[{n}][{k}] = {int(argl[n, k])} instead of {int(first[n, k])} (Y there {float(Yv[n, argl[n, k], k])!r}, "
                     f"maximum {float(m[n, k])!r})")
    if not torch.equal(cmax, m):
        fails.append(f"cmax: {int((cmax != m).sum())} entries differ from the maximum of Y over l < {Lo}")
    want_vp = torch.where(sp < torch.tensor(thr, dtype=torch.float32), torch.zeros_like(sp), sp)
    if not torch.equal(view_p, want_vp):
        fails.append(f"view_p: {int((view_p != want_vp).sum())} entries differ from where(sp < {thr!r}, 0, sp)")
    kept = view_p > 0
    f = forward64(x, argl, kept)
    stats["sp_margin"] = float((f.sp - thr).abs().min())
    bad = kept != (f.sp >= thr)
    if bool(bad.any()):
        n, v = [int(i) for i in torch.nonzero(bad)[0]]
        fails.append(f"threshold: {int(bad.sum())} decisions differ from sp64 >= thr, first [{n}][{v}]: kept {bool(kept[n, v])}, "
                     f"sp64 = {float(f.sp[n, v])!r}, HIP sp = {float(sp[n, v])!r}")
    tied = ((Yv == m.unsqueeze(1)).sum(1) > 1) & (m > 0)
    padded = argl >= x["lengths"].view(N, 1)
    stats.update(dead=float((m <= 0).double().mean()), tied_live=float(tied.double().sum() / max(1, int((m > 0).sum()))),
                 padded=float(padded.double().mean()))
    if view_score is not None:
        vs = view_score.detach().cpu().float().reshape(B, V)
        if not bool(torch.isfinite(vs).all()):
            fails.append("view_score: not finite")
        _, _, sa = self_atte(x.get("X_snet", x["X"]).double(), x["Ms"].double(), x["Ws"].double())
        g = gate_forward64(sa.view(B, S, D), x["ssW"], x["ssb"], f.view_p.view(B, S, V), f.final)
        stats["vs_margin"] = float((g.vs - 0.5).abs().min())
        bad = (vs > 0.5) != g.side
        if bool(bad.any()):
            b, v = [int(i) for i in torch.nonzero(bad)[0]]
            fails.append(f"gate: {int(bad.sum())} sides differ from vs64 > 0.5, first [{b}][{v}]: vs64 = {float(g.vs[b, v])!r}, "
                         f"HIP view_score = {float(vs[b, v])!r}")
    return fails, stats


def evaluate32(x, thr=THR32):
    """The float32 CPU evaluation of the head and gate forward with its own decisions, in the layout of the HIP outputs: Y
    [N][L][KC] (all L positions of the window GEMM), cmax, argl, sp, view_p, final, view_score."""
    B, S, L, V, KS, KC = x["dims"]
    Y = torch.relu(_conv(x["X"], x["Wc"], x["bc"], KS, full=True))
    cmax, argl = first_argmax(Y[:, :lout(L, KS)])
    sp = torch.sigmoid(cmax @ x["Wl"].t() + x["bl"])
    vp = torch.where(sp < torch.tensor(thr, dtype=torch.float32), torch.zeros_like(sp), sp)
    final = (vp * vp).view(B, S, V).sum(1)
    _, _, sa = self_atte(x["X"], x["Ms"], x["Ws"])
    g = gate_forward64(sa.view(B, S, D), x["ssW"], x["ssb"], vp.view(B, S, V), final, dtype=torch.float32)
    return SimpleNamespace(Y=Y, cmax=cmax, argl=argl.int(), sp=sp, view_p=vp, final=final, view_score=g.vs)


def median_and_least_route(parts, alive, argl, Lo):
    """((n, k) of the live entry with the median |dc|, (n, k) of the live entry with the smallest non-zero |dc|) among the
    entries that have a next valid position, argl + 1 < Lo; None where there is no such entry"""
    dc = parts["dc"].abs()
    ok = alive.cpu().bool() & (argl.cpu().long() + 1 < Lo) & (dc > 0)
    idx = torch.nonzero(ok)
    if idx.shape[0] == 0:
        return None, None
    w = dc[ok]
    order = w.argsort()
    med, least = idx[order[(len(order) - 1) // 2]], idx[order[0]]
    return (int(med[0]), int(med[1])), (int(least[0]), int(least[1]))


def conditions(x):
    """What the reference alone says about one shape's inputs (float64): the facts test_conditions asserts."""
    B, S, L, V, KS, KC = x["dims"]
    N, Lo = B * S, lout(L, KS)
    d = decisions64(x)
    full = conv64(x["X"], x["Wc"], x["bc"], KS, full=True)
    Y = d.f.Y
    m = Y.max(1).values
    live = m > 0
    c = {"sp_margin": float((d.f.sp - THR32).abs().min()), "vs_margin": float((d.gate.vs - 0.5).abs().min()),
         "dead": float((~live).double().mean()), "n_tied_live": int((((Y == m.unsqueeze(1)).sum(1) > 1) & live).sum()),
         "n_live": int(live.sum()), "n_padded": int((d.argl >= x["lengths"].view(N, 1)).sum()),
         "n_excluded_wins": int((full[:, L - 1] > full[:, :Lo].max(1).values).sum()) if Lo < L else None,
         "sides": (int(d.gate.side.sum()), int((~d.gate.side).sum())),
         "n_zero_columns": int((d.f.view_p.view(B, S, V) == 0).all(1).sum()), "n_kept": int(d.f.kept.sum())}
    return c
