"""Decision-conditioned reference of the R-Net co-attention (test helper, not a test module; CPU only).

umpr_amd/csrc/coattn.hip never stores A = tanh(G_i M G_u^T): the forward keeps the column and row maxima with their first
argmax, and the backward is routed through those indices.  Which index wins is a decision; once the decisions are fixed the
backward is a smooth function of every value.  The functions here
  * compute the scores in float64 (scores64) and check every decision the HIP forward took against them within the a-priori
    rounding of a float32 evaluation (rounding_delta, check_decisions),
  * run the backward in float64 - or, for the yardstick, in float32 - with the decisions given (backward64), and
  * compare a HIP gradient with the float64 one at a bound that is a small multiple K of the distance the float32 CPU
    evaluation of the very same formula has (gate).
tests/test_coattn_decisions.py checks them against autograd on the CPU; tests/test_gpu_coattn.py uses them on the GPU.
"""
import torch

D = 128                     # 2 * gru_size, the only width the kernels are built for
EPS32 = 2.0 ** -24          # unit roundoff of float32
FLOOR = 2.0 ** -22          # gate: smallest distance the float32 yardstick is credited with
K_START, K_MAX = 4.0, 14.0  # gate factor: where it starts and what it may never exceed
# The factor the GPU tests use.  Worst measured ratio of a HIP distance to the floored float32 CPU distance:
# see profiles/r04_c_coattn_gates.txt - below 2, so K stays at its starting value.
K = K_START
SHAPES = ((2, 1), (2, 63), (1, 64), (3, 65), (2, 130), (3, 400))      # (B, SL) of the GPU tests


def make_inputs(B, SL, seed=None, m_scale=0.01):
    """The seeded inputs of one shape: Gu, Gi = 0.5 randn, M = m_scale randn, the four upstream gradients randn."""
    g = torch.Generator().manual_seed(1000 * B + SL if seed is None else seed)
    rn = lambda *s: torch.randn(*s, generator=g)
    return {"Gu": 0.5 * rn(B, SL, D), "Gi": 0.5 * rn(B, SL, D), "M": m_scale * rn(D, D),
            "d_atte_u": rn(B, D), "d_atte_i": rn(B, D), "d_soft_u": rn(B, SL), "d_soft_i": rn(B, SL)}


def bf16_round(x):
    """x rounded to bf16 (round to nearest even, as the staging of coattn_scores_bf16_kernel does), as float32"""
    return x.float().bfloat16().float()


def scores64(T, Gu):
    """tanh(T Gu^T) in float64: [B][SL(j)][SL(k)]"""
    return torch.tanh(T.double() @ Gu.double().transpose(-1, -2))


def rounding_delta(T, Gu):
    """delta[b][j][k] = 2 * 128 * 2^-24 * sum_c |T[j,c]| |Gu[k,c]| + 4 * 2^-24: the a-priori bound of a 128-term float32 dot
    product whose left operand carries the rounding of its own 128-term product (T = Gi M), through the 1-Lipschitz tanh, plus
    four units for tanhf's last bits.  Derived, not measured."""
    return 2 * D * EPS32 * (T.double().abs() @ Gu.double().abs().transpose(-1, -2)) + 4 * EPS32


def check_decisions(A64, T, Gu, argcol, colmax, argrow, rowmax):
    """Every saved decision of the forward against the float64 scores A64 [B][SL][SL].  For a column k with j* = argcol[k]:
    0 <= j* < SL; A64[j*, k] is within the rounding of the column's float64 maximum; colmax[k] is within delta of
    A64[j*, k].  Rows alike.  A float32 evaluation a with |a - A64| <= delta that picked j* has a[j*] >= a[j] for every j,
    hence A64[j*, k] + delta[j*, k] >= A64[j, k] - delta[j, k]: that is the `max - 2 delta` of equal deltas, with each
    entry's own delta.  Returns (list of failure strings, stats): stats holds, per side, the largest observed
    |value error| / delta and (max - chosen) / (sum of the two deltas) - the record for a later tightening."""
    B, SL, _ = A64.shape
    delta = rounding_delta(T, Gu)
    fails, stats = [], {}
    for side, arg, val, dim in (("col", argcol, colmax, 1), ("row", argrow, rowmax, 2)):
        arg, val = arg.cpu().long(), val.cpu().double()
        assert arg.shape == (B, SL) and val.shape == (B, SL), (side, arg.shape, val.shape)
        inside = (arg >= 0) & (arg < SL)
        if not bool(inside.all()):
            b, p = [int(v) for v in torch.nonzero(~inside)[0]]
            fails.append(f"arg{side}: {int((~inside).sum())} indices outside [0, {SL}), first [{b}][{p}] = {int(arg[b, p])}")
            stats[side] = (float("nan"), float("nan"))
            continue
        chosen = A64.gather(dim, arg.unsqueeze(dim)).squeeze(dim)           # A64 at the decision
        d_chosen = delta.gather(dim, arg.unsqueeze(dim)).squeeze(dim)
        best_low = (A64 - delta).max(dim).values                           # max_j (A64[j] - delta[j])
        slack = chosen + d_chosen - best_low                               # >= 0 for a legitimate decision
        lead = A64.max(dim).values - chosen
        d_lead = delta.gather(dim, A64.argmax(dim).unsqueeze(dim)).squeeze(dim)
        r_arg = float((lead / (d_chosen + d_lead)).max())
        r_val = float(((val - chosen).abs() / d_chosen).max())
        stats[side] = (r_val, r_arg)
        if not bool(torch.isfinite(val).all()):
            fails.append(f"{side}max: not finite")
        n_arg = int((slack < 0).sum())
        if n_arg:
            b, p = [int(v) for v in torch.nonzero(slack < 0)[0]]
            fails.append(f"arg{side}: {n_arg} decisions are not a float64 maximum within rounding, first [{b}][{p}] = "
                         f"{int(arg[b, p])}: {float(lead[b, p]):.3e} below the maximum, delta {float(d_chosen[b, p]):.3e}")
        n_val = int(((val - chosen).abs() > d_chosen).sum())
        if n_val:
            fails.append(f"{side}max: {n_val} values further than delta from A64 at their index, worst {r_val:.2f} delta")
    return fails, stats


def forward64(Gu, Gi, A, argcol, argrow, dtype=torch.float64):
    """soft_u, soft_i, atte_u, atte_i (src/model.py:52-55) with the maxima taken at the given decisions."""
    ac, ar = argcol.cpu().long(), argrow.cpu().long()
    A, Gu, Gi = A.to(dtype), Gu.to(dtype), Gi.to(dtype)
    cm = A.gather(1, ac.unsqueeze(1)).squeeze(1)             # cm[k] = A[argcol[k], k]
    rm = A.gather(2, ar.unsqueeze(2)).squeeze(2)             # rm[j] = A[j, argrow[j]]
    soft_u, soft_i = torch.softmax(cm, -1), torch.softmax(rm, -1)
    atte_u = (Gu * soft_u.unsqueeze(-1)).sum(1)
    atte_i = (Gi * soft_i.unsqueeze(-1)).sum(1)
    return cm, rm, soft_u, soft_i, atte_u, atte_i


def backward64(Gu, Gi, M, T, A, argcol, argrow, d_atte_u, d_atte_i, d_soft_u=None, d_soft_i=None, dtype=torch.float64,
               parts=None, saved_at=None):
    """(dGu, dGi, dM) of the co-attention with the argmax decisions given, in `dtype` (float64: the reference; float32: the
    yardstick `ref32` of gate).  A [B][SL][SL] are the scores the maxima are read from at the decisions; T [B][SL][128] is
    the left operand the routed products use (G_i M; in the bf16 path A comes from the rounded operands and T stays the
    unrounded one, as the kernels differentiate the float32 function at the rounded forward values).
        ds_u[k]   = d_soft_u[k] + Gu[k] . d_atte_u
        dS_col[k] = soft_u[k] (ds_u[k] - sum soft_u ds_u) (1 - cm[k]^2)                       (item side by symmetry)
        dGu[k]    = soft_u[k] d_atte_u + dS_col[k] T[argcol[k]] + sum_{j: argrow[j] = k} dS_row[j] T[j]
        dT[j]     = dS_row[j] Gu[argrow[j]] + sum_{k: argcol[k] = j} dS_col[k] Gu[k]
        dGi       = soft_i (x) d_atte_i + dT M^T            dM = Gi^T dT
    A dict passed as `parts` receives dS_col, dS_row and dT.  `saved_at` = (argcol, argrow) makes the maxima, and with them
    soft_* and the 1 - max^2 factors, those of OTHER decisions than the routing ones: a backward that misroutes while the
    forward's saved colmax / rowmax / soft_* are right - what umpr_coattention_bwd does when handed one altered index.
    """
    cm, rm, soft_u, soft_i, _, _ = forward64(Gu, Gi, A, *(saved_at or (argcol, argrow)), dtype)
    Gu, Gi, M, T = Gu.to(dtype), Gi.to(dtype), M.to(dtype), T.to(dtype)
    dau, dai = d_atte_u.to(dtype), d_atte_i.to(dtype)
    ac = argcol.cpu().long().unsqueeze(-1).expand(-1, -1, D)
    ar = argrow.cpu().long().unsqueeze(-1).expand(-1, -1, D)
    ds_u = (Gu @ dau.unsqueeze(-1)).squeeze(-1)
    ds_i = (Gi @ dai.unsqueeze(-1)).squeeze(-1)
    if d_soft_u is not None:
        ds_u = ds_u + d_soft_u.to(dtype)
    if d_soft_i is not None:
        ds_i = ds_i + d_soft_i.to(dtype)
    dS_col = soft_u * (ds_u - (soft_u * ds_u).sum(-1, keepdim=True)) * (1 - cm * cm)
    dS_row = soft_i * (ds_i - (soft_i * ds_i).sum(-1, keepdim=True)) * (1 - rm * rm)
    dGu = soft_u.unsqueeze(-1) * dau.unsqueeze(1) + dS_col.unsqueeze(-1) * T.gather(1, ac)
    dGu.scatter_add_(1, ar, dS_row.unsqueeze(-1) * T)
    dT = dS_row.unsqueeze(-1) * Gu.gather(1, ar)
    dT.scatter_add_(1, ac, dS_col.unsqueeze(-1) * Gu)
    dGi = soft_i.unsqueeze(-1) * dai.unsqueeze(1) + dT @ M.t()
    dM = torch.einsum("bjc,bjd->cd", Gi, dT)
    if parts is not None:
        parts.update(dS_col=dS_col, dS_row=dS_row, dT=dT)
    return dGu, dGi, dM


def runner_up(A64, b, k):
    """(first, second) row of column k of sample b by float64 score"""
    top = A64[b, :, k].topk(2).indices
    return int(top[0]), int(top[1])


def distances(got, ref):
    """(max |got - ref| / max |ref|, relative L2) in float64.  Where the reference is identically zero - dM at SL = 1,
    where the softmax over one position is the constant 1 - the only result at distance 0 is exact zero.  Computed where `ref`
    lives (the CPU everywhere but for the 103 M-element classifier gradients, whose reference is held on the device)."""
    ref = ref.detach().double()
    got = got.detach().to(ref.device).double()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    scale, norm = float(ref.abs().max()), float(ref.norm())
    if scale == 0.0:
        z = 0.0 if bool((got == 0).all()) else float("inf")
        return z, z
    return float((got - ref).abs().max()) / scale, float((got - ref).norm()) / norm


def gate(got, ref, ref32, names=("dGu", "dGi", "dM"), K=K, log=None, tag=""):
    """Per tensor: both distances of `got` from the float64 `ref` must be within K x the same distance of `ref32` (the
    float32 CPU evaluation of the same formula with the same decisions), floored at 2^-22.  Every tensor is logged before
    anything is judged.  Returns (all passed, rows); a row is a dict with name, d_max, d_l2 (got), r_max, r_l2 (ref32),
    ratio (worst distance / floored ref32 distance), over (worst distance / bound) and ok."""
    assert K <= K_MAX, K
    rows = []
    for name, g, r, r32 in zip(names, got, ref, ref32):
        finite = bool(torch.isfinite(g).all())
        d_max, d_l2 = distances(g, r) if finite else (float("inf"), float("inf"))
        r_max, r_l2 = distances(r32, r)
        ratio = max(d_max / max(r_max, FLOOR), d_l2 / max(r_l2, FLOOR))
        row = {"name": name, "d_max": d_max, "d_l2": d_l2, "r_max": r_max, "r_l2": r_l2, "ratio": ratio, "over": ratio / K,
               "ok": finite and ratio <= K}
        rows.append(row)
        if log is not None:
            log(f"{tag} {name}: max/max={d_max:.3e} rel_l2={d_l2:.3e} | ref32 max/max={r_max:.3e} rel_l2={r_l2:.3e} | "
                f"ratio={ratio:.2f} K={K:g} ref_max={float(r.abs().max()):.3e}{'' if row['ok'] else '  OUTSIDE'}")
    return all(r["ok"] for r in rows), rows
