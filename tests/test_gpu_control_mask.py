"""`--mask_control True` and `--unsort_gru True` on the GPU: umpr_cnet_head_fwd_masked (+ the unchanged umpr_cnet_head_bwd), the
general fused entry points umpr_review_net_fwd_ex / _bwd_ex and umpr_control_net_fwd_ex / _bwd_ex, and the two model options.

The yardsticks are the merged ones.  A masked head case is compacted - every defined sentence cut to its n_s - and then goes through
check_decisions, forward64 / backward64 and gate of tests/control_decisions.py at its K, unchanged.  What the mask adds is checked
exactly: -1 / +0.0 at undefined sentences, +0.0 gradients there, all-valid masks giving the bits of umpr_cnet_head_fwd, no NaN from
a sample without a defined sentence.  Every call runs on NaN-filled, guard-banded outputs and a NaN-filled workspace (the fused
entries: a NaN-filled arena too).  The invariance batch and the quantity each one-off leg is held on are fixed on the CPU
(tests/test_control_mask_reference.py::test_invariance_batch).
"""
import os
from types import SimpleNamespace

import pytest
import torch

import control_decisions as C
import control_mask_reference as K
import masked_attention_reference as MA
from test_control_mask_reference import INV_SEED
from test_gpu_mask_padding import Banded, _bits, _nan, _ws
from test_gpu_parity import LOG as PARITY_LOG
from test_gpu_parity import L, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "control_mask.log")
D, AT = C.D, C.AT
PARITY = K.PARITY
WORST = {"ratio": 0.0, "where": ""}


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def _gate(tag, names, got, ref, ref32):
    ok, rows = C.gate(got, ref, ref32, names=names, K=C.K, log=log, tag=tag)
    for r in rows:
        if r["ratio"] == r["ratio"] and r["ratio"] > WORST["ratio"]:
            WORST.update(ratio=r["ratio"], where=f"{tag} {r['name']}")
    log(f"worst gate ratio so far: {WORST['ratio']:.3f} ({WORST['where']}); K = {C.K}")
    assert ok, [(r["name"], r["d_max"], r["r_max"], r["ratio"]) for r in rows if not r["ok"]]


# ==================================================================================================== umpr_cnet_head_fwd_masked
# (B, S, L, V, KS, KC, pattern): one wave; a full block of 4 waves + a second block; a partial block; L above one ballot; KC = 4 / 120 /
# 512 (one lane trip with idle lanes, two, eight); every KS of 1..4; V = 1 and 4
HEAD_CASES = [(1, 1, 1, 1, 1, 4, "all"), (1, 1, 1, 1, 3, 4, "none"), (2, 4, 7, 4, 2, 120, "ragged"), (2, 4, 7, 1, 3, 120, "ragged"),
              (3, 5, 20, 4, 4, 512, "ragged"), (1, 9, 65, 4, 3, 120, "ragged"), (1, 9, 65, 1, 2, 4, "ragged"), (3, 5, 20, 4, 3, 120, "all"),
              (2, 4, 7, 4, 4, 120, "all")]


def _head_problem(B, S, Lm, V, KS, KC, pattern):
    """make_inputs' parameters and upstream gradients with an X and a validity of this file's: tokens[n] real tokens per sentence
    (X zero past max(tokens, 1): the GRU runs one step on a padded sentence, so its row 0 is NOT zero).  ragged: sentence 0 full, 1
    one token, 2 padded, 3 with a hole at token 1 (n_s = 1; X is live behind the hole), the rest uniform in 0..L; the last sample of
    B >= 2 is all padded - no defined sentence; in L = 65 sentence 4 has its only hole at token 64 (the second ballot)."""
    x = C.make_inputs(B, S, Lm, V, KS, KC)
    N = B * S
    g = torch.Generator().manual_seed(900 + 31 * B + 7 * S + Lm + KS)
    tokens = torch.randint(0, Lm + 1, (N,), generator=g)
    hole = torch.full((N,), -1)
    if pattern == "all":
        tokens[:] = Lm
    elif pattern == "none":
        tokens[:] = 0
    else:
        tokens[0] = Lm
        if N > 1:
            tokens[1] = 1
        if N > 2:
            tokens[2] = 0
        if N > 3 and Lm >= 3:
            tokens[3], hole[3] = min(Lm, 5), 1
        if N > 4 and Lm > 64:
            tokens[4], hole[4] = Lm, 64
        if B >= 2:
            tokens[(B - 1) * S:] = 0
    X = 0.7 * torch.randn(N, Lm, D, generator=g)
    X = X * (torch.arange(Lm).view(1, Lm, 1) < tokens.clamp(min=1).view(N, 1, 1))
    valid = torch.arange(Lm).view(1, Lm) < tokens.view(N, 1)
    for n in range(N):
        if hole[n] >= 0:
            valid[n, hole[n]] = False
    x["X"] = X.contiguous()
    x["lengths"] = tokens.clamp(min=1)
    ns = K.leading_run(valid)
    return x, valid, ns, hole


def _head_forward(L, dev, x, valid, masked=True):
    B, S, Lm, V, KS, KC = x["dims"]
    d = {k: x[k].to(dev).contiguous() for k in ("X", "Wc", "bc", "Wl", "bl")}
    o = SimpleNamespace(Y=_nan(dev, B, S, Lm, KC), cmax=Banded(dev, (B, S, KC)), sp=Banded(dev, (B, S, V)), view_p=Banded(dev, (B, S, V)),
                        final=Banded(dev, (B, V)), argl=Banded(dev, (B, S, KC), torch.int32, -7), **d)
    ws, wsb = _ws(L, dev, "umpr_cnet_head_fwd_ws_bytes", B, S, Lm, KS)
    head = (o.X, o.Wc, o.bc, o.Wl, o.bl, float(C.THR32), B, S, Lm, KC, KS, V, o.Y, o.cmax.t, o.argl.t, o.sp.t, o.view_p.t, o.final.t)
    if masked:
        o.valid = valid.to(dev).to(torch.uint8).contiguous()
        L.call("umpr_cnet_head_fwd_masked", *head, o.valid, ws, wsb, st())
    else:
        L.call("umpr_cnet_head_fwd", *head, ws, wsb, st())
    torch.cuda.synchronize()
    for name in ("cmax", "sp", "view_p", "final", "argl"):
        assert getattr(o, name).intact(), f"{name}: written outside its buffer"
    return o


@pytest.mark.parametrize("case", HEAD_CASES, ids=lambda c: "-".join(str(v) for v in c))
def test_masked_head(L, dev, case):
    B, S, Lm, V, KS, KC, pattern = case
    x, valid, ns, hole = _head_problem(*case)
    N = B * S
    o = _head_forward(L, dev, x, valid)
    Y, cmax, argl = o.Y.cpu().view(N, Lm, KC), o.cmax.t.cpu().view(N, KC), o.argl.t.cpu().view(N, KC).long()
    sp, vp, fin = o.sp.t.cpu().view(N, V), o.view_p.t.cpu().view(N, V), o.final.t.cpu()
    lo = C.lout(ns, KS)
    und = lo < 1
    tag = f"masked head {case}"
    # ---- the conventions, bit for bit
    for name, t in (("cmax", cmax), ("sp", sp), ("view_p", vp)):
        assert bool((_bits(t)[und] == 0).all()), f"{name} of an undefined sentence is not +0.0"
        assert bool(torch.isfinite(t).all()), name
    assert bool((argl[und] == -1).all()) and bool(((argl[~und] >= 0) & (argl[~und] < lo[~und].view(-1, 1))).all())
    want_fin = (vp.double().view(B, S, V) ** 2).sum(1)               # cnet_final_kernel, unchanged: S fused multiply-adds in float32
    assert bool(((fin.double() - want_fin).abs() <= S * C.EPS32 * want_fin).all()), (fin, want_fin)
    empty = und.view(B, S).all(1)
    assert bool((_bits(fin)[empty] == 0).all()), "a sample without a defined sentence: final is not +0.0"
    if pattern == "ragged":
        assert bool(und.any()) and bool((~und).any()) and (B < 2 or bool(empty.any()))
        assert int(ns[3]) == 1 and bool(und[1]) == (KS % 2 == 0)       # the hole; one token under an even KS
        if Lm > 64:
            assert int(ns[4]) == 64
    # ---- all valid: the bits of the unmasked entry
    if pattern == "all":
        u = _head_forward(L, dev, x, valid, masked=False)
        for name in ("cmax", "argl", "sp", "view_p", "final"):
            assert torch.equal(_bits(getattr(o, name).t), _bits(getattr(u, name).t)), name
        assert torch.equal(_bits(o.Y), _bits(u.Y))
    # ---- the backward, unchanged, on the masked forward's saved tensors
    grads = None
    if KC % 4 == 0:
        dX, w = _nan(dev, N, Lm, D), [_nan(dev, *s) for s in ((KC, D, KS), (KC,), (V, KC), (V,))]
        ws, wsb = _ws(L, dev, "umpr_cnet_head_bwd_ws_bytes", B, S, Lm, KC, KS, V)
        L.call("umpr_cnet_head_bwd", o.X, o.Wc, o.Wl, o.cmax.t, o.argl.t, o.sp.t, o.view_p.t, x["d_final"].to(dev).contiguous(),
               x["d_view_p"].to(dev).contiguous(), B, S, Lm, KC, KS, V, dX, 0, 0, *w, ws, wsb, st())
        torch.cuda.synchronize()
        grads = [dX.cpu()] + [t.cpu() for t in w]
        for name, t in zip(C.HEAD_GRADS, grads):
            assert bool(torch.isfinite(t).all()), f"{name} is not finite"
        assert bool((_bits(grads[0])[und] == 0).all()), "dX of an undefined sentence is not +0.0"
    # ---- compaction: every defined sentence cut to n_s, through the merged yardsticks.  (A sentence with a hole stays uncut: the
    # windows of its eligible positions reach behind the hole, so its Y is the padded width's; its decisions are checked directly and
    # the decision-conditioned forward64 / backward64 then run on the whole row.)
    f64, f32, b64, b32, got_f, got_dX, inside_dX = [], [], None, None, [], [], []
    stats_all = {}
    for n in range(N):
        if und[n]:
            continue
        m = int(ns[n]) if hole[n] < 0 else Lm
        b = n // S
        xs = dict(x)
        xs.update(dims=(1, 1, m, V, KS, KC), X=x["X"][n:n + 1, :m].contiguous(), lengths=torch.tensor([m]), d_final=x["d_final"][b:b + 1],
                  d_view_p=x["d_view_p"][b:b + 1, n % S:n % S + 1])
        if hole[n] >= 0:
            first = C.first_argmax(Y[n:n + 1, :int(lo[n])])
            assert torch.equal(cmax[n], first[0][0]) and torch.equal(argl[n], first[1][0])
            assert torch.equal(vp[n], torch.where(sp[n] < torch.tensor(C.THR32), torch.zeros_like(sp[n]), sp[n]))
        else:
            fails, stats = C.check_decisions(xs, Y[n:n + 1, :m], cmax[n:n + 1], argl[n:n + 1], sp[n:n + 1], vp[n:n + 1])
            assert not fails, (n, fails)
            stats_all[n] = stats["y_over_delta"]
        kept, alive = vp[n:n + 1] > 0, cmax[n:n + 1] > 0
        f64.append(C.forward64(xs, argl[n:n + 1], kept)); f32.append(C.forward64(xs, argl[n:n + 1], kept, dtype=torch.float32))
        got_f.append((sp[n:n + 1], vp[n:n + 1]))
        if grads is not None:
            r64 = C.backward64(xs, argl[n:n + 1], alive, kept, xs["d_final"], xs["d_view_p"])
            r32 = C.backward64(xs, argl[n:n + 1], alive, kept, xs["d_final"], xs["d_view_p"], dtype=torch.float32)
            got_dX.append(grads[0][n, :m].reshape(-1)); inside_dX.append((r64[0].reshape(-1), r32[0].reshape(-1)))
            b64 = list(r64[1:]) if b64 is None else [a + c for a, c in zip(b64, r64[1:])]
            b32 = list(r32[1:]) if b32 is None else [a + c for a, c in zip(b32, r32[1:])]
    log(f"{tag}: {len(f64)} sentences compacted, worst |Y - Y64| / delta {max(stats_all.values(), default=0):.3f}")
    if f64:
        cat = lambda fs, k: torch.cat([getattr(f, k) for f in fs])
        _gate(f"{tag} forward", ("sp", "view_p"), (torch.cat([g[0] for g in got_f]), torch.cat([g[1] for g in got_f])),
              (cat(f64, "sp"), cat(f64, "view_p")), (cat(f32, "sp"), cat(f32, "view_p")))
    if grads is not None and b64 is not None:
        _gate(f"{tag} backward", C.HEAD_GRADS, [torch.cat(got_dX)] + grads[1:], [torch.cat([a for a, _ in inside_dX])] + b64,
              [torch.cat([c for _, c in inside_dX])] + b32)


def test_masked_head_refuses_a_null_mask(L, dev):
    x, valid, _, _ = _head_problem(2, 4, 7, 4, 3, 120, "ragged")
    B, S, Lm, V, KS, KC = x["dims"]
    d = [x[k].to(dev).contiguous() for k in ("X", "Wc", "bc", "Wl", "bl")]
    outs = [_nan(dev, B, S, Lm, KC), _nan(dev, B, S, KC), torch.full((B, S, KC), -7, dtype=torch.int32, device=dev), _nan(dev, B, S, V),
            _nan(dev, B, S, V), _nan(dev, B, V)]
    ws, wsb = _ws(L, dev, "umpr_cnet_head_fwd_ws_bytes", B, S, Lm, KS)
    rc = L.fn["umpr_cnet_head_fwd_masked"](*[t.data_ptr() for t in d], float(C.THR32), B, S, Lm, KC, KS, V, *[t.data_ptr() for t in outs],
                                           None, ws.data_ptr(), wsb, st())
    torch.cuda.synchronize()
    assert rc != 0 and "null validity mask" in L.last_error()
    assert all(bool(torch.isnan(t).all()) for i, t in enumerate(outs) if i != 2) and bool((outs[2] == -7).all())
    assert bool(torch.isnan(ws).all()), "the refused call wrote to its workspace"


# ============================================================================================================ the fused entry points
R_NAMES = ["review_net.r_net.M", "review_net.s_net_u.Ms", "review_net.s_net_u.Ws", "review_net.s_net_i.Ms", "review_net.s_net_i.Ws",
           "review_net.linear_u.weight", "review_net.linear_i.weight"]
C_NAMES = ["control_net.c_net.cnn.0.weight", "control_net.c_net.cnn.0.bias", "control_net.c_net.linear.0.weight",
           "control_net.c_net.linear.0.bias", "control_net.s_net.Ms", "control_net.s_net.Ws", "control_net.ss_net.linear.0.weight",
           "control_net.ss_net.linear.0.bias"]
FUSED_SHAPES = [(1, 1, 1, 1, 1), (3, 2, 5, 7, 9), (2, 5, 13, 5, 13)]          # (B, S_ui, L_ui, S, L)


def _gru_names(prefix):
    return [prefix + n + s for s in ("", "_reverse") for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]


def _fused_problem(dev, B, S_ui, L_ui, S, Lm, V=2, KS=3, KC=120):
    from umpr_amd.model import UMPR
    from umpr_amd.synthetic import make_param_state
    E, vocab = 50, 300
    P = make_param_state(17, E, vocab, V, False, with_vgg=False, m_scale=0.3, kernel_size=KS, kernel_count=KC)
    g = torch.Generator().manual_seed(5 + 100 * B + 10 * S + Lm)

    def side(n_sent, width):
        n = torch.randint(1, width + 1, (n_sent,), generator=g)
        n[0] = width
        t = torch.randint(0, vocab, (n_sent, width), generator=g) * (torch.arange(width).view(1, width) < n.view(n_sent, 1))
        if n_sent > 2:
            t[2], n[2] = 0, 1                                            # a padded sentence
        return t, n
    (iu, nu), (ii, ni), (iui, nui) = side(B * S, Lm), side(B * S, Lm), side(B * S_ui, L_ui)
    (lu, ou), (li, oi), (lui, oui) = UMPR._host_perm(nu, dev), UMPR._host_perm(ni, dev), UMPR._host_perm(nui, dev)
    N = B * S
    q = SimpleNamespace(E=E, V=V, KS=KS, KC=KC, emb=P["embedding.weight"].to(dev).contiguous(), N=N,
                        rp=[P[n].to(dev).contiguous() for n in _gru_names("review_net.r_net.gru.module.") + R_NAMES],
                        cp=[P[n].to(dev).contiguous() for n in _gru_names("control_net.c_net.gru.module.") + C_NAMES],
                        ids_pair=torch.cat([iu, ii]).to(dev).contiguous(), ids_ui=iui.to(dev).contiguous(),
                        lens=torch.cat([lu, li]).contiguous(), order=torch.cat([ou, oi + N]).contiguous(), lens_ui=lui.contiguous(),
                        ord_ui=oui.contiguous())
    q.cp[13] = q.cp[13].view(-1).contiguous()
    perm = lambda n, off=0: (torch.randperm(n, generator=g) + off).to(torch.int32)
    q.dst = {"order": (q.order, q.ord_ui),
             "identity": (torch.arange(2 * N, dtype=torch.int32, device=dev), torch.arange(B * S_ui, dtype=torch.int32, device=dev)),
             "random": (torch.cat([perm(N), perm(N, N)]).to(dev), perm(B * S_ui).to(dev))}
    q.valid_pair = torch.empty(2 * N, Lm, dtype=torch.uint8, device=dev)
    q.valid_ui = torch.empty(B * S_ui, L_ui, dtype=torch.uint8, device=dev)
    return q


def _ptrs(ts):
    return torch.tensor([t.data_ptr() for t in ts], dtype=torch.int64)


@pytest.mark.parametrize("need_grad,b16", [(0, 0), (1, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize("shape", FUSED_SHAPES)
def test_review_net_ex(L, dev, shape, need_grad, b16):
    """umpr_review_net_fwd_ex / _bwd_ex: bit-equal to the stage chain for dst = order, the identity and a random permutation, with and
    without the mask; with dst = order bit-equal to umpr_review_net_fwd / _fwd_masked / _bwd_dx (arena, output, every gradient)."""
    from umpr_amd._lib import TLS
    B, _, _, S, Lm = shape
    q = _fused_problem(dev, *shape)
    N, SL, E = q.N, S * Lm, q.E
    L.call("umpr_token_mask", q.ids_pair, q.lens, 2 * N, Lm, 0, q.valid_pair, st())
    pp = _ptrs(q.rp)
    na = L.size("umpr_review_net_arena_bytes", B, S, Lm) // 4
    gshapes = [t.shape for t in q.rp]
    d_out = torch.randn(B, D, generator=torch.Generator().manual_seed(3)).to(dev)

    def fused(kind, valid, ex=True):
        arena = _nan(dev, na + 64)
        ws, wsb = _ws(L, dev, "umpr_review_net_ws_bytes", B, S, Lm, E)
        out = Banded(dev, (B, D))
        if ex:
            L.call("umpr_review_net_fwd_ex", q.ids_pair, q.emb, E, pp.data_ptr(), q.lens, q.order, q.dst[kind][0], B, S, Lm, b16, b16,
                   need_grad, arena, out.t, ws, wsb, valid, st())
        elif valid is not None:
            L.call("umpr_review_net_fwd_masked", q.ids_pair, q.emb, E, pp.data_ptr(), q.lens, q.order, B, S, Lm, b16, b16, need_grad,
                   arena, out.t, ws, wsb, valid, st())
        else:
            L.call("umpr_review_net_fwd", q.ids_pair, q.emb, E, pp.data_ptr(), q.lens, q.order, B, S, Lm, b16, b16, need_grad, arena,
                   out.t, ws, wsb, st())
        torch.cuda.synchronize()
        assert out.intact() and bool(torch.isnan(arena[na:]).all())
        res = [out.t.clone()]
        if need_grad:
            G = [_nan(dev, *s) for s in gshapes]
            gp = _ptrs(G)            # stays alive across the call: the library reads this host array
            dx = _nan(dev, 2 * N * Lm, E)
            ws, wsb = _ws(L, dev, "umpr_review_net_ws_bytes", B, S, Lm, E)
            if ex:
                L.call("umpr_review_net_bwd_ex", q.ids_pair, q.emb, E, pp.data_ptr(), q.lens, q.order, q.dst[kind][0], B, S, Lm, b16,
                       arena, d_out, gp.data_ptr(), dx, ws, wsb, st())
            else:
                L.call("umpr_review_net_bwd_dx", q.ids_pair, q.emb, E, pp.data_ptr(), q.lens, q.order, B, S, Lm, b16, arena, d_out,
                       gp.data_ptr(), dx, ws, wsb, st())
            torch.cuda.synchronize()
            res += G + [dx]
        return res

    def staged(kind, valid):
        dst = q.dst[kind][0]
        TLS.gemm_b16 = bool(b16)
        try:
            gru, saved = _nan(dev, 2 * N, Lm, D), _nan(dev, 2, 2 * N, Lm, 4, 64)
            w, wb = _ws(L, dev, "umpr_embed_gru_bidir_ws_bytes", 2 * N, Lm, E)
            L.call("umpr_embed_gru_bidir_fwd", q.ids_pair, q.emb, E, *q.rp[:8], q.lens, q.order, dst, 2 * N, Lm, gru, saved if need_grad else None,
                   w, wb, st())
            gu, gi = gru[:N].view(B, SL, D), gru[N:].view(B, SL, D)
            T, su, si, cm, rm = (_nan(dev, B, SL, D), _nan(dev, B, SL), _nan(dev, B, SL), _nan(dev, B, SL), _nan(dev, B, SL))
            ac, ar = torch.full((B, SL), -7, dtype=torch.int32, device=dev), torch.full((B, SL), -7, dtype=torch.int32, device=dev)
            ru, ri = _nan(dev, B, 2 * D), _nan(dev, B, 2 * D)
            w, wb = _ws(L, dev, "umpr_coattention_fwd_ws_bytes", B, SL)
            co = (gu, gi, q.rp[8], B, SL, T, su, si, ru, 2 * D, ri, 2 * D, cm, ac, rm, ar)
            if valid is not None:
                vu, vi = valid[:N].view(B, SL), valid[N:].view(B, SL)
                L.call("umpr_coattention_fwd_masked", *co, vu, vi, b16, w, wb, st())
            else:
                vu = vi = None
                L.call("umpr_coattention_fwd_bf16" if b16 else "umpr_coattention_fwd", *co, w, wb, st())
            sn = []
            for X, Ms, Ws, soft, rep, v in ((gu, q.rp[9], q.rp[10], su, ru, vu), (gi, q.rp[11], q.rp[12], si, ri, vi)):
                s_ = SimpleNamespace(U=_nan(dev, N, Lm, AT), P=_nan(dev, N, Lm), wsum=_nan(dev, B, S), sa=_nan(dev, B, S, D))
                a = (X, Ms, Ws, soft, Lm, B, S, Lm, s_.U, s_.P, s_.wsum, s_.sa, rep.data_ptr() + 4 * D, 2 * D)
                L.call("umpr_snet_fwd_masked", *a, v, st()) if v is not None else L.call("umpr_snet_fwd", *a, st())
                sn.append(s_)
            out = _nan(dev, B, D)
            L.call("umpr_review_merge_fwd", ru, ri, q.rp[13], q.rp[14], B, out, st())
            res = [out]
            if need_grad:
                G = [_nan(dev, *s) for s in gshapes]
                dG, dru, dri, dsu, dsi = _nan(dev, 2 * N, Lm, D), _nan(dev, B, 2 * D), _nan(dev, B, 2 * D), _nan(dev, B, SL), _nan(dev, B, SL)
                w, wb = _ws(L, dev, "umpr_review_merge_bwd_ws_bytes", B)
                L.call("umpr_review_merge_bwd", ru, ri, q.rp[13], q.rp[14], out, d_out, B, dru, dri, G[13], G[14], w, wb, st())
                w, wb = _ws(L, dev, "umpr_snet_bwd_ws_bytes", B, S, Lm)
                for k, (X, s_, dr, ds) in enumerate(((gu, sn[0], dru, dsu), (gi, sn[1], dri, dsi))):
                    L.call("umpr_snet_bwd", X, q.rp[9 + 2 * k], q.rp[10 + 2 * k], s_.U, s_.P, s_.wsum, s_.sa, dr.data_ptr() + 4 * D, 2 * D, None, B, S,
                           Lm, Lm, dG[k * N:(k + 1) * N], G[9 + 2 * k], G[10 + 2 * k], ds, w, wb, st())
                w, wb = _ws(L, dev, "umpr_coattention_bwd_ws_bytes", B, SL)
                L.call("umpr_coattention_bwd", gu, gi, q.rp[8], T, su, si, cm, ac, rm, ar, dru, 2 * D, dri, 2 * D, dsu, dsi, B, SL, dG[:N], dG[N:],
                       G[8], 1, w, wb, st())
                dx = _nan(dev, 2 * N * Lm, E)
                w, wb = _ws(L, dev, "umpr_embed_gru_bidir_ws_bytes", 2 * N, Lm, E)
                L.call("umpr_embed_gru_bidir_bwd_dx", q.ids_pair, q.emb, E, q.rp[1], q.rp[5], q.lens, q.order, dst, 2 * N, Lm, dG, gru, saved, *G[:8],
                       0, q.rp[0], q.rp[4], dx, 0, w, wb, st())
                res += G + [dx]
        finally:
            TLS.gemm_b16 = False
        torch.cuda.synchronize()
        return res

    for kind in ("order", "identity", "random"):
        for valid in (None, q.valid_pair):
            a, b = fused(kind, valid), staged(kind, valid)
            assert len(a) == len(b)
            for k, (x_, y_) in enumerate(zip(a, b)):
                assert not bool(torch.isnan(x_).any()), (kind, k)
                assert torch.equal(_bits(x_), _bits(y_)), (kind, valid is not None, k)
            if kind == "order":
                for k, (x_, y_) in enumerate(zip(a, fused(kind, valid, ex=False))):
                    assert torch.equal(_bits(x_), _bits(y_)), ("existing entry", valid is not None, k)
    if B * S > 1:
        assert not torch.equal(fused("order", None)[0], fused("identity", None)[0]), "dst_row changes nothing"


@pytest.mark.parametrize("need_grad,b16", [(0, 0), (1, 0), (1, 1), (0, 1)])
@pytest.mark.parametrize("shape", FUSED_SHAPES)
def test_control_net_ex(L, dev, shape, need_grad, b16):
    """umpr_control_net_fwd_ex / _bwd_ex: bit-equal to the stage chain (two GRU calls, three heads, control S-Net, gate and their
    backwards in the fused order) for the three dst kinds, with and without the masks; with dst = order and no mask bit-equal to
    umpr_control_net_fwd / _bwd_dx; one NULL mask of the two is refused before anything is written."""
    from umpr_amd._lib import TLS
    B, S_ui, L_ui, S, Lm = shape
    q = _fused_problem(dev, *shape)
    N, Nui, E, V, KS, KC = q.N, B * S_ui, q.E, q.V, q.KS, q.KC
    L.call("umpr_token_mask", q.ids_pair, q.lens, 2 * N, Lm, 0, q.valid_pair, st())
    L.call("umpr_token_mask", q.ids_ui, q.lens_ui, Nui, L_ui, 0, q.valid_ui, st())
    pp = _ptrs(q.cp)
    dims = (B, S_ui, L_ui, S, Lm)
    na = L.size("umpr_control_net_arena_bytes", *dims, KC, V) // 4
    gshapes = [t.shape for t in q.cp]
    gen = torch.Generator().manual_seed(4)
    ups = [torch.randn(B, V, generator=gen).to(dev) for _ in range(4)]
    thr = float(C.THR32)

    def fused(kind, masked, ex=True):
        arena = _nan(dev, na + 64)
        ws, wsb = _ws(L, dev, "umpr_control_net_ws_bytes", *dims, E, KC, KS, V)
        outs = [Banded(dev, (B, V)) for _ in range(4)]
        dpair, dui = q.dst[kind]
        if ex:
            L.call("umpr_control_net_fwd_ex", q.ids_ui, q.ids_pair, q.emb, E, pp.data_ptr(), q.lens_ui, q.ord_ui, dui, q.lens, q.order, dpair,
                   *dims, KC, KS, V, thr, b16, need_grad, arena, *[o.t for o in outs], ws, wsb, q.valid_ui if masked else None,
                   q.valid_pair if masked else None, st())
        else:
            L.call("umpr_control_net_fwd", q.ids_ui, q.ids_pair, q.emb, E, pp.data_ptr(), q.lens_ui, q.ord_ui, q.lens, q.order, *dims, KC, KS,
                   V, thr, b16, need_grad, arena, *[o.t for o in outs], ws, wsb, st())
        torch.cuda.synchronize()
        assert all(o.intact() for o in outs) and bool(torch.isnan(arena[na:]).all())
        res = [o.t.clone() for o in outs]
        if need_grad:
            G = [_nan(dev, *s) for s in gshapes]
            gp = _ptrs(G)            # stays alive across the call: the library reads this host array
            dxp, dxu = _nan(dev, 2 * N * Lm, E), _nan(dev, Nui * L_ui, E)
            ws, wsb = _ws(L, dev, "umpr_control_net_ws_bytes", *dims, E, KC, KS, V)
            if ex:
                L.call("umpr_control_net_bwd_ex", q.ids_ui, q.ids_pair, q.emb, E, pp.data_ptr(), q.lens_ui, q.ord_ui, dui, q.lens, q.order,
                       dpair, *dims, KC, KS, V, b16, arena, *ups, gp.data_ptr(), dxp, dxu, ws, wsb, st())
            else:
                L.call("umpr_control_net_bwd_dx", q.ids_ui, q.ids_pair, q.emb, E, pp.data_ptr(), q.lens_ui, q.ord_ui, q.lens, q.order, *dims,
                       KC, KS, V, b16, arena, *ups, gp.data_ptr(), dxp, dxu, ws, wsb, st())
            torch.cuda.synchronize()
            res += G + [dxp, dxu]
        return res

    def staged(kind, masked):
        dpair, dui = q.dst[kind]
        P_ = q.cp
        TLS.gemm_b16 = bool(b16)
        try:
            g_ui, s_ui = _nan(dev, Nui, L_ui, D), _nan(dev, 2, Nui, L_ui, 4, 64)
            g_p, s_p = _nan(dev, 2 * N, Lm, D), _nan(dev, 2, 2 * N, Lm, 4, 64)
            w, wb = _ws(L, dev, "umpr_embed_gru_bidir_ws_bytes", Nui, L_ui, E)
            L.call("umpr_embed_gru_bidir_fwd", q.ids_ui, q.emb, E, *P_[:8], q.lens_ui, q.ord_ui, dui, Nui, L_ui, g_ui, s_ui if need_grad else None,
                   w, wb, st())
            w, wb = _ws(L, dev, "umpr_embed_gru_bidir_ws_bytes", 2 * N, Lm, E)
            L.call("umpr_embed_gru_bidir_fwd", q.ids_pair, q.emb, E, *P_[:8], q.lens, q.order, dpair, 2 * N, Lm, g_p, s_p if need_grad else None,
                   w, wb, st())
            X = (g_ui, g_p[:N], g_p[N:])
            ss, ll = (S_ui, S, S), (L_ui, Lm, Lm)
            vv = (q.valid_ui, q.valid_pair[:N], q.valid_pair[N:])
            h = []
            for k in range(3):
                o = SimpleNamespace(Y=_nan(dev, B, ss[k], ll[k], KC), cmax=_nan(dev, B, ss[k], KC), sp=_nan(dev, B, ss[k], V),
                                    vp=_nan(dev, B, ss[k], V), fin=_nan(dev, B, V),
                                    argl=torch.full((B, ss[k], KC), -7, dtype=torch.int32, device=dev))
                w, wb = _ws(L, dev, "umpr_cnet_head_fwd_ws_bytes", B, ss[k], ll[k], KS)
                a = (X[k], P_[8], P_[9], P_[10], P_[11], thr, B, ss[k], ll[k], KC, KS, V, o.Y, o.cmax, o.argl, o.sp, o.vp, o.fin)
                L.call("umpr_cnet_head_fwd_masked", *a, vv[k], w, wb, st()) if masked else L.call("umpr_cnet_head_fwd", *a, w, wb, st())
                h.append(o)
            sn = SimpleNamespace(U=_nan(dev, Nui, L_ui, AT), P=_nan(dev, Nui, L_ui), wsum=_nan(dev, B, S_ui), sa=_nan(dev, B, S_ui, D))
            a = (g_ui, P_[12], P_[13], h[0].vp, V, B, S_ui, L_ui, sn.U, sn.P, sn.wsum, sn.sa, _nan(dev, B, D), D)
            L.call("umpr_snet_fwd_masked", *a, q.valid_ui, st()) if masked else L.call("umpr_snet_fwd", *a, st())
            senti, vs, ppos, pneg = _nan(dev, B, S_ui), _nan(dev, B, V), _nan(dev, B, V), _nan(dev, B, V)
            L.call("umpr_control_gate_fwd", sn.sa, P_[14], P_[15], h[0].vp, h[0].fin, B, S_ui, V, senti, vs, ppos, pneg, st())
            res = [h[1].fin, h[2].fin, ppos, pneg]
            if need_grad:
                G = [_nan(dev, *s) for s in gshapes]
                d_sa, d_vp, d_cout = _nan(dev, B, S_ui, D), _nan(dev, B, S_ui, V), _nan(dev, B, V)
                dX_ui, dX_p = _nan(dev, Nui, L_ui, D), _nan(dev, 2 * N, Lm, D)
                w, wb = _ws(L, dev, "umpr_control_gate_bwd_ws_bytes", B)
                L.call("umpr_control_gate_bwd", sn.sa, P_[14], h[0].vp, h[0].fin, senti, vs, ups[2], ups[3], B, S_ui, V, d_sa, d_vp, d_cout,
                       G[14], G[15], w, wb, st())
                w, wb = _ws(L, dev, "umpr_snet_bwd_ws_bytes", B, S_ui, L_ui)
                L.call("umpr_snet_bwd", g_ui, P_[12], P_[13], sn.U, sn.P, sn.wsum, sn.sa, torch.zeros(B, D, device=dev), D, d_sa, B, S_ui, L_ui, V,
                       dX_ui, G[12], G[13], None, w, wb, st())
                dX = (dX_ui, dX_p[:N], dX_p[N:])
                dfin, dvp = (d_cout, ups[0], ups[1]), (d_vp, None, None)
                for k in range(3):
                    w, wb = _ws(L, dev, "umpr_cnet_head_bwd_ws_bytes", B, ss[k], ll[k], KC, KS, V)
                    L.call("umpr_cnet_head_bwd", X[k], P_[8], P_[10], h[k].cmax, h[k].argl, h[k].sp, h[k].vp, dfin[k], dvp[k], B, ss[k], ll[k], KC,
                           KS, V, dX[k], 1 if k == 0 else 0, 0 if k == 0 else 1, G[8], G[9], G[10], G[11], w, wb, st())
                dxp, dxu = _nan(dev, 2 * N * Lm, E), _nan(dev, Nui * L_ui, E)
                w, wb = _ws(L, dev, "umpr_embed_gru_bidir_ws_bytes", Nui, L_ui, E)
                L.call("umpr_embed_gru_bidir_bwd_dx", q.ids_ui, q.emb, E, P_[1], P_[5], q.lens_ui, q.ord_ui, dui, Nui, L_ui, dX_ui, g_ui, s_ui,
                       *G[:8], 0, P_[0], P_[4], dxu, 0, w, wb, st())
                w, wb = _ws(L, dev, "umpr_embed_gru_bidir_ws_bytes", 2 * N, Lm, E)
                L.call("umpr_embed_gru_bidir_bwd_dx", q.ids_pair, q.emb, E, P_[1], P_[5], q.lens, q.order, dpair, 2 * N, Lm, dX_p, g_p, s_p,
                       *G[:8], 1, P_[0], P_[4], dxp, 0, w, wb, st())
                res += G + [dxp, dxu]
        finally:
            TLS.gemm_b16 = False
        torch.cuda.synchronize()
        return res

    for kind in ("order", "identity", "random"):
        for masked in (False, True):
            a, b = fused(kind, masked), staged(kind, masked)
            assert len(a) == len(b)
            for k, (x_, y_) in enumerate(zip(a, b)):
                assert not bool(torch.isnan(x_).any()), (kind, masked, k)
                assert torch.equal(_bits(x_), _bits(y_)), (kind, masked, k)
            if kind == "order" and not masked:
                for k, (x_, y_) in enumerate(zip(a, fused(kind, False, ex=False))):
                    assert torch.equal(_bits(x_), _bits(y_)), ("existing entry", k)
    # one mask without the other: refused, nothing written
    arena = _nan(dev, na + 64)
    ws, wsb = _ws(L, dev, "umpr_control_net_ws_bytes", *dims, E, KC, KS, V)
    outs = [_nan(dev, B, V) for _ in range(4)]
    conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in
            (q.ids_ui, q.ids_pair, q.emb, E, pp, q.lens_ui, q.ord_ui, q.ord_ui, q.lens, q.order, q.order, *dims, KC, KS, V, thr, b16, need_grad,
             arena, *outs, ws, wsb, q.valid_ui, None, st())]
    assert L.fn["umpr_control_net_fwd_ex"](*conv) != 0 and "go together" in L.last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(arena).all()) and bool(torch.isnan(ws).all()) and all(bool(torch.isnan(o).all()) for o in outs)


# ================================================================================================================== the model
def _cfg(**kw):
    from umpr_amd.config import Config
    cfg = Config(argv=[])
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


_PARAMS = {}


def _params(seed, review_net_only=False):
    """the text-path, visual-head and fusion parameters the CPU test chose its batch with (make_param_state(with_vgg=False)), plus
    a VGG16 from another seeded state: the CPU conditions then speak about this very model"""
    from umpr_amd.synthetic import make_param_state
    key = (seed, review_net_only)
    if key not in _PARAMS:
        P = make_param_state(seed, 50, 900, 1, review_net_only, with_vgg=False, m_scale=0.05)
        if not review_net_only:
            if "vgg" not in _PARAMS:
                Pv = make_param_state(11, 50, 900, 1, False, m_scale=0.05)
                _PARAMS["vgg"] = {k: v for k, v in Pv.items() if ".vgg16." in k}
            P.update(_PARAMS["vgg"])
        _PARAMS[key] = P
    return _PARAMS[key]


def _model(dev, P, review_net_only=False, **kw):
    from umpr_amd.model import UMPR
    model = UMPR(_cfg(review_net_only=review_net_only, views=["unknown"], **kw), P["embedding.weight"].numpy())
    model.load_state_dict(P)
    return model.to(dev)


def _control_outputs(monkeypatch):
    """records what _ControlNetF returns (c_u, c_i, prefer_pos, prefer_neg) at every forward"""
    import umpr_amd.model as Mdl
    seen = []
    orig = Mdl._ControlNetF.apply

    def spy(*a):
        out = orig(*a)
        seen.append(torch.stack([t.detach().clone() for t in out]))
        return out
    monkeypatch.setattr(Mdl._ControlNetF, "apply", staticmethod(spy))
    return seen


LEGS = (("on", dict(mask_padding=True, mask_control=True, unsort_gru=True)),
        ("mask_padding", dict(mask_padding=False, mask_control=True, unsort_gru=True)),
        ("mask_control", dict(mask_padding=True, mask_control=False, unsort_gru=True)),
        ("unsort_gru", dict(mask_padding=True, mask_control=True, unsort_gru=False)))


def test_full_model_invariance(dev, monkeypatch):
    """Full model, V = 1, P = 1, eval mode, the batch of tests/test_control_mask_reference.py::test_invariance_batch.  All three
    options on: the sample alone and as row 0 of the batch agree within PARITY (prediction and the ControlNet's four outputs), and
    the batch prediction matches the float64 restatement (fed the HIP VGG16's own features) within PARITY.  One option off: the
    quantity the CPU test fixed for that leg - the prediction for mask_padding and unsort_gru, the ControlNet's four outputs for
    mask_control - differs by more than 10 x PARITY."""
    P = _params(700 + INV_SEED)
    alone, batch = K.invariance_batch(INV_SEED)
    seen = _control_outputs(monkeypatch)
    d = {}
    for leg, opts in LEGS:
        model = _model(dev, P, **opts).eval()
        del seen[:]
        with torch.no_grad():
            p1, p4 = model(*alone)[0].cpu(), model(*batch)[0].cpu()
            c1, c4 = seen[0][:, 0].cpu(), seen[1][:, 0].cpu()
            if leg == "on":
                feats = model.visual_net.vgg16[0](batch[6].reshape(-1, 3, 224, 224).to(dev).float()).double().cpu()
                P64 = {k: v.double() for k, v in P.items() if ".vgg16." not in k}
                b64 = tuple(t.double() if t.is_floating_point() else t for t in batch)
                ref = K.umpr_forward(P64, b64, review_net_only=False, vgg_fn=lambda x: feats, **opts)[0]
                err = float((p4.double() - ref).abs().max())
                print(f"batch prediction against the float64 restatement: {err:.3e}")
                assert err < PARITY
        d[leg] = (abs(float(p1[0]) - float(p4[0])), float((c1 - c4).abs().max()))
    print(d)
    log(f"full model invariance (|d prediction|, |d ControlNet outputs|): {d}")
    assert d["on"][0] <= PARITY and d["on"][1] <= PARITY, d
    assert d["mask_padding"][0] > 10 * PARITY, d
    assert d["mask_control"][1] > 10 * PARITY, d
    assert d["unsort_gru"][0] > 10 * PARITY, d


def test_umpr_r_invariance(dev):
    """UMPR-R with mask_padding + unsort_gru (mask_control is accepted and ignored): invariant within PARITY on the same batch - whose
    batch-mates have LONGER sentences, what mask_padding alone cannot be (its own test builds a batch without them) - and not with
    either option off."""
    P = _params(700 + INV_SEED, True)
    alone, batch = K.invariance_batch(INV_SEED, full=False)
    d = {}
    for leg, opts in (("on", dict(mask_padding=True, unsort_gru=True, mask_control=True)), ("mask_padding", dict(unsort_gru=True)),
                      ("unsort_gru", dict(mask_padding=True))):
        model = _model(dev, P, True, **opts).eval()
        with torch.no_grad():
            p1, p4 = model(*alone)[0].cpu(), model(*batch)[0].cpu()
            ref = K.umpr_forward({k: v.double() for k, v in P.items()}, batch, review_net_only=True,
                                 mask_padding=opts.get("mask_padding", False), unsort_gru=opts.get("unsort_gru", False))[0]
        assert float((p4.double() - ref).abs().max()) < PARITY, leg
        d[leg] = abs(float(p1[0]) - float(p4[0]))
    print(d)
    log(f"UMPR-R invariance |d prediction|: {d}")
    assert d["on"] <= PARITY, d
    assert d["mask_padding"] > 10 * PARITY and d["unsort_gru"] > 10 * PARITY, d


def test_training_step_against_the_restatement(dev):
    """One full-model step (eval mode, so that no dropout draws) on a ragged synthetic batch with padded sentences, all three options
    on, against the float64 restatement fed the HIP VGG16's features: predictions and loss 1e-4, every text-path gradient 2e-3 of
    its maximum (the tolerances of tests/test_gpu_e2e.py), no NaN in any gradient."""
    from umpr_amd.synthetic import make_batch
    P = _params(311)
    batch = make_batch(312, 4, 900, 1, max_sent_count=6, min_sent_count=2, max_ui_sent_count=4, max_sent_length=11)
    vu, _ = MA.batch_valid(batch)
    assert not bool(vu.view(4, -1, batch[0].shape[2]).any(-1).all()), "the batch has no padded sentence"
    opts = dict(mask_padding=True, mask_control=True, unsort_gru=True)
    model = _model(dev, P, **opts).eval()
    pred, loss = model(*batch)
    loss.backward()
    with torch.no_grad():
        feats = model.visual_net.vgg16[0](batch[6].reshape(-1, 3, 224, 224).to(dev).float()).double().cpu()
    P64 = {k: v.double().requires_grad_(k != "embedding.weight") for k, v in P.items() if ".vgg16." not in k}
    b64 = tuple(t.double() if t.is_floating_point() else t for t in batch)
    keep = {}
    rp, rl = K.umpr_forward(P64, b64, review_net_only=False, vgg_fn=lambda x: feats, keep=keep, **opts)
    rl.backward()
    assert float(keep["c_u"].abs().max()) > 0 and float((keep["prefer_pos"] + keep["prefer_neg"]).abs().max()) > 0
    dp, dl = float((pred.detach().cpu().double() - rp.detach()).abs().max()), abs(float(loss.detach()) - float(rl.detach()))
    print(f"|dpred| {dp:.3e} |dloss| {dl:.3e}")
    assert dp < 1e-4 and dl < 1e-4
    checked = 0
    for k, p in model.named_parameters():
        if p.grad is not None:
            assert bool(torch.isfinite(p.grad).all()), k
        if p.requires_grad and (k.startswith("review_net.") or k.startswith("control_net.")):
            ref = P64[k].grad
            err = float((p.grad.cpu().double() - ref).abs().max())
            print(f"{k}: {err:.3e} of {float(ref.abs().max()):.3e}")
            assert err <= 2e-3 * float(ref.abs().max()) + 1e-6, (k, err, float(ref.abs().max()))
            checked += 1
    assert checked == 31, checked


def _ragged_batches(n, review_net_only, B=4):
    from umpr_amd.synthetic import make_batch
    batches = [make_batch(40 + k, B, 900, 1, review_net_only=review_net_only, full_pad=True, max_sent_count=5, max_ui_sent_count=3,
                          max_sent_length=9) for k in range(n)]
    gen = torch.Generator().manual_seed(78)
    for b in batches:
        for lens in (b[3], b[4]) if review_net_only else (b[3], b[4], b[5]):
            lens[:, -2:] = torch.randint(1, 9, lens[:, -2:].shape, generator=gen)
    return batches


def _run_steps(model, batches, graphed):
    from umpr_amd.graphs import GraphedTrainStep
    from umpr_amd.optim import FusedAdam
    from umpr_amd.train import train_step
    opt = FusedAdam(model, 1e-3, 1e-3)
    step = GraphedTrainStep(model, opt, batches[0]) if graphed else (lambda b: train_step(model, opt, b))
    losses = [float(step(b)[1].detach()) for b in batches]
    torch.cuda.synchronize()
    return losses, {k: v.detach().clone() for k, v in model.state_dict().items()}


def test_graphed_umpr_r_step_with_unsort_gru_equals_eager(dev):
    """GraphedTrainStep captures the UMPR-R step only (umpr_amd/graphs.py asserts review_net_only: the full model cannot be captured
    today, so mask_control has no captured form to test).  With unsort_gru + mask_padding the identity rows are a cached static
    tensor: losses and every parameter after two steps are bit-identical to eager, and differ from the options off."""
    P = _params(21, True)
    batches = _ragged_batches(2, True)
    res = {g: _run_steps(_model(dev, P, True, unsort_gru=True, mask_padding=True), batches, g) for g in (False, True)}
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    for k in res[False][1]:
        assert torch.equal(res[False][1][k], res[True][1][k]), k
    assert _run_steps(_model(dev, P, True, mask_padding=True), batches, False)[0] != res[False][0], "unsort_gru changes nothing"


def test_checkpoint_records_and_refuses(dev, tmp_path):
    """both settings round-trip; each mismatch is refused by the option's name before anything is loaded; a checkpoint from before
    the options counts as False"""
    from umpr_amd.checkpoint import load_checkpoint, save_checkpoint
    P = _params(21, True)
    path = str(tmp_path / "ck.pt")
    for mc, ug in ((True, False), (False, True), (True, True)):
        save_checkpoint(path, _model(dev, P, True, mask_control=mc, unsort_gru=ug))
        ck = torch.load(path, weights_only=True)
        assert ck["mask_control"] is mc and ck["unsort_gru"] is ug
        load_checkpoint(path, _model(dev, P, True, mask_control=mc, unsort_gru=ug))
        for name, other in (("mask_control", dict(mask_control=not mc, unsort_gru=ug)), ("unsort_gru", dict(mask_control=mc, unsort_gru=not ug))):
            fresh = _model(dev, P, True, **other)
            with torch.no_grad():
                fresh.linear_fusion[0].bias.fill_(7.0)
            with pytest.raises(ValueError, match=f"--{name}"):
                load_checkpoint(path, fresh)
            assert float(fresh.linear_fusion[0].bias[0]) == 7.0, "the refused load wrote into the model"
    old = {k: v for k, v in ck.items() if k not in ("mask_control", "unsort_gru")}
    torch.save(old, path)
    load_checkpoint(path, _model(dev, P, True))
    with pytest.raises(ValueError, match="--unsort_gru"):
        load_checkpoint(path, _model(dev, P, True, unsort_gru=True))


def test_options_off_are_the_model_without_the_attributes(dev):
    """both options False against a model whose two attributes were removed (a model from before them): prediction, loss and every
    gradient of one full-model training step are bit-identical"""
    P = _params(311)
    batch = _ragged_batches(1, False)[0]
    res = []
    for bare in (False, True):
        model = _model(dev, P, mask_control=False, unsort_gru=False)
        if bare:
            del model.mask_control, model.unsort_gru
            assert not hasattr(model, "mask_control") and not hasattr(model, "unsort_gru")
        model.eval()
        pred, loss = model(*batch)
        loss.backward()
        torch.cuda.synchronize()
        res.append((pred.detach().clone(), loss.detach().clone(), {k: p.grad.clone() for k, p in model.named_parameters() if p.grad is not None}))
    assert torch.equal(_bits(res[0][0]), _bits(res[1][0])) and torch.equal(_bits(res[0][1]), _bits(res[1][1]))
    assert res[0][2].keys() == res[1][2].keys() and len(res[0][2]) > 40
    for k in res[0][2]:
        assert torch.equal(res[0][2][k], res[1][2][k]), k
