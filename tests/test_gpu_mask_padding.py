"""`--mask_padding True` on the GPU: umpr_token_mask, umpr_coattention_fwd_masked (+ the unchanged umpr_coattention_bwd),
umpr_snet_fwd_masked (+ the unchanged umpr_snet_bwd), umpr_review_net_fwd_masked and the model option.

The yardsticks are the merged ones.  A masked co-attention case is compacted per sample - the valid rows of Gu, Gi and T gathered,
the saved indices mapped to the compacted ones - and then goes through check_decisions, backward64 and gate of
tests/coattn_decisions.py at its K, unchanged; the S-Net goes through the same gate against the float64 restatement of
tests/masked_attention_reference.py.  What the mask adds is checked exactly: -1 / +0.0 at undefined positions, +0.0 gradients at
masked rows, all-valid masks giving the bits of the unmasked entry points, no NaN from empty sides.  Every call runs on NaN-filled
outputs and a NaN-filled workspace (for the fused entry: a NaN-filled arena too - what UMPR_POISON_WS=1 does inside the library, done
here by the caller so that no child process is needed), so a read through a -1 index or of a never-written partial shows up.
"""
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import coattn_decisions as C
import masked_attention_reference as MA
from test_cabi_sizes import SNET as CABI_SNET
from test_gpu_parity import LOG as PARITY_LOG
from test_gpu_parity import L, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "mask_padding.log")
D, AT = C.D, 64
BAND = 64            # guard band, in elements, on either side of every output the masked kernels write


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def _nan(dev, *shape):
    return torch.full(shape, float("nan"), device=dev)


def _ws(L, dev, name, *dims):
    wsb = L.size(name, *dims)
    return _nan(dev, wsb // 4 + 64), wsb


class Banded:
    """A buffer of `shape` with BAND elements of `fill` in front of it and behind it"""

    def __init__(self, dev, shape, dtype=torch.float32, fill=float("nan")):
        n = int(np.prod(shape))
        self.fill, self.n = fill, n
        self.whole = torch.full((n + 2 * BAND,), fill, dtype=dtype, device=dev)
        self.t = self.whole[BAND:BAND + n].view(*shape)

    def intact(self):
        b = torch.cat([self.whole[:BAND], self.whole[BAND + self.n:]])
        return bool(torch.isnan(b).all()) if self.fill != self.fill else bool((b == self.fill).all())


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ============================================================================================================ umpr_token_mask
@pytest.mark.parametrize("N,Lm", [(1, 1), (5, 7), (64, 20), (65, 64), (3, 256)])
def test_token_mask(L, dev, N, Lm):
    """Bit for bit the numpy rule.  Lengths run from -2 to L + 3 (0 and above L included), ids from 0 to 4 with pad_id 0 and 3
    (so the pad id stands inside the length), a byte-filled guard band on either side of the mask."""
    g = torch.Generator().manual_seed(100 * N + Lm)
    ids = torch.randint(0, 5, (N, Lm), generator=g)
    lengths = torch.randint(-2, Lm + 4, (N,), generator=g).to(torch.int32)
    lengths[0] = Lm
    if N > 2:
        lengths[1], lengths[2] = 0, Lm + 3
    for pad_id in (0, 3):
        out = Banded(dev, (N, Lm), torch.uint8, 0xAB)
        L.call("umpr_token_mask", ids.to(dev), lengths.to(dev), N, Lm, pad_id, out.t, st())
        torch.cuda.synchronize()
        want = MA.token_valid(ids.numpy(), lengths.numpy(), pad_id)
        assert np.array_equal(out.t.cpu().numpy(), want.astype(np.uint8)), (N, Lm, pad_id)
        assert out.intact()
        assert 0 < want.sum() < want.size or N == 1


def test_token_mask_refuses_bad_arguments(L, dev):
    x = torch.zeros(4, dtype=torch.int64, device=dev)
    for args, text in (((None, x, 1, 1, 0, x), "null pointer"), ((x, None, 1, 1, 0, x), "null pointer"),
                       ((x, x, 1, 1, 0, None), "null pointer"), ((x, x, 0, 1, 0, x), "bad shape"), ((x, x, 1, 0, 0, x), "bad shape")):
        conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
        assert L.fn["umpr_token_mask"](*conv, st()) != 0 and text in L.last_error()


# ========================================================================================================== the co-attention
def _sentence_mask(g, B, SL):
    """sentence-structured: chunks of up to 20 positions, each valid up to a random length (0 .. chunk), position 0 of a sample kept"""
    w = max(1, min(20, (SL + 2) // 3))
    v = torch.zeros(B, SL, dtype=torch.bool)
    for b in range(B):
        for s0 in range(0, SL, w):
            n = min(w, SL - s0)
            v[b, s0:s0 + int(torch.randint(0, n + 1, (1,), generator=g))] = True
        v[b, 0] = True
    return v


def _only(B, SL, pos):
    v = torch.zeros(B, SL, dtype=torch.bool)
    v[:, pos] = True
    return v


def _masks(pattern, B, SL):
    g = torch.Generator().manual_seed(7 * B + SL)
    full = torch.ones(B, SL, dtype=torch.bool)
    if pattern == "all_valid":
        return full, full.clone()
    if pattern == "ragged":
        return _sentence_mask(g, B, SL), _sentence_mask(g, B, SL)
    if pattern == "only_63":
        return _only(B, SL, 63), _only(B, SL, 63)
    if pattern == "only_64":
        return _only(B, SL, 64), _only(B, SL, 64)
    if pattern == "tile_masked_u":          # the first 64-tile of the user side masked, the item side full
        vu = full.clone()
        vu[:, :64] = False
        return vu, full
    if pattern == "tile_masked_i":          # the last (partial or whole) 64-tile of the item side masked, the user side full
        vi = full.clone()
        vi[:, (SL - 1) // 64 * 64:] = False
        return full, vi
    if pattern == "single":                 # one valid position per side and sample
        vu, vi = torch.zeros(B, SL, dtype=torch.bool), torch.zeros(B, SL, dtype=torch.bool)
        for b in range(B):
            vu[b, int(torch.randint(0, SL, (1,), generator=g))] = True
            vi[b, int(torch.randint(0, SL, (1,), generator=g))] = True
        return vu, vi
    if pattern == "empty_user_sample":      # the last sample of the batch has no valid user position, the others are ragged
        vu, vi = _sentence_mask(g, B, SL), _sentence_mask(g, B, SL)
        vu[B - 1] = False
        return vu, vi
    raise KeyError(pattern)


def _coattn_cases():
    out = []
    for B, SL in C.SHAPES:
        pats = ["all_valid", "ragged", "single", "empty_user_sample"]
        if SL >= 64:
            pats.append("only_63")
        if SL >= 65:
            pats += ["only_64", "tile_masked_u", "tile_masked_i"]
        out += [(B, SL, p) for p in pats]
    return out


def _fwd(L, dev, x, entry, vu=None, vi=None):
    """umpr_coattention_fwd_masked (vu given) or the unmasked entry on NaN-filled, banded outputs and a NaN-filled workspace"""
    B, SL, _ = x["Gu"].shape
    d = {k: x[k].to(dev).contiguous() for k in ("Gu", "Gi", "M")}
    o = SimpleNamespace(**d)
    o.band = {k: Banded(dev, (B, SL)) for k in ("soft_u", "soft_i", "colmax", "rowmax")}
    o.band.update({k: Banded(dev, (B, SL), torch.int32, -7) for k in ("argcol", "argrow")})
    o.band["T"] = Banded(dev, (B, SL, D))
    for k, b in o.band.items():
        setattr(o, k, b.t)
    o.rep_u, o.rep_i = _nan(dev, B, 2 * D), _nan(dev, B, 2 * D)
    ws, wsb = _ws(L, dev, "umpr_coattention_fwd_ws_bytes", B, SL)
    head = (o.Gu, o.Gi, o.M, B, SL, o.T, o.soft_u, o.soft_i, o.rep_u, 2 * D, o.rep_i.data_ptr() + D * 4, 2 * D, o.colmax, o.argcol,
            o.rowmax, o.argrow)
    if vu is None:
        L.call("umpr_coattention_fwd_bf16" if entry == "bf16" else "umpr_coattention_fwd", *head, ws, wsb, st())
    else:
        L.call("umpr_coattention_fwd_masked", *head, vu.to(dev).to(torch.uint8).contiguous(), vi.to(dev).to(torch.uint8).contiguous(),
               1 if entry == "bf16" else 0, ws, wsb, st())
    torch.cuda.synchronize()
    return o


def _bwd(L, dev, o, x, with_soft=True, prefill=None):
    """the unchanged umpr_coattention_bwd on the saved tensors of a masked forward (as tests/test_gpu_coattn.py calls it)"""
    B, SL, _ = x["Gu"].shape
    du, di = _nan(dev, B, 2 * D), _nan(dev, B, 2 * D)
    du[:, :D] = x["d_atte_u"].to(dev)
    di[:, D:] = x["d_atte_i"].to(dev)
    dsu = x["d_soft_u"].to(dev).contiguous() if with_soft else None
    dsi = x["d_soft_i"].to(dev).contiguous() if with_soft else None
    dGu = prefill[0].to(dev).contiguous() if prefill else _nan(dev, B, SL, D)
    dGi = prefill[1].to(dev).contiguous() if prefill else _nan(dev, B, SL, D)
    dM = _nan(dev, D, D)
    ws, wsb = _ws(L, dev, "umpr_coattention_bwd_ws_bytes", B, SL)
    L.call("umpr_coattention_bwd", o.Gu, o.Gi, o.M, o.T, o.soft_u, o.soft_i, o.colmax, o.argcol, o.rowmax, o.argrow, du, 2 * D,
           di.data_ptr() + D * 4, 2 * D, dsu, dsi, B, SL, dGu, dGi, dM, 1 if prefill else 0, ws, wsb, st())
    torch.cuda.synchronize()
    return dGu.cpu(), dGi.cpu(), dM.cpu()


def check_conventions(vu, vi, h):
    """h: CPU tensors soft_u, soft_i, colmax, rowmax, argcol, argrow.  Exactly -1 / +0.0 / +0.0 at undefined positions, an index
    of a VALID partner and a non-zero softmax weight elsewhere, no NaN.  Returns (defined_u, defined_i)."""
    def_u, def_i = vu & vi.any(-1, keepdim=True), vi & vu.any(-1, keepdim=True)
    for name, d, arg, mx, soft, partner in (("col", def_u, h.argcol, h.colmax, h.soft_u, vi), ("row", def_i, h.argrow, h.rowmax, h.soft_i, vu)):
        assert not bool(torch.isnan(mx).any()) and not bool(torch.isnan(soft).any()), name
        assert bool((arg[~d] == -1).all()), (name, arg[~d][:8])
        assert bool((_bits(mx)[~d] == 0).all()) and bool((_bits(soft)[~d] == 0).all()), name       # +0.0, not -0.0
        a = arg.long()
        assert bool(((a[d] >= 0) & (a[d] < vu.shape[1])).all()), name
        assert bool(partner.gather(1, a.clamp(min=0))[d].all()), f"{name}: a masked position is somebody's argmax partner"
        assert bool((soft[d] > 0).all()), name
        s = soft.double().sum(-1)
        assert bool(((s - d.any(-1).double()).abs() <= 1e-5).all()), (name, s)
    return def_u, def_i


def compacted(x, vu, vi, h, entry, b):
    """Sample b of a masked case as the unmasked problem on its valid rows: what tests/coattn_decisions.py needs, or None when a
    side is empty.  check_decisions wants a square score matrix, so the shorter side is filled up with copies of its first valid
    row (appended: a copy is never a first maximum, and its own saved entry is that of the original) - for the decisions only;
    backward64 runs on the rectangular problem as it stands."""
    ku, ki = vu[b].nonzero().squeeze(-1), vi[b].nonzero().squeeze(-1)
    nu, ni = len(ku), len(ki)
    if nu == 0 or ni == 0:
        return None
    inv_u, inv_i = torch.full((vu.shape[1],), -1, dtype=torch.long), torch.full((vu.shape[1],), -1, dtype=torch.long)
    inv_u[ku], inv_i[ki] = torch.arange(nu), torch.arange(ni)
    c = SimpleNamespace(ku=ku, ki=ki)
    c.Gu, c.Gi, c.M = x["Gu"][b][ku].unsqueeze(0), x["Gi"][b][ki].unsqueeze(0), x["M"]
    c.argcol, c.argrow = inv_i[h.argcol[b][ku].long()].unsqueeze(0), inv_u[h.argrow[b][ki].long()].unsqueeze(0)
    assert bool((c.argcol >= 0).all()) and bool((c.argrow >= 0).all()), "a saved index names a masked position"
    c.colmax, c.rowmax = h.colmax[b][ku].unsqueeze(0), h.rowmax[b][ki].unsqueeze(0)
    T_hip = h.T[b][ki].unsqueeze(0)
    if entry == "fp32":
        T64 = c.Gi.double() @ c.M.double()
        c.T_scores, c.Gu_scores, c.T_route, c.T32 = T64, c.Gu, T64, c.Gi @ c.M
        c.A32 = torch.tanh(c.T32 @ c.Gu.transpose(-1, -2))
    else:
        c.T_scores, c.Gu_scores, c.T_route, c.T32 = C.bf16_round(T_hip), C.bf16_round(c.Gu), T_hip.double(), T_hip
        c.A32 = torch.tanh(c.T_scores @ c.Gu_scores.transpose(-1, -2))
    c.A64 = C.scores64(c.T_scores, c.Gu_scores)
    # the square completion for check_decisions
    n = max(nu, ni)
    pu, pi = torch.cat([torch.arange(nu), torch.zeros(n - nu, dtype=torch.long)]), torch.cat([torch.arange(ni), torch.zeros(n - ni, dtype=torch.long)])
    c.square = (C.scores64(c.T_scores[:, pi], c.Gu_scores[:, pu]), c.T_scores[:, pi], c.Gu_scores[:, pu], c.argcol[:, pu], c.colmax[:, pu],
                c.argrow[:, pi], c.rowmax[:, pi])
    return c


def check_forward_and_reference(x, vu, vi, h, entry, tag):
    """Conventions, decisions and forward values of one masked case from CPU copies of the HIP outputs; returns the float64
    reference and float32 yardstick of the backward (plain and without d_soft), scattered to full size, with the masks."""
    B, SL, _ = x["Gu"].shape
    def_u, def_i = check_conventions(vu, vi, h)
    assert not bool(torch.isnan(h.atte_u).any()) and not bool(torch.isnan(h.atte_i).any()) and not bool(torch.isnan(h.T).any())
    z = lambda dt: [torch.zeros(B, SL, D, dtype=dt), torch.zeros(B, SL, D, dtype=dt), torch.zeros(D, D, dtype=dt)]
    ref = {k: z(torch.float64) for k in ("soft", "nosoft")}
    ref32 = {k: z(torch.float32) for k in ("soft", "nosoft")}
    for b in range(B):
        c = compacted(x, vu, vi, h, entry, b)
        if c is None:
            assert bool((_bits(h.atte_u[b]) == 0).all()) and bool((_bits(h.atte_i[b]) == 0).all()), "atte of an empty side is not +0.0"
            continue
        fails, stats = C.check_decisions(*c.square)
        log(f"{tag} b{b} ({len(c.ku)} x {len(c.ki)} valid) decisions: " + " ".join(f"{s}: {v[0]:.3e} / {v[1]:.3e}" for s, v in stats.items()))
        assert not fails, (tag, b, fails)
        _, _, su, si, au, ai = C.forward64(c.Gu, c.Gi, c.A64, c.argcol, c.argrow)
        for name, got, want in (("soft_u", h.soft_u[b][c.ku], su[0]), ("soft_i", h.soft_i[b][c.ki], si[0]), ("atte_u", h.atte_u[b], au[0]),
                                ("atte_i", h.atte_i[b], ai[0])):
            assert float((got.double() - want).abs().max()) <= 2e-6, (tag, b, name)
        up = (x["d_atte_u"][b:b + 1], x["d_atte_i"][b:b + 1])
        soft = (x["d_soft_u"][b][c.ku].unsqueeze(0), x["d_soft_i"][b][c.ki].unsqueeze(0))
        for key, extra in (("soft", soft), ("nosoft", ())):
            r = C.backward64(c.Gu, c.Gi, c.M, c.T_route, c.A64, c.argcol, c.argrow, *up, *extra)
            r32 = C.backward64(c.Gu, c.Gi, c.M, c.T32, c.A32, c.argcol, c.argrow, *up, *extra, dtype=torch.float32)
            for full, part in ((ref[key], r), (ref32[key], r32)):
                full[0][b, c.ku] = part[0][0]
                full[1][b, c.ki] = part[1][0]
                full[2] += part[2]
    return ref, ref32, def_u, def_i


def _assert_gate(tag, got, ref, ref32):
    ok, rows = C.gate(got, ref, ref32, log=log, tag=tag)
    assert ok, [(r["name"], r["d_max"], r["d_l2"], r["r_max"], r["r_l2"], r["ratio"]) for r in rows if not r["ok"]]


def _host(o):
    return SimpleNamespace(soft_u=o.soft_u.cpu(), soft_i=o.soft_i.cpu(), colmax=o.colmax.cpu(), rowmax=o.rowmax.cpu(),
                           argcol=o.argcol.cpu(), argrow=o.argrow.cpu(), T=o.T.cpu(), atte_u=o.rep_u[:, :D].cpu(), atte_i=o.rep_i[:, D:].cpu())


@pytest.mark.parametrize("entry", ["fp32", "bf16"])
@pytest.mark.parametrize("B,SL,pattern", _coattn_cases())
def test_coattention_masked(L, dev, B, SL, pattern, entry):
    """One mask pattern at one shape of tests/coattn_decisions.py::SHAPES: conventions, guard bands, decisions and forward values
    by compaction, then the unchanged backward in its plain, d_soft = NULL and accumulate variants - valid rows through C.gate
    against the float64 backward of the compacted problems, masked rows exactly +0.0 (bit-equal to the prefill under accumulate).
    d_soft_* is random and non-zero at masked positions.  all_valid is in addition bit-equal to the unmasked entry point."""
    x = C.make_inputs(B, SL)
    vu, vi = _masks(pattern, B, SL)
    tag = f"masked B{B} SL{SL} {pattern} {entry}"
    o = _fwd(L, dev, x, entry, vu, vi)
    assert all(b.intact() for b in o.band.values()), [k for k, b in o.band.items() if not b.intact()]
    assert bool(torch.isnan(o.rep_u[:, D:]).all()) and bool(torch.isnan(o.rep_i[:, :D]).all()), "atte written outside its half"
    h = _host(o)
    if pattern == "all_valid":
        p = _host(_fwd(L, dev, x, entry))
        for k in vars(h):
            assert torch.equal(_bits(getattr(h, k)), _bits(getattr(p, k))), f"{k}: an all-valid mask changes the bits"
    ref, ref32, def_u, def_i = check_forward_and_reference(x, vu, vi, h, entry, tag)
    assert bool((x["d_soft_u"][~def_u] != 0).all()) and bool((x["d_soft_i"][~def_i] != 0).all())
    got = _bwd(L, dev, o, x)
    _assert_gate(tag + " plain", got, ref["soft"], ref32["soft"])
    assert bool((_bits(got[0])[~def_u] == 0).all()) and bool((_bits(got[1])[~def_i] == 0).all()), "a masked row's gradient is not +0.0"
    got = _bwd(L, dev, o, x, with_soft=False)
    _assert_gate(tag + " d_soft NULL", got, ref["nosoft"], ref32["nosoft"])
    assert bool((_bits(got[0])[~def_u] == 0).all()) and bool((_bits(got[1])[~def_i] == 0).all())
    g = torch.Generator().manual_seed(B + SL)
    pre = (torch.randn(B, SL, D, generator=g), torch.randn(B, SL, D, generator=g))
    got = _bwd(L, dev, o, x, prefill=pre)
    add = lambda r, dt: (r[0] + pre[0].to(dt), r[1] + pre[1].to(dt), r[2])
    _assert_gate(tag + " accumulate", got, add(ref["soft"], torch.float64), add(ref32["soft"], torch.float32))
    assert torch.equal(_bits(got[0])[~def_u], _bits(pre[0])[~def_u]) and torch.equal(_bits(got[1])[~def_i], _bits(pre[1])[~def_i])


def test_coattention_masked_refuses_a_null_mask(L, dev):
    x = C.make_inputs(2, 3)
    o = _fwd(L, dev, x, "fp32")
    ws, wsb = _ws(L, dev, "umpr_coattention_fwd_ws_bytes", 2, 3)
    v = torch.ones(2, 3, dtype=torch.uint8, device=dev)
    for vu, vi in ((None, v), (v, None)):
        args = [o.Gu, o.Gi, o.M, 2, 3, o.T, o.soft_u, o.soft_i, o.rep_u, 2 * D, o.rep_i, 2 * D, o.colmax, o.argcol, o.rowmax, o.argrow, vu, vi,
                0, ws, wsb]
        conv = [a.data_ptr() if isinstance(a, torch.Tensor) else a for a in args]
        assert L.fn["umpr_coattention_fwd_masked"](*conv, st()) != 0 and "null validity mask" in L.last_error()


# ================================================================================================================== the S-Net
SNET_SHAPES = tuple(CABI_SNET) + tuple((5, 1, l) for l in (64, 65, 128, 129, 256))


def _snet_masks(pattern, B, S, Lm):
    g = torch.Generator().manual_seed(31 * B + 7 * S + Lm)
    if pattern == "all_valid":
        return torch.ones(B, S, Lm, dtype=torch.bool)
    if pattern == "first_token":
        v = torch.zeros(B, S, Lm, dtype=torch.bool)
        v[..., 0] = True
        return v
    lengths = torch.randint(1, Lm + 1, (B, S), generator=g)
    v = torch.arange(Lm).view(1, 1, Lm) < lengths.unsqueeze(-1)
    v &= torch.rand(B, S, Lm, generator=g) < 0.9              # a pad id inside the length now and then
    v[..., 0] = True
    if pattern == "empty_sentence":
        v.view(B * S, Lm)[(B * S) // 2] = False
    return v


def _snet_fwd(L, dev, x, valid=None):
    B, S, Lm, wl = x["dims"]
    o = SimpleNamespace(X=x["X"].to(dev).contiguous(), Ms=x["Ms"].to(dev).contiguous(), Ws=x["Ws"].to(dev).contiguous(),
                        word_soft=x["word_soft"].to(dev).contiguous(), U=_nan(dev, B * S, Lm, AT), senti_buf=_nan(dev, B, 2 * D))
    o.band = {"P": Banded(dev, (B * S, Lm)), "wsum": Banded(dev, (B, S)), "self_atte": Banded(dev, (B, S, D))}
    for k, b in o.band.items():
        setattr(o, k, b.t)
    head = (o.X, o.Ms, o.Ws, o.word_soft, wl, B, S, Lm, o.U, o.P, o.wsum, o.self_atte, o.senti_buf.data_ptr() + 4 * D, 2 * D)
    if valid is None:
        L.call("umpr_snet_fwd", *head, st())
    else:
        L.call("umpr_snet_fwd_masked", *head, valid.to(dev).to(torch.uint8).contiguous(), st())
    torch.cuda.synchronize()
    return o


@pytest.mark.parametrize("pattern", ["all_valid", "ragged", "first_token", "empty_sentence"])
@pytest.mark.parametrize("B,S,Lm", SNET_SHAPES)
def test_snet_masked(L, dev, B, S, Lm, pattern):
    """umpr_snet_fwd_masked and the unchanged umpr_snet_bwd in the form the ReviewNet calls them (wl = L, senti in the upper half of
    [B][256] rows).  all_valid: every output has the bits of umpr_snet_fwd.  Otherwise U, P, wsum, self_atte, senti and dX, dMs,
    dWs, d_word_soft go through C.gate (K = 4 x the float32 CPU evaluation's own distance, floored at 2^-22) against the float64
    restatement; P is exactly +0.0 at masked tokens, self_atte exactly 0 for a sentence without a valid token, and dX - the
    buffer umpr_snet_bwd returns, i.e. after the GEMM dPre Ms was added, whose dPre rows are zero there - exactly 0 at masked
    tokens."""
    import control_decisions as CD
    x = CD.make_snet_inputs(B, S, Lm, Lm)
    valid = _snet_masks(pattern, B, S, Lm)
    tag = f"snet masked B{B} S{S} L{Lm} {pattern}"
    o = _snet_fwd(L, dev, x, valid)
    assert all(b.intact() for b in o.band.values())
    senti = o.senti_buf.cpu()
    assert bool(torch.isnan(senti[:, :D]).all())
    if pattern == "all_valid":
        p = _snet_fwd(L, dev, x)
        for k in ("U", "P", "wsum", "self_atte", "senti_buf"):
            assert torch.equal(_bits(getattr(o, k)), _bits(getattr(p, k))), f"{k}: an all-valid mask changes the bits"
    Pm = o.P.cpu().view(B, S, Lm)
    assert bool((_bits(Pm)[~valid] == 0).all()), "P at a masked token is not +0.0"
    empty = ~valid.any(-1)
    assert bool((o.self_atte.cpu()[empty] == 0).all()) and not bool(torch.isnan(o.self_atte).any())
    Xs = x["X"].view(B, S, Lm, D)
    out = {dt: MA.snet_forward(Xs, x["Ms"], x["Ws"], x["word_soft"], valid, dt) for dt in (torch.float64, torch.float32)}
    pick = lambda f: (f["U"].reshape(B * S, Lm, AT), f["P"].reshape(B * S, Lm), f["wsum"], f["self_atte"], f["senti"])
    ok, rows = C.gate((o.U.cpu(), o.P.cpu(), o.wsum.cpu(), o.self_atte.cpu(), senti[:, D:]), pick(out[torch.float64]), pick(out[torch.float32]),
                      names=CD.SNET_OUT, K=C.K, log=log, tag=tag)
    assert ok, [(r["name"], r["ratio"]) for r in rows if not r["ok"]]
    ds = _nan(dev, B, 2 * D)
    ds[:, D:] = x["d_senti"].to(dev)
    dX, dMs, dWs, dws = _nan(dev, B * S, Lm, D), _nan(dev, AT, D), _nan(dev, AT), _nan(dev, B, S, Lm)
    ws, wsb = _ws(L, dev, "umpr_snet_bwd_ws_bytes", B, S, Lm)
    L.call("umpr_snet_bwd", o.X, o.Ms, o.Ws, o.U, o.P, o.wsum, o.self_atte, ds.data_ptr() + 4 * D, 2 * D, None, B, S, Lm, Lm, dX, dMs, dWs, dws,
           ws, wsb, st())
    torch.cuda.synchronize()
    g = {dt: MA.snet_backward64(Xs, x["Ms"], x["Ws"], x["word_soft"], valid, x["d_senti"], None, dt) for dt in (torch.float64, torch.float32)}
    shape = lambda t: (t[0].reshape(B * S, Lm, D), t[1], t[2], t[3])
    ok, rows = C.gate((dX.cpu(), dMs.cpu(), dWs.cpu(), dws.cpu()), shape(g[torch.float64]), shape(g[torch.float32]),
                      names=("dX", "dMs", "dWs", "d_word_soft"), K=C.K, log=log, tag=tag)
    assert ok, [(r["name"], r["ratio"]) for r in rows if not r["ok"]]
    assert bool((dX.cpu().view(B, S, Lm, D)[~valid] == 0).all()), "dX at a masked token is not 0"


# ==================================================================================================== umpr_review_net_fwd_masked
def _review_problem(dev, B, S, Lm, seed=3):
    from umpr_amd.model import UMPR
    from umpr_amd.synthetic import make_param_state
    E, vocab, N = 50, 300, B * S
    P = make_param_state(17, E, vocab, 1, True, m_scale=0.3)
    g = torch.Generator().manual_seed(seed + 100 * B + 10 * S + Lm)
    ids, lens = [], []
    for _ in range(2):
        n = torch.randint(1, Lm + 1, (N,), generator=g)
        n[0] = Lm
        t = torch.randint(0, vocab, (N, Lm), generator=g)             # id 0 = <PAD> turns up inside a length now and then
        t = t * (torch.arange(Lm).view(1, Lm) < n.view(N, 1))
        if N > 2:
            t[2], n[2] = 0, 1                                            # a padded sentence: length 1, id 0
        ids.append(t); lens.append(n)
    (lu, ou), (li, oi) = UMPR._host_perm(lens[0], dev), UMPR._host_perm(lens[1], dev)
    pre = "review_net."
    gp = pre + "r_net.gru.module."
    names = [gp + n + s for s in ("", "_reverse") for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    names += [pre + "r_net.M", pre + "s_net_u.Ms", pre + "s_net_u.Ws", pre + "s_net_i.Ms", pre + "s_net_i.Ws", pre + "linear_u.weight",
              pre + "linear_i.weight"]
    return SimpleNamespace(E=E, emb=P["embedding.weight"].to(dev).contiguous(), params=[P[n].to(dev).contiguous() for n in names],
                           ids_pair=torch.cat(ids).to(dev).contiguous(), lens=torch.cat([lu, li]).contiguous(),
                           order=torch.cat([ou, oi + N]).contiguous(), ids=ids, lens_cpu=lens)


@pytest.mark.parametrize("need_grad", [0, 1])
@pytest.mark.parametrize("b16", [0, 1])
@pytest.mark.parametrize("B,S,Lm", [(2, 1, 1), (3, 7, 9), (2, 5, 13)])
def test_fused_masked_entry_equals_the_masked_stages(L, dev, B, S, Lm, b16, need_grad):
    """umpr_review_net_fwd_masked on a NaN-filled arena and workspace against the chain it issues - umpr_embed_gru_bidir_fwd,
    umpr_coattention_fwd_masked, umpr_snet_fwd_masked twice, umpr_review_merge_fwd - with the mask of umpr_token_mask: torch.equal.
    b16 sets both b16_gemm and b16_scores (the stage calls run under umpr_set_gemm_bf16(1))."""
    from umpr_amd._lib import TLS
    q = _review_problem(dev, B, S, Lm)
    N, SL, E = B * S, S * Lm, q.E
    valid = torch.full((2 * N, Lm), 0xAB, dtype=torch.uint8, device=dev)
    L.call("umpr_token_mask", q.ids_pair, q.lens, 2 * N, Lm, 0, valid, st())
    want = np.concatenate([MA.token_valid(q.ids[k].numpy(), q.lens_cpu[k].numpy()) for k in (0, 1)])
    assert np.array_equal(valid.cpu().numpy(), want.astype(np.uint8))
    ptrs = torch.tensor([t.data_ptr() for t in q.params], dtype=torch.int64)
    arena = _nan(dev, L.size("umpr_review_net_arena_bytes", B, S, Lm) // 4 + 64)
    ws, wsb = _ws(L, dev, "umpr_review_net_ws_bytes", B, S, Lm, E)
    fused = _nan(dev, B, D)
    L.call("umpr_review_net_fwd_masked", q.ids_pair, q.emb, E, ptrs.data_ptr(), q.lens, q.order, B, S, Lm, b16, b16, need_grad, arena, fused,
           ws, wsb, valid, st())
    torch.cuda.synchronize()
    assert not bool(torch.isnan(fused).any())
    TLS.gemm_b16 = bool(b16)
    try:
        gru, saved = _nan(dev, 2 * N, Lm, D), _nan(dev, 2, 2 * N, Lm, 4, 64)
        w, wb = _ws(L, dev, "umpr_embed_gru_bidir_ws_bytes", 2 * N, Lm, E)
        L.call("umpr_embed_gru_bidir_fwd", q.ids_pair, q.emb, E, *q.params[:8], q.lens, q.order, q.order, 2 * N, Lm, gru, saved if need_grad else None,
               w, wb, st())
        gu, gi = gru[:N].view(B, SL, D), gru[N:].view(B, SL, D)
        vu, vi = valid[:N].view(B, SL), valid[N:].view(B, SL)
        T, su, si, cm, rm = _nan(dev, B, SL, D), _nan(dev, B, SL), _nan(dev, B, SL), _nan(dev, B, SL), _nan(dev, B, SL)
        ac, ar = torch.full((B, SL), -7, dtype=torch.int32, device=dev), torch.full((B, SL), -7, dtype=torch.int32, device=dev)
        ru, ri = _nan(dev, B, 2 * D), _nan(dev, B, 2 * D)
        w, wb = _ws(L, dev, "umpr_coattention_fwd_ws_bytes", B, SL)
        L.call("umpr_coattention_fwd_masked", gu, gi, q.params[8], B, SL, T, su, si, ru, 2 * D, ri, 2 * D, cm, ac, rm, ar, vu, vi, b16, w, wb, st())
        for X, Ms, Ws, soft, rep, v in ((gu, q.params[9], q.params[10], su, ru, vu), (gi, q.params[11], q.params[12], si, ri, vi)):
            L.call("umpr_snet_fwd_masked", X, Ms, Ws, soft, Lm, B, S, Lm, _nan(dev, N, Lm, AT), _nan(dev, N, Lm), _nan(dev, B, S), _nan(dev, B, S, D),
                   rep.data_ptr() + 4 * D, 2 * D, v, st())
        staged = _nan(dev, B, D)
        L.call("umpr_review_merge_fwd", ru, ri, q.params[13], q.params[14], B, staged, st())
    finally:
        TLS.gemm_b16 = False
    torch.cuda.synchronize()
    assert torch.equal(_bits(fused), _bits(staged))


# ================================================================================================================== the model
def _cfg(**kw):
    from umpr_amd.config import Config
    cfg = Config(argv=[])
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _model(dev, P, **kw):
    from umpr_amd.model import UMPR
    model = UMPR(_cfg(review_net_only=True, **kw), P["embedding.weight"].numpy())
    model.load_state_dict(P)
    return model.to(dev)


def test_padding_invariance(dev):
    """One sample alone (S = 4, L = 10), then as row 0 of a batch of 4 padded to S = 6, L = 13 (MA.invariance_batch(1): why its
    batch-mates are shorter sentences and the larger L is padding width is said there).  With the option on the two predictions agree
    within the parity bound 1e-4; with it off they differ by more than ten times that.  The references alone, chosen on
    the CPU (tests/test_masked_attention_reference.py): on 0.0 in float32 and in float64, off 1.50e-2 in both."""
    from umpr_amd.synthetic import make_param_state
    from test_masked_attention_reference import INVARIANCE_SEED, PARITY, invariance_differences
    P = make_param_state(21, 50, 900, 1, True, m_scale=0.05)
    alone, batch = MA.invariance_batch(INVARIANCE_SEED)
    ref_on, ref_off = invariance_differences(torch.float32)
    diff = {}
    for on in (True, False):
        model = _model(dev, P, mask_padding=on).eval()
        with torch.no_grad():
            p1, p4 = model(*alone)[0], model(*batch)[0]
        diff[on] = abs(float(p1[0]) - float(p4[0]))
        ref = MA.umpr_r_forward(P, batch, mask=on)[0]
        assert float((p4.cpu() - ref).abs().max()) < PARITY, on
    print(f"padding invariance: HIP on {diff[True]:.3e} off {diff[False]:.3e} | references on {ref_on:.3e} off {ref_off:.3e}")
    log(f"padding invariance: HIP on {diff[True]:.3e} off {diff[False]:.3e} | references on {ref_on:.3e} off {ref_off:.3e}")
    assert diff[True] <= PARITY, diff
    assert diff[False] > 10 * PARITY, diff


def test_training_step_against_the_restatement(dev):
    """UMPR-R with the option on, one step on a ragged synthetic batch, against the float64 restatement driven through the oracle's
    other stages (embedding, ImprovedRnn, merge, fusion, loss), at the tolerances tests/test_gpu_e2e.py uses for UMPR-R: predictions
    and loss 1e-4, every gradient 2e-3 of its maximum.  No gradient is NaN: the batch has padded sentences, i.e. sentences without a valid token."""
    from umpr_amd.synthetic import make_batch, make_param_state
    P = make_param_state(211, 50, 900, 1, True, m_scale=0.05)
    batch = make_batch(212, 5, 900, review_net_only=True, max_sent_count=7, min_sent_count=2, max_sent_length=11)
    vu, vi = MA.batch_valid(batch)
    assert not bool(vu.view(5, -1, batch[0].shape[2]).any(-1).all()), "the batch has no padded sentence"
    model = _model(dev, P, mask_padding=True).eval()
    pred, loss = model(*batch)
    loss.backward()
    P64 = {k: v.double().requires_grad_(k != "embedding.weight") for k, v in P.items()}
    b64 = tuple(t.double() if t.is_floating_point() else t for t in batch)
    rp, rl = MA.umpr_r_forward(P64, b64, mask=True)
    rl.backward()
    tol_out, tol_g = 1e-4, 2e-3
    print(f"|dpred| {float((pred.detach().cpu().double() - rp.detach()).abs().max()):.3e} |dloss| {abs(float(loss.detach()) - float(rl.detach())):.3e}")
    assert float((pred.detach().cpu().double() - rp.detach()).abs().max()) < tol_out
    assert abs(float(loss.detach()) - float(rl.detach())) < tol_out
    for k, p in model.named_parameters():
        if p.requires_grad:
            ref = P64[k].grad
            assert not bool(torch.isnan(p.grad).any()), k
            err = float((p.grad.cpu().double() - ref).abs().max())
            assert err <= tol_g * float(ref.abs().max()) + 1e-6, (k, err, float(ref.abs().max()))
    # the unmasked oracle is another function: the option is really on
    op, _ = MA.umpr_r_forward(P, batch, mask=False)
    assert float((op.detach() - rp.detach().float()).abs().max()) > 10 * tol_out


def _ragged_full_batches(n, B=6, vocab=900):
    """full-size batches (one geometry, as a captured step needs) whose lengths are ragged in the last sentences of either side"""
    from umpr_amd.synthetic import make_batch
    batches = [make_batch(30 + k, B, vocab, review_net_only=True, full_pad=True, max_sent_count=6, max_sent_length=9) for k in range(n)]
    gen = torch.Generator().manual_seed(77)
    for b in batches:
        for lens in (b[3], b[4]):
            lens[:, -3:] = torch.randint(1, 9, lens[:, -3:].shape, generator=gen)
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


def test_graphed_step_with_the_mask_equals_eager(dev):
    """GraphedTrainStep with the option on: the mask is computed on the device inside the capture, nothing new is static.  Losses and
    every parameter after two steps are bit-identical to the eager steps."""
    from umpr_amd.synthetic import make_param_state
    P = make_param_state(21, 50, 900, 1, True, m_scale=0.05)
    batches = _ragged_full_batches(2)
    res = {g: _run_steps(_model(dev, P, mask_padding=True), batches, g) for g in (False, True)}
    assert res[False][0] == res[True][0], (res[False][0], res[True][0])
    for k in res[False][1]:
        assert torch.equal(res[False][1][k], res[True][1][k]), k
    off = _run_steps(_model(dev, P), batches, False)
    assert off[0] != res[False][0], "the option changes nothing on a ragged batch"


def test_option_off_is_the_model_without_the_attribute(dev):
    """mask_padding=False against a model whose attribute was removed (what a model from before the option is): losses and parameters
    after two steps are bit-identical."""
    from umpr_amd.synthetic import make_param_state
    P = make_param_state(21, 50, 900, 1, True, m_scale=0.05)
    batches = _ragged_full_batches(2)
    off = _model(dev, P, mask_padding=False)
    bare = _model(dev, P)
    del bare.mask_padding
    assert not hasattr(bare, "mask_padding")
    a, b = _run_steps(off, batches, False), _run_steps(bare, batches, False)
    assert a[0] == b[0]
    for k in a[1]:
        assert torch.equal(a[1][k], b[1][k]), k
