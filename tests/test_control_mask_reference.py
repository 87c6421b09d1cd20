"""tests/control_mask_reference.py pinned on the CPU (no GPU): the definitions of `--mask_control True` and `--unsort_gru True`.

  * truncation identity: the masked C-Net head, control S-Net and gate on a padded sample equal the reference's own formulas
    (oracle/umpr_ref.py) on the same sample with every sentence cut to n_s and the undefined sentences removed - outputs and
    gradients, float64, 1e-12;
  * the own-states GRU equals the oracle's ImprovedRnn where its permutation is the identity and differs where it is not;
  * the invariance batch: with the three options on, a sample's float64 prediction is the same alone and as row 0 of a batch of 4
    whose other samples are larger on every review input; with exactly one option off it is not.
"""
import pytest
import torch
import torch.nn.functional as F

import control_decisions as C
import control_mask_reference as K
import masked_attention_reference as M
from oracle import umpr_ref as R

D = C.D
INV_SEED = 3        # the seed of the invariance batch the GPU tests share (test_invariance_batch holds its conditions)


def test_leading_run_ends_at_a_hole():
    v = torch.tensor([[1, 0, 1, 1], [1, 1, 1, 1], [0, 1, 1, 1], [1, 1, 0, 0], [0, 0, 0, 0]]).bool()
    assert K.leading_run(v).tolist() == [1, 4, 0, 2, 0]
    # token validity of what the loader produces has no hole: n_s is the number of valid tokens
    ids = torch.tensor([[5, 6, 7, 0, 0], [0, 0, 0, 0, 0], [4, 4, 4, 4, 4]])
    valid = torch.from_numpy(M.token_valid(ids.numpy(), torch.tensor([3, 1, 9]).numpy()))
    assert K.leading_run(valid).tolist() == [3, 0, 5] == valid.sum(-1).tolist()
    # a (valid, invalid, valid) sentence has n_s = 1: under an even KS it is undefined, under an odd one position 0 alone counts
    assert int(C.lout(K.leading_run(v)[0], 2)) == 0 and int(C.lout(K.leading_run(v)[0], 3)) == 1


def _stage_case(KS, seed=0):
    """X [B][S][L][128] float64 with per-sentence token counts: full, ragged, one token, padded (0 valid tokens: the GRU still ran
    one step, so row 0 of a padded sentence is NOT zero), a sample without any defined sentence."""
    B, S, L, V, KC = 3, 4, 7, 3, 12
    x = C.make_inputs(B, S, L, V, KS, KC, seed)
    ns = torch.tensor([[7, 3, 1, 0], [0, 0, 0, 0], [1, 2, 5, 0]])
    g = torch.Generator().manual_seed(40 + KS)
    X = 0.7 * torch.randn(B, S, L, D, generator=g, dtype=torch.float64)
    X = X * (torch.arange(L).view(1, 1, L, 1) < torch.clamp(ns, min=1).view(B, S, 1, 1))
    valid = torch.arange(L).view(1, 1, L) < ns.view(B, S, 1)
    pre = "control_net."
    P = {pre + "c_net.cnn.0.weight": x["Wc"], pre + "c_net.cnn.0.bias": x["bc"], pre + "c_net.linear.0.weight": x["Wl"],
         pre + "c_net.linear.0.bias": x["bl"], pre + "s_net.Ms": x["Ms"], pre + "s_net.Ws": x["Ws"].view(1, -1),
         pre + "ss_net.linear.0.weight": x["ssW"].view(1, -1), pre + "ss_net.linear.0.bias": x["ssb"]}
    P = {k: v.double().clone().requires_grad_(True) for k, v in P.items()}
    up = {k: torch.randn(B, V, generator=g, dtype=torch.float64) for k in ("pp", "pn", "final")}
    up["vp"] = torch.randn(B, S, V, generator=g, dtype=torch.float64)
    return X.requires_grad_(True), valid, ns, P, up, (B, S, L, V, KS, KC)


def _masked_stage(X, valid, P, dims):
    B, S, L, V, KS, KC = dims
    pre = "control_net."
    keep = {}
    vp = K.head(X.view(B * S, L, D), valid.view(B * S, L), P[pre + "c_net.cnn.0.weight"], P[pre + "c_net.cnn.0.bias"],
                P[pre + "c_net.linear.0.weight"], P[pre + "c_net.linear.0.bias"], C.THR32, keep)[0].view(B, S, V)
    final = (vp ** 2).sum(1)
    s, _ = M.s_net(X.view(B, S * L, D), vp, L, P, pre + "s_net.", valid.view(B, S * L))
    pp, pn, vs = K.gate(s, vp, final, P)
    return vp, final, pp, pn, vs, keep


def _truncated_stage(X, ns, P, dims):
    """the reference's formulas on each sample's defined sentences, each cut to n_s"""
    B, S, L, V, KS, KC = dims
    pre = "control_net."
    vp_all = torch.zeros(B, S, V, dtype=X.dtype)
    final, pp, pn, vs = ([torch.zeros(V, dtype=X.dtype) for _ in range(B)] for _ in range(4))
    for b in range(B):
        rows, sa, where = [], [], []
        for s in range(S):
            n = int(ns[b, s])
            if C.lout(n, KS) < 1:
                continue
            Xs = X[b, s, :n]
            out = F.relu(F.conv1d(Xs.t().unsqueeze(0), P[pre + "c_net.cnn.0.weight"], P[pre + "c_net.cnn.0.bias"], padding=(KS - 1) // 2))
            vp = torch.sigmoid(F.linear(out.max(dim=-1)[0], P[pre + "c_net.linear.0.weight"], P[pre + "c_net.linear.0.bias"]))
            vp = torch.where(vp < C.THR32, torch.zeros_like(vp), vp)                       # [1][V]
            rows.append(vp)
            sa.append(R.s_net(Xs.unsqueeze(0), vp, n, P, pre + "s_net.")[0])               # [1][1][128]
            where.append(s)
        if rows:
            view_p = torch.cat(rows).unsqueeze(0)                                           # [1][Sd][V]
            final[b] = (view_p ** 2).sum(-2)[0]
            p_, n_, v_ = K.gate(torch.cat(sa, 1), view_p, final[b].unsqueeze(0), P)
            pp[b], pn[b], vs[b] = p_[0], n_[0], v_[0]
            idx = torch.zeros(S, len(where), dtype=X.dtype)
            idx[where, range(len(where))] = 1
            vp_all = vp_all + F.pad((idx @ view_p[0]).unsqueeze(0), (0, 0, 0, 0, b, B - 1 - b))
    return vp_all, torch.stack(final), torch.stack(pp), torch.stack(pn), torch.stack(vs)


@pytest.mark.parametrize("KS", [1, 2, 3, 4])
def test_truncation_identity(KS):
    """Outputs and gradients of the masked stage chain against the truncated reference within 1e-12; the -1 / +0.0 conventions;
    exact zero gradients.  KS = 2 and 4 make the one-token sentences undefined.  A 'same' convolution reads KS - 1 - pad rows
    past its last eligible position (zero rows, the truncated form's own zero padding): those rows of X may receive a gradient,
    which the GRU backward drops (no dout at t >= length reaches its results); every row further out, and every row of an
    undefined sentence, takes exactly zero."""
    X, valid, ns, P, up, dims = _stage_case(KS)
    B, S, L, V, _, KC = dims
    vp, final, pp, pn, vs, keep = _masked_stage(X, valid, P, dims)
    defined = (C.lout(ns, KS) >= 1)
    assert bool(defined[0].any()) and not bool(defined[1].any()) and not bool(defined.view(-1)[3])
    assert (KS % 2 == 1) == bool(defined[0, 2])          # the one-token sentence
    und = ~defined.view(-1)
    for name in ("cmax", "sp", "view_p"):
        t = keep[name][und]
        assert torch.equal(t, torch.zeros_like(t)) and not bool(torch.signbit(t).any()), name
    assert bool((keep["argl"][und] == -1).all()) and bool((keep["argl"][~und] >= 0).all())
    assert bool((keep["argl"][~und] < keep["lout"][~und].view(-1, 1)).all())
    for t in (final[1], pp[1], pn[1], vs[1]):               # the sample without a defined sentence: 0, never NaN
        assert torch.equal(t, torch.zeros_like(t))
    tv, tf, tpp, tpn, tvs = _truncated_stage(X, ns, P, dims)
    for name, a, b in (("view_p", vp, tv), ("final", final, tf), ("prefer_pos", pp, tpp), ("prefer_neg", pn, tpn), ("view_score", vs, tvs)):
        assert float((a - b).detach().abs().max()) <= 1e-12, (name, float((a - b).detach().abs().max()))
    assert float(pp.detach().abs().max()) > 0 or float(pn.detach().abs().max()) > 0
    leaves = [X] + list(P.values())
    loss = lambda o: (o[0] * up["vp"]).sum() + (o[1] * up["final"]).sum() + (o[2] * up["pp"]).sum() + (o[3] * up["pn"]).sum()
    gm = torch.autograd.grad(loss((vp, final, pp, pn)), leaves, allow_unused=True)
    gt = torch.autograd.grad(loss((tv, tf, tpp, tpn)), leaves, allow_unused=True)
    spill = KS - 1 - (KS - 1) // 2
    inside = torch.arange(L).view(1, 1, L) < ns.view(B, S, 1)
    for name, a, b in zip(["X"] + list(P), gm, gt):
        a = torch.zeros_like(leaves[0] if name == "X" else P[name]) if a is None else a
        b = torch.zeros_like(a) if b is None else b
        assert bool(torch.isfinite(a).all()), name
        if name == "X":
            far = (torch.arange(L).view(1, 1, L) >= (ns + spill).view(B, S, 1)) | ~defined.view(B, S, 1)
            # S-Net-valid tokens of a head-undefined sentence (one token, even KS) still take exactly zero: view_p = 0 there
            assert torch.equal(a[far], torch.zeros_like(a[far])), "masked rows of X take a gradient"
            a, b = a * inside.unsqueeze(-1), b * inside.unsqueeze(-1)
        assert float((a - b).abs().max()) <= 1e-12 * max(1.0, float(b.abs().max())), (name, float((a - b).abs().max()))
        assert float(b.abs().max()) > 0, name


def test_all_valid_mask_is_the_oracle_head():
    x = C.make_inputs(2, 3, 11, 4, 2, 120)
    B, S, L, V, KS, KC = x["dims"]
    keep = {}
    K.head(x["X"].double(), torch.ones(B * S, L, dtype=torch.bool), x["Wc"].double(), x["bc"].double(), x["Wl"].double(),
           x["bl"].double(), C.THR32, keep)
    d = C.decisions64(x)
    assert torch.equal(keep["argl"], d.argl) and torch.equal(keep["cmax"], d.f.cmax) and torch.equal(keep["view_p"], d.f.view_p)


def _gru_params(seed):
    from umpr_amd.synthetic import make_param_state
    return {k: v.double() for k, v in make_param_state(seed, 50, 900, 1, False, with_vgg=False, m_scale=0.05).items()}


def test_own_states_gru():
    """equal to ImprovedRnn when the flat lengths are strictly descending (the sort is the identity); different as soon as a
    longer sentence stands later in the batch"""
    P = _gru_params(5)
    pre = "control_net.c_net.gru.module."
    g = torch.Generator().manual_seed(6)
    x = torch.randn(5, 9, 50, generator=g, dtype=torch.float64)
    desc = torch.tensor([9, 7, 4, 2, 1])
    own = K.gru(x, desc, P, pre, unsort=True)
    assert torch.equal(own, R.improved_rnn(x, desc, P, pre))
    assert torch.equal(own, R.improved_rnn(x, desc, P, pre, aten=True)) or float((own - R.improved_rnn(x, desc, P, pre, aten=True)).abs().max()) < 1e-12
    for n in range(5):
        assert torch.equal(own[n, int(desc[n]):], torch.zeros_like(own[n, int(desc[n]):])) and float(own[n, :int(desc[n])].abs().min()) > 0
    later = torch.tensor([4, 7, 9, 2, 1])
    a, b = K.gru(x, later, P, pre, unsort=True), R.improved_rnn(x, later, P, pre)
    assert float((a - b).abs().max()) > 1e-2
    # own states: out[n] depends on x[n] and len[n] only
    assert torch.equal(a[1], own[1]) and torch.equal(a[3:], own[3:])


def _stand_in_vgg(flat):
    """a per-photo stand-in for the VGG (batch independent, like the real one): 1000 features of each photo's own pixels"""
    return torch.tanh(flat.flatten(1)[:, ::150][:, :1000] * 3 - 1.5)


def invariance_legs(seed=INV_SEED):
    """float64 predictions / ControlNet outputs of row 0, alone and in the batch, for the four option settings"""
    from umpr_amd.synthetic import make_param_state
    P = {k: v.double() for k, v in make_param_state(700 + seed, 50, 900, 1, False, with_vgg=False, m_scale=0.05).items()}
    alone, batch = K.invariance_batch(seed)
    alone, batch = ([t.double() if t.is_floating_point() else t for t in b] for b in (alone, batch))
    out = {}
    with torch.no_grad():
        for leg, opts in (("on", (True, True, True)), ("mask_padding", (False, True, True)), ("mask_control", (True, False, True)),
                          ("unsort_gru", (True, True, False))):
            res = []
            for b in (alone, batch):
                keep = {}
                pred, _ = K.umpr_forward(P, b, review_net_only=False, mask_padding=opts[0], mask_control=opts[1], unsort_gru=opts[2],
                                         vgg_fn=_stand_in_vgg, keep=keep)
                res.append((pred[0], torch.stack([keep[k][0] for k in ("c_u", "c_i", "prefer_pos", "prefer_neg")])))
            out[leg] = res
    return out, alone, batch


def test_invariance_batch():
    """Chosen here, on the CPU, from the reference alone (float64).  The batch-mates enlarge S, L, S_ui and L_ui and the length sort
    moves row 0's sentences.  All three options on: prediction and ControlNet outputs of row 0 agree within 1e-12.  One option
    off - which quantity each leg is held on:
      * mask_padding off: the PREDICTION (the ControlNet does not depend on this option at all);
      * mask_control off: the ControlNet's four outputs c_u, c_i, prefer_pos, prefer_neg.  The prediction sees them only through
        c_u c_i (1 - match), and match comes from the VGG, which this file replaces by a per-photo stand-in (a float64 VGG16 is
        minutes of CPU): the reference alone, without the VGG, settles the condition on the four outputs only.  (With the
        stand-in features the prediction moves by 9e-3 as well; asserted below, not relied on by the GPU test.)
      * unsort_gru off: the PREDICTION.
    tests/test_gpu_control_mask.py holds the model to the same quantities."""
    out, alone, batch = invariance_legs()
    assert batch[0].shape[1] > alone[0].shape[1] and batch[0].shape[2] > alone[0].shape[2]
    assert batch[2].shape[1] > alone[2].shape[1] and batch[2].shape[2] > alone[2].shape[2]
    # the sort moves row 0's sentences: the reference's permutation is not the identity on them
    for lens in (batch[3], batch[4], batch[5]):
        order, _ = R.gru_sort_indices(lens.reshape(-1))
        S = lens.shape[1]
        assert order[:S].tolist() != list(range(S))
    (pa, ca), (pb, cb) = out["on"]
    assert float(pa) > 0.05, "the fusion ReLU must not clip the prediction"
    assert abs(float(pa - pb)) <= 1e-12 and float((ca - cb).abs().max()) <= 1e-12
    assert float(ca.abs().max()) > 0
    big = 10 * K.PARITY
    d = {leg: (abs(float(out[leg][0][0] - out[leg][1][0])), float((out[leg][0][1] - out[leg][1][1]).abs().max())) for leg in out}
    print(d)
    assert d["mask_padding"][0] > big, d
    assert d["mask_control"][1] > big and d["mask_control"][0] > big, d
    assert d["unsort_gru"][0] > big, d


def umpr_r_legs(seed=INV_SEED):
    """|prediction alone - prediction in the batch| of row 0 in float64 for UMPR-R: both options on, and each one off"""
    from umpr_amd.synthetic import make_param_state
    P = {k: v.double() for k, v in make_param_state(700 + seed, 50, 900, 1, True, with_vgg=False, m_scale=0.05).items()}
    alone, batch = K.invariance_batch(seed, full=False)
    d = {}
    with torch.no_grad():
        for leg, (mp, ug) in (("on", (True, True)), ("mask_padding", (False, True)), ("unsort_gru", (True, False))):
            pa, pb = (K.umpr_forward(P, b, review_net_only=True, mask_padding=mp, unsort_gru=ug)[0][0] for b in (alone, batch))
            d[leg] = (abs(float(pa - pb)), float(pa))
    return d


def test_invariance_batch_umpr_r():
    """the same batch for UMPR-R (mask_padding + unsort_gru; there is no ControlNet): held on the prediction"""
    d = umpr_r_legs()
    print(d)
    assert d["on"][1] > 0.05 and d["on"][0] <= 1e-12, d
    assert d["mask_padding"][0] > 10 * K.PARITY and d["unsort_gru"][0] > 10 * K.PARITY, d


def constructed_legs(seed=INV_SEED):
    """float64 prediction / ControlNet outputs of row 0, alone and in the batch, for both options on and each one off"""
    from umpr_amd.synthetic import make_param_state
    P = {k: v.double() for k, v in make_param_state(700 + seed, 50, 900, 1, False, with_vgg=False, m_scale=0.05).items()}
    alone, batch = K.constructed_batch(seed)
    alone, batch = ([t.double() if t.is_floating_point() else t for t in b] for b in (alone, batch))
    out = {}
    with torch.no_grad():
        for leg, opts in (("on", (True, True)), ("mask_padding", (False, True)), ("mask_control", (True, False))):
            res = []
            for b in (alone, batch):
                keep = {}
                pred, _ = K.umpr_forward(P, b, review_net_only=False, mask_padding=opts[0], mask_control=opts[1], vgg_fn=_stand_in_vgg, keep=keep)
                res.append((pred[0], torch.stack([keep[k][0] for k in ("c_u", "c_i", "prefer_pos", "prefer_neg")])))
            out[leg] = res
    return out, alone, batch


def test_constructed_batch():
    """The two masks WITHOUT --unsort_gru, under the reference's GRU permutation: a batch built so that row 0's real sentences keep
    their own states (what the masks alone can promise).  Chosen here, on the CPU, from the reference alone (float64).  The batch pads row 0 further on all three review inputs: S, L,
    S_ui and L_ui all grow, and row 0's padded sentences receive other sentences' states.  Both options on: prediction and
    ControlNet outputs of row 0 agree within 1e-12.  One option off - which quantity each leg is held on:
      * mask_padding off: the PREDICTION (the ControlNet does not depend on this option at all);
      * mask_control off: the ControlNet's four outputs c_u, c_i, prefer_pos, prefer_neg.  The prediction sees them only through
        c_u c_i (1 - match), and match comes from the VGG, which this file replaces by a per-photo stand-in (a float64 VGG16 is
        minutes of CPU): the reference alone, without the VGG, settles the condition on the four outputs only.
    tests/test_gpu_control_mask.py holds the model to the same quantities."""
    out, alone, batch = constructed_legs()
    assert batch[0].shape[1] > alone[0].shape[1] and batch[0].shape[2] > alone[0].shape[2]
    assert batch[2].shape[1] > alone[2].shape[1] and batch[2].shape[2] > alone[2].shape[2]
    (pa, ca), (pb, cb) = out["on"]
    assert float(pa) > 0.05, "the fusion ReLU must not clip the prediction"
    assert abs(float(pa - pb)) <= 1e-12 and float((ca - cb).abs().max()) <= 1e-12
    assert float(ca.abs().max()) > 0
    big = 10 * K.PARITY
    d = {leg: (abs(float(out[leg][0][0] - out[leg][1][0])), float((out[leg][0][1] - out[leg][1][1]).abs().max())) for leg in out}
    print(d)
    assert d["mask_padding"][0] > big, d
    assert d["mask_control"][1] > big, d
