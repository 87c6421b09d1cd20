"""The key-padding mask of the ReviewNet's softmaxes (`--mask_padding True`), CPU half: the restatement of
tests/masked_attention_reference.py against the oracle (all-valid mask: the same bits), against the definition (compaction
identity in float64: at the valid positions the masked result IS the reference's formulas on the inputs with the masked positions
removed, gradients included, and masked positions take exactly zero gradient), its hand-written backwards against autograd, and
the option's way through main.py's flags, the model and the checkpoints.  No GPU needed."""
import numpy as np
import pytest
import torch

import masked_attention_reference as MA
from oracle import umpr_ref as R
from umpr_amd.synthetic import make_batch, make_param_state

REL = 1e-12          # compaction identity, float64: the two sides differ in summation order only
F64 = torch.float64


def _close(got, ref, what, rel=REL):
    scale = float(ref.abs().max())
    err = float((got - ref).abs().max())
    assert err <= rel * max(scale, 1e-300) or (scale == 0 and err == 0), (what, err, scale)


@pytest.fixture
def main_config():
    import main
    from umpr_amd.config import Config
    saved = Config._extra
    Config.extend(main.EXTRA_OPTIONS)
    yield lambda *argv: Config(argv=list(argv))
    Config._extra = saved


# ---- the validity rule ----------------------------------------------------------------------------------------------------------
def test_token_valid_rule():
    ids = np.array([[5, 0, 7, 9], [1, 2, 3, 4], [0, 0, 0, 0], [6, 6, 6, 6], [2, 2, 2, 2]])
    lengths = np.array([3, 9, 1, 0, -2])                 # inside, above L, a padded sentence (length 1, id 0), zero, negative
    v = MA.token_valid(ids, lengths)
    assert v.dtype == np.bool_ and v.tolist() == [[True, False, True, False], [True] * 4, [False] * 4, [False] * 4, [False] * 4]
    assert MA.token_valid(ids, lengths, pad_id=6)[3].tolist() == [False] * 4
    assert MA.token_valid(ids, np.array([4] * 5), pad_id=2).tolist()[4] == [False] * 4      # <UNK> = 1, <NUM> = 2 are words at pad_id 0
    assert MA.token_valid(ids, np.array([4] * 5))[1].tolist() == [True] * 4


# ---- all valid: the oracle's bits -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_all_valid_mask_is_the_oracle_bit_for_bit(dtype):
    P = {k: v.to(dtype) for k, v in make_param_state(3, 50, 200, 1, True, m_scale=0.05).items()}
    batch = make_batch(11, 3, 200, 1, max_sent_count=4, min_sent_count=2, max_sent_length=9, review_net_only=True)
    u, i, _, ul, il = batch[:5]
    ue, ie = torch.nn.functional.embedding(u, P["embedding.weight"]), torch.nn.functional.embedding(i, P["embedding.weight"])
    B, S, L = u.shape
    ones = torch.ones(B, S * L, dtype=torch.bool)
    ko, km = {}, {}
    out_o = R.review_net(ue, ie, ul, il, P, keep=ko)
    out_m = MA.review_net(ue, ie, ul, il, P, ones, ones, keep=km)
    assert torch.equal(out_o, out_m)
    for k in ko:
        assert torch.equal(ko[k], km[k]), k
    sa_o, se_o = R.s_net(ko["gru_u"], ko["soft_u"], L, P, "review_net.s_net_u.")
    sa_m, se_m = MA.s_net(ko["gru_u"], ko["soft_u"], L, P, "review_net.s_net_u.", ones)
    assert torch.equal(sa_o, sa_m) and torch.equal(se_o, se_m)


# ---- compaction identity --------------------------------------------------------------------------------------------------------
def _coattn_problem(seed=5, B=4, SL=13, Dm=8):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    Gu, Gi, M = rn(B, SL, Dm), rn(B, SL, Dm), 0.3 * rn(Dm, Dm)
    vu, vi = torch.rand(B, SL, generator=g) < 0.6, torch.rand(B, SL, generator=g) < 0.6
    vu[1] = False; vu[1, 7] = True                      # a single valid user position
    vi[2] = False                                       # no valid item position: nothing of sample 2 is defined
    vu[3] = True; vi[3] = True                          # all valid
    w = dict(su=rn(B, SL), si=rn(B, SL), au=rn(B, Dm), ai=rn(B, Dm))
    return Gu, Gi, M, vu, vi, w


def _unmasked_coattention(gu, gi, M):
    """oracle r_net, model.py:50-55, on one sample [n][D]"""
    A = torch.tanh(gi @ M @ gu.transpose(-1, -2))
    soft_u = torch.softmax(torch.max(A, dim=-2).values, dim=-1)
    soft_i = torch.softmax(torch.max(A, dim=-1).values, dim=-1)
    return soft_u, soft_i, gu.transpose(-1, -2) @ soft_u, gi.transpose(-1, -2) @ soft_i


def test_coattention_compaction_identity():
    Gu, Gi, M, vu, vi, w = _coattn_problem()
    B = Gu.shape[0]
    a = [t.clone().requires_grad_(True) for t in (Gu, Gi, M)]
    su, si, au, ai = MA.coattention(*a, vu, vi)
    assert not any(bool(torch.isnan(t).any()) for t in (su, si, au, ai))
    ((su * w["su"]).sum() + (si * w["si"]).sum() + (au * w["au"]).sum() + (ai * w["ai"]).sum()).backward()
    c = [t.clone().requires_grad_(True) for t in (Gu, Gi, M)]
    loss = 0
    for b in range(B):
        ku, ki = vu[b].nonzero().squeeze(-1), vi[b].nonzero().squeeze(-1)
        if len(ku) == 0 or len(ki) == 0:               # nothing defined: soft = 0 and atte = 0 on both sides, exactly
            for t in (su[b], si[b], au[b], ai[b]):
                assert bool((t == 0).all())
            continue
        csu, csi, cau, cai = _unmasked_coattention(c[0][b][ku], c[1][b][ki], c[2])
        _close(su[b][ku].detach(), csu.detach(), f"soft_u[{b}]"); _close(si[b][ki].detach(), csi.detach(), f"soft_i[{b}]")
        _close(au[b].detach(), cau.detach(), f"atte_u[{b}]"); _close(ai[b].detach(), cai.detach(), f"atte_i[{b}]")
        assert bool((su[b][~vu[b]] == 0).all()) and bool((si[b][~vi[b]] == 0).all())
        loss = loss + (csu * w["su"][b][ku]).sum() + (csi * w["si"][b][ki]).sum() + (cau * w["au"][b]).sum() + (cai * w["ai"][b]).sum()
    loss.backward()
    defined_u, defined_i = vu & vi.any(-1, keepdim=True), vi & vu.any(-1, keepdim=True)
    _close(a[0].grad[defined_u], c[0].grad[defined_u], "dGu"); _close(a[1].grad[defined_i], c[1].grad[defined_i], "dGi")
    _close(a[2].grad, c[2].grad, "dM")
    assert bool((a[0].grad[~defined_u] == 0).all()) and bool((a[1].grad[~defined_i] == 0).all())
    assert float(a[0].grad[defined_u].abs().max()) > 0 and float(a[2].grad.abs().max()) > 0


def _snet_problem(seed=9, B=2, S=3, L=7, Dm=8, AT=5):
    g = torch.Generator().manual_seed(seed)
    rn = lambda *s: torch.randn(*s, generator=g, dtype=F64)
    X, Ms, Ws, word_soft = rn(B, S, L, Dm), 0.4 * rn(AT, Dm), rn(AT), torch.rand(B, S, L, generator=g, dtype=F64)
    valid = torch.rand(B, S, L, generator=g) < 0.6
    valid[0, 1] = False                                 # an empty sentence
    valid[1, 0] = False; valid[1, 0, 0] = True          # first token only
    valid[1, 2] = True                                  # a full sentence
    return X, Ms, Ws, word_soft, valid, rn(B, Dm), rn(B, S, Dm)


def test_snet_compaction_identity():
    X, Ms, Ws, word_soft, valid, d_senti, d_sa = _snet_problem()
    B, S, L, Dm = X.shape
    P = {"p.Ms": Ms.clone().requires_grad_(True), "p.Ws": Ws.reshape(1, -1).clone().requires_grad_(True)}
    Xa = X.clone().requires_grad_(True)
    keep = {}
    sa, senti = MA.s_net(Xa.reshape(B, S * L, Dm), word_soft.reshape(B, S * L), L, P, "p.", valid.reshape(B, S * L), keep=keep)
    ((senti * d_senti).sum() + (sa * d_sa).sum()).backward()
    Pc = {"p.Ms": Ms.clone().requires_grad_(True), "p.Ws": Ws.reshape(1, -1).clone().requires_grad_(True)}
    Xc = X.clone().requires_grad_(True)
    loss = 0
    for b in range(B):
        senti_b = torch.zeros(Dm, dtype=F64)
        for s in range(S):
            k = valid[b, s].nonzero().squeeze(-1)
            if len(k) == 0:
                assert bool((sa[b, s] == 0).all()) and bool((keep["P"][b, s] == 0).all())
                continue
            # oracle s_net, model.py:75-80, on the sentence with its masked tokens removed; wsum keeps its formula (all of word_soft)
            sa_c, senti_c = R.s_net(Xc[b, s][k].unsqueeze(0), word_soft[b, s].unsqueeze(0), len(k), Pc, "p.")
            _close(sa[b, s].detach(), sa_c.reshape(-1).detach(), f"self_atte[{b}][{s}]")
            assert bool((keep["P"][b, s][~valid[b, s]] == 0).all())
            senti_b = senti_b + senti_c.reshape(-1)
            loss = loss + (sa_c.reshape(-1) * d_sa[b, s]).sum()
        _close(senti[b].detach(), senti_b.detach(), f"senti[{b}]")
        loss = loss + (senti_b * d_senti[b]).sum()
    loss.backward()
    _close(Xa.grad[valid], Xc.grad[valid], "dX"); _close(P["p.Ms"].grad, Pc["p.Ms"].grad, "dMs"); _close(P["p.Ws"].grad, Pc["p.Ws"].grad, "dWs")
    assert bool((Xa.grad[~valid] == 0).all()) and float(Xa.grad[valid].abs().max()) > 0


# ---- the hand-written backwards -------------------------------------------------------------------------------------------------
def test_hand_written_coattention_backward_agrees_with_autograd():
    Gu, Gi, M, vu, vi, w = _coattn_problem(seed=6)
    a = [t.clone().requires_grad_(True) for t in (Gu, Gi, M)]
    keep = {}
    su, si, au, ai = MA.coattention(*a, vu, vi, keep=keep)
    ((su * w["su"]).sum() + (si * w["si"]).sum() + (au * w["au"]).sum() + (ai * w["ai"]).sum()).backward()
    undefined = ~(vu & vi.any(-1, keepdim=True))
    assert bool((keep["argcol"][undefined] == -1).all()) and bool((keep["colmax"][undefined] == 0).all())
    assert bool((keep["argcol"][~undefined] >= 0).all())
    got = MA.coattention_backward64(Gu, Gi, M, keep["argcol"], keep["argrow"], w["au"], w["ai"], w["su"], w["si"])
    for name, g, r in zip(("dGu", "dGi", "dM"), got, (t.grad for t in a)):
        _close(g, r, name, rel=1e-11)
    assert bool((got[0][undefined] == 0).all())


def test_hand_written_snet_backward_agrees_with_autograd():
    X, Ms, Ws, word_soft, valid, d_senti, d_sa = _snet_problem(seed=10)
    a = [t.clone().requires_grad_(True) for t in (X, Ms, Ws, word_soft)]
    f = MA.snet_forward(*a, valid)
    ((f["senti"] * d_senti).sum() + (f["self_atte"] * d_sa).sum()).backward()
    got = MA.snet_backward64(X, Ms, Ws, word_soft, valid, d_senti, d_sa)
    for name, g, r in zip(("dX", "dMs", "dWs", "d_word_soft"), got, (t.grad for t in a)):
        _close(g, r, name, rel=1e-11)
    assert bool((got[0][~valid] == 0).all())
    # snet_forward is s_net
    B, S, L, Dm = X.shape
    sa, senti = MA.s_net(X.reshape(B, S * L, Dm), word_soft.reshape(B, S * L), L, {"p.Ms": Ms, "p.Ws": Ws.reshape(1, -1)}, "p.",
                         valid.reshape(B, S * L))
    _close(f["self_atte"].detach(), sa, "self_atte"); _close(f["senti"].detach(), senti, "senti")


# ---- padding invariance of the references (the seed of tests/test_gpu_mask_padding.py) ------------------------------------------
INVARIANCE_SEED = 1
PARITY = 1e-4        # the project's parity bound for predictions


def invariance_differences(dtype):
    """|pred alone - pred as row 0 of the batch of 4| of the references, (mask on, mask off)"""
    P = {k: v.to(dtype) for k, v in make_param_state(21, 50, 900, 1, True, m_scale=0.05).items()}
    alone, batch = MA.invariance_batch(INVARIANCE_SEED)
    cast = lambda b: tuple(t.to(dtype) if t.is_floating_point() else t for t in b)
    with torch.no_grad():
        d = [abs(float(MA.umpr_r_forward(P, cast(batch), mask=m)[0][0]) - float(MA.umpr_r_forward(P, cast(alone), mask=m)[0][0]))
             for m in (True, False)]
    return d


@pytest.mark.parametrize("dtype", [torch.float32, torch.float64])
def test_references_are_padding_invariant_with_the_mask_only(dtype):
    """Seed 1: 0.0 with the mask (float32 and float64), 1.50e-2 without."""
    alone, batch = MA.invariance_batch(INVARIANCE_SEED)
    assert alone[0].shape == (1, 4, 10) and batch[0].shape == (4, 6, 13)
    assert torch.equal(batch[0][0, :4, :10], alone[0][0]) and torch.equal(batch[1][0, :4, :10], alone[1][0])
    on, off = invariance_differences(dtype)
    assert on <= 0.1 * PARITY, on
    assert off > 10 * PARITY, off


# ---- the option: flags, model, checkpoints --------------------------------------------------------------------------------------
EMB = np.zeros((40, 50), dtype=np.float32)


def test_option_parses_and_travels(main_config, tmp_path):
    import main
    from umpr_amd.checkpoint import load_checkpoint, save_checkpoint
    from umpr_amd.model import UMPR
    cfg = main_config("--review_net_only", "True")
    assert cfg.mask_padding is False
    main.check_flags(cfg)
    on = main_config("--review_net_only", "True", "--mask_padding", "True")
    assert on.mask_padding is True
    main.check_flags(on)
    main.check_flags(main_config("--mask_padding", "True", "--train_embedding", "True", "--review_store", "True", "--freeze_conv", "True"))
    with pytest.raises(SystemExit, match="--mask_padding takes True or False"):
        main.check_flags(main_config("--mask_padding", "1"))
    plain, masked = UMPR(cfg, EMB), UMPR(on, EMB)
    assert plain.mask_padding is False and masked.mask_padding is True
    assert list(plain.state_dict()) == list(masked.state_dict())               # no parameter added: weights interchange
    masked.load_state_dict(plain.state_dict())
    p_on, p_off = str(tmp_path / "on.pt"), str(tmp_path / "off.pt")
    save_checkpoint(p_on, masked)
    save_checkpoint(p_off, plain)
    assert torch.load(p_on, weights_only=True)["mask_padding"] is True
    assert torch.load(p_off, weights_only=True)["mask_padding"] is False
    load_checkpoint(p_on, UMPR(on, EMB))
    load_checkpoint(p_off, UMPR(cfg, EMB))
    for path, model in ((p_on, plain), (p_off, masked)):
        before = {k: v.clone() for k, v in model.state_dict().items()}
        with pytest.raises(ValueError, match="--mask_padding"):
            load_checkpoint(path, model)
        assert all(torch.equal(v, before[k]) for k, v in model.state_dict().items())
    # a checkpoint from before the option, and a bare state_dict: both count as False
    old = torch.load(p_off, weights_only=True)
    del old["mask_padding"]
    p_old, p_bare = str(tmp_path / "old.pt"), str(tmp_path / "bare.pt")
    torch.save(old, p_old)
    torch.save(old["model"], p_bare)
    for path in (p_old, p_bare):
        load_checkpoint(path, plain)
        with pytest.raises(ValueError, match="--mask_padding False"):
            load_checkpoint(path, masked)
