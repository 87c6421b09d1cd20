"""`--mask_control True` and `--unsort_gru True`, restated on the CPU (test helper, not a test module).

The definitions the kernels are held to (umpr_cnet_head_fwd_masked, umpr_control_net_fwd_ex, umpr_review_net_fwd_ex), written with
torch in whatever dtype the inputs have, so that autograd differentiates them:

  token validity   masked_attention_reference.token_valid on ids_ui / len_ui and on ids_pair / len_pair, PAD_ID = 0
  n_s              the length of the LEADING run of valid bytes of a sentence (leading_run): for everything the loader produces the
                   number of valid tokens; a hole ends the run - (valid, invalid, valid) gives n_s = 1
  C-Net head       the conv Y over the padded width as in the reference; cmax[k] / argl[k] over the conv positions
                   l < control_decisions.lout(n_s, KS) only, argl the first position that attains the maximum.  A sentence with
                   lout(n_s, KS) < 1 (a padded sentence; one token under an even KS) is undefined: cmax = +0.0, argl = -1,
                   sp = +0.0, view_p = +0.0 for every k and v - it adds +0.0 to final, and a sample without a defined sentence has
                   final = 0, view_score = 0, prefer_* = 0                                                                  (head)
  control S-Net    masked_attention_reference.s_net on the ui validity                                               (control_net)
  gate             the reference's formulas, unchanged: every term carries a factor view_p
  own-states GRU   out[n] = BiGRU(x[n])[:len[n]], zero past len[n]: pack_padded_sequence(enforce_sorted=False) +
                   pad_packed_sequence without the reference's extra gather                                               (gru)

With an all-valid mask and unsort_gru off every function performs the oracle's operations.  tests/test_control_mask_reference.py
pins the definitions without trusting this file: the masked result equals the reference's own formulas on the sample with every
sentence cut to n_s and the undefined sentences removed.
"""
import torch
import torch.nn.functional as F

import control_decisions as C
import masked_attention_reference as M
from oracle import umpr_ref as R

PAD_ID = M.PAD_ID
PARITY = 1e-4


def leading_run(valid):
    """n_s [...]: the length of the leading run of True along the last axis of valid [...][L]"""
    return torch.cumprod(torch.as_tensor(valid).long(), -1).sum(-1)


def gru(x, lengths, P, prefix, unsort=False, aten=False):
    """ImprovedRnn (oracle.improved_rnn) or, with unsort, the same recurrence with every row keeping its own states"""
    if not unsort:
        return R.improved_rnn(x, lengths, P, prefix, aten)
    names = ["weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"]
    fw = [P[prefix + n] for n in names]
    bw = [P[prefix + n + "_reverse"] for n in names]
    lens = lengths.to(x.device)
    return torch.cat([R.gru_cell_seq(x, lens, *fw, reverse=False), R.gru_cell_seq(x, lens, *bw, reverse=True)], dim=-1)


def head(X, valid, Wc, bc, Wl, bl, thr=C.THR32, keep=None):
    """The masked C-Net head on X [N][L][128] with valid bool [N][L]: (view_p [N][V], sp, cmax [N][KC], argl [N][KC])."""
    N, L, _ = X.shape
    KS = Wc.shape[-1]
    pad = (KS - 1) // 2
    # all L positions, as the window GEMM writes them; the eligible ones are a prefix of nn.Conv1d's
    Y = torch.relu(F.conv1d(F.pad(X.transpose(1, 2), (pad, KS - 1 - pad)), Wc, bc).transpose(1, 2))
    lo = C.lout(leading_run(valid), KS)                                         # [N]
    defined = lo >= 1
    elig = torch.arange(L).view(1, L) < lo.view(N, 1)
    Ym = torch.where(elig.unsqueeze(-1), Y, torch.full_like(Y, float("-inf")))
    Ym = torch.where(defined.view(N, 1, 1), Ym, torch.zeros_like(Y))            # no all -inf column reaches a max
    _, first = C.first_argmax(Ym.detach())
    cmax = Ym.gather(1, first.unsqueeze(1)).squeeze(1)
    cmax = torch.where(defined.view(N, 1), cmax, torch.zeros_like(cmax))
    sp = torch.sigmoid(cmax @ Wl.t() + bl)
    sp = torch.where(defined.view(N, 1), sp, torch.zeros_like(sp))
    vp = torch.where(sp < thr, torch.zeros_like(sp), sp)
    argl = torch.where(defined.view(N, 1), first, torch.full_like(first, -1))
    if keep is not None:
        keep.update(Y=Y, cmax=cmax, argl=argl, sp=sp, view_p=vp, defined=defined, lout=lo)
    return vp, sp, cmax, argl


def c_net(review_emb, lengths, P, threshold, valid=None, unsort=False, prefix="control_net.c_net.", aten=False):
    """oracle c_net; valid bool [B*S][L] switches the head to the masked one"""
    B, S, L, E = review_emb.shape
    g = gru(review_emb.reshape(B * S, L, E), lengths.reshape(-1), P, prefix + "gru.module.", unsort, aten)
    if valid is None:
        k = P[prefix + "cnn.0.weight"].shape[-1]
        out = F.relu(F.conv1d(g.transpose(-1, -2), P[prefix + "cnn.0.weight"], P[prefix + "cnn.0.bias"], padding=(k - 1) // 2))
        out = out.max(dim=-1)[0]
        view_p = torch.sigmoid(F.linear(out, P[prefix + "linear.0.weight"], P[prefix + "linear.0.bias"]))
        view_p = torch.where(view_p < threshold, torch.zeros_like(view_p), view_p)
    else:
        view_p = head(g, valid, P[prefix + "cnn.0.weight"], P[prefix + "cnn.0.bias"], P[prefix + "linear.0.weight"],
                      P[prefix + "linear.0.bias"], threshold)[0]
    view_p = view_p.view(B, S, -1)
    return g.reshape(B, S * L, -1), view_p, torch.sum(view_p ** 2, dim=-2)


def gate(s, view_p, c_out, P, pre="control_net."):
    """oracle control_net lines 154-161 on the control S-Net's self attention s [B][S][128]"""
    senti = torch.sigmoid(F.linear(s, P[pre + "ss_net.linear.0.weight"], P[pre + "ss_net.linear.0.bias"]))
    senti = senti.expand(-1, -1, view_p.shape[-1])
    view_score = torch.sum(senti * view_p ** 2, dim=-2).div(torch.sum(view_p ** 2, dim=-2) + 1e-4)
    q_p = (view_score > 0.5).to(view_score.dtype)
    q_pos = torch.where(view_score < 0.5, torch.zeros_like(view_score), 4 * (view_score - 0.5) ** 2)
    q_neg = torch.where(view_score > 0.5, torch.zeros_like(view_score), 4 * (0.5 - view_score) ** 2)
    return c_out * q_p * q_pos, c_out * (1 - q_p) * q_neg, view_score


def control_net(user_emb, item_emb, ui_emb, u_len, i_len, ui_len, P, threshold, valid=None, unsort=False, aten=False):
    """oracle control_net; valid = (v_ui [B*S_ui][L_ui], v_u [B*S][L], v_i [B*S][L]) bool for --mask_control"""
    pre = "control_net."
    L_ui = ui_emb.shape[-2]
    v_ui, v_u, v_i = valid if valid is not None else (None, None, None)
    gru_repr, view_p, c_out = c_net(ui_emb, ui_len, P, threshold, v_ui, unsort, pre + "c_net.", aten)
    _, _, c_u = c_net(user_emb, u_len, P, threshold, v_u, unsort, pre + "c_net.", aten)
    _, _, c_i = c_net(item_emb, i_len, P, threshold, v_i, unsort, pre + "c_net.", aten)
    if valid is None:
        s, _ = R.s_net(gru_repr, view_p, L_ui, P, pre + "s_net.")
    else:
        s, _ = M.s_net(gru_repr, view_p, L_ui, P, pre + "s_net.", v_ui)
    pp, pn, vs = gate(s, view_p, c_out, P, pre)
    return c_u, c_i, pp, pn, dict(view_p=view_p, view_score=vs, c_out=c_out)


def review_net(user_emb, item_emb, u_len, i_len, P, valid=None, unsort=False, aten=False):
    """oracle review_net; valid = (vu, vi) bool [B][S*L] for --mask_padding"""
    pre = "review_net."
    B, S, L, E = user_emb.shape
    gp = pre + "r_net.gru.module."
    gru_u = gru(user_emb.reshape(B * S, L, E), u_len.reshape(-1), P, gp, unsort, aten).reshape(B, S * L, -1)
    gru_i = gru(item_emb.reshape(B * S, L, E), i_len.reshape(-1), P, gp, unsort, aten).reshape(B, S * L, -1)
    if valid is None:
        A = torch.tanh(gru_i @ P[pre + "r_net.M"] @ gru_u.transpose(-1, -2))
        soft_u = torch.softmax(torch.max(A, dim=-2).values, dim=-1)
        soft_i = torch.softmax(torch.max(A, dim=-1).values, dim=-1)
        atte_u = (gru_u.transpose(-1, -2) @ soft_u.unsqueeze(-1)).squeeze(-1)
        atte_i = (gru_i.transpose(-1, -2) @ soft_i.unsqueeze(-1)).squeeze(-1)
        _, senti_u = R.s_net(gru_u, soft_u, L, P, pre + "s_net_u.")
        _, senti_i = R.s_net(gru_i, soft_i, L, P, pre + "s_net_i.")
    else:
        vu, vi = valid
        soft_u, soft_i, atte_u, atte_i = M.coattention(gru_u, gru_i, P[pre + "r_net.M"], vu, vi)
        _, senti_u = M.s_net(gru_u, soft_u, L, P, pre + "s_net_u.", vu)
        _, senti_i = M.s_net(gru_i, soft_i, L, P, pre + "s_net_i.", vi)
    repr_u = torch.cat([atte_u, senti_u], dim=-1)
    repr_i = torch.cat([atte_i, senti_i], dim=-1)
    return torch.tanh(F.linear(repr_u, P[pre + "linear_u.weight"]) + F.linear(repr_i, P[pre + "linear_i.weight"]))


def batch_valid_ui(batch):
    """bool [B*S_ui][L_ui] of a batch tuple"""
    ui, ui_len = batch[2], batch[5]
    B, S, L = ui.shape
    return torch.from_numpy(M.token_valid(ui.reshape(B * S, L).numpy(), ui_len.reshape(-1).numpy(), PAD_ID))


def umpr_forward(P, batch, *, review_net_only, mask_padding=False, mask_control=False, unsort_gru=False, threshold=0.35,
                 loss_v_rate=0.1, vgg_fn=None, aten=False, keep=None):
    """oracle umpr_forward (eval mode) with the three options; all off is the oracle's arithmetic"""
    user_reviews, item_reviews, ui_reviews, u_len, i_len, ui_len, photos, labels = batch
    emb = P["embedding.weight"]
    user_emb, item_emb = F.embedding(user_reviews, emb), F.embedding(item_reviews, emb)
    vu, vi = M.batch_valid(batch)
    rr = review_net(user_emb, item_emb, u_len, i_len, P, (vu, vi) if mask_padding else None, unsort_gru, aten)
    w, b = P["linear_fusion.0.weight"], P["linear_fusion.0.bias"]
    if review_net_only:
        pred = F.relu(F.linear(rr, w, b)).squeeze(-1)
        return pred, F.mse_loss(pred, labels, reduction="mean")
    B, S, L = user_reviews.shape
    valid = (batch_valid_ui(batch), vu.reshape(B * S, L), vi.reshape(B * S, L)) if mask_control else None
    c_u, c_i, pp, pn, kc = control_net(user_emb, item_emb, F.embedding(ui_reviews, emb), u_len, i_len, ui_len, P, threshold, valid,
                                       unsort_gru, aten)
    pos_match, neg_match, final_pos, final_neg, img = R.visual_net(photos, c_u, c_i, P, False, None, vgg_fn)
    pred = F.relu(F.linear(torch.cat([rr, final_pos, final_neg], dim=-1), w, b)).squeeze(-1)
    loss_r = F.mse_loss(pred, labels, reduction="mean")
    loss_v = torch.mean(pp.transpose(-1, -2) @ pos_match + pn.transpose(-1, -2) @ neg_match)
    if keep is not None:
        keep.update(review_repr=rr, c_u=c_u, c_i=c_i, prefer_pos=pp, prefer_neg=pn, final_pos=final_pos, final_neg=final_neg,
                    loss_r=loss_r, loss_v=loss_v, **kc)
    return pred, loss_r + loss_v * loss_v_rate


def invariance_batch(seed, vocab=900, V=1, full=True):
    """(alone, batch): one sample padded to its own size, and the same sample as row 0 of a batch of 4 whose other samples have MORE
    and LONGER sentences on all three review inputs, so that S, L, S_ui and L_ui all grow and the descending length sort moves row
    0's sentences to later ranks - what masked_attention_reference.invariance_batch had to avoid.  Photos are one seeded
    3 x 224 x 224 image per (sample, view); full=False leaves them out (UMPR-R)."""
    g = torch.Generator().manual_seed(seed)
    tok = lambda n: torch.randint(3, vocab, (n,), generator=g)
    own = {"u": (5, 3, 4), "i": (2, 6, 3, 4), "ui": (4, 2)}
    grow = {"u": (5, 9), "i": (6, 10), "ui": (3, 8)}               # batch-mates: (least sentence count, longest sentence)
    rows = {}
    for k in ("u", "i", "ui"):
        rows[k] = [[tok(n) for n in own[k]]]
        for _ in range(3):
            count = int(torch.randint(grow[k][0], grow[k][0] + 2, (1,), generator=g))
            lens = torch.randint(1, grow[k][1] + 1, (count,), generator=g)
            lens[0] = grow[k][1]
            rows[k].append([tok(int(n)) for n in lens])

    def pad(rr_, S_, L_):
        ids, lengths = torch.zeros(len(rr_), S_, L_, dtype=torch.int64), torch.ones(len(rr_), S_, dtype=torch.int64)
        for b_, ss in enumerate(rr_):
            for s_, t in enumerate(ss):
                ids[b_, s_, :len(t)] = t
                lengths[b_, s_] = len(t)
        return ids, lengths

    labels = torch.randint(1, 6, (4,), generator=g).float()
    photos = torch.rand(4, V, 1, 3, 224, 224, generator=g) if full else torch.zeros(0)
    out = []
    for n in (1, 4):
        part = {k: rows[k][:n] for k in rows}
        S_ = max(len(ss) for k in ("u", "i") for ss in part[k])
        L_ = max(len(t) for k in ("u", "i") for ss in part[k] for t in ss)
        S_ui, L_ui = max(len(ss) for ss in part["ui"]), max(len(t) for ss in part["ui"] for t in ss)
        (u, ul), (i, il), (ui, uil) = pad(part["u"], S_, L_), pad(part["i"], S_, L_), pad(part["ui"], S_ui, L_ui)
        out.append((u, i, ui, ul, il, uil, photos[:n] if full else photos, labels[:n]))
    return out[0], out[1]


def constructed_batch(seed, vocab=900, V=1, own=((9, 8, 7), (10, 6, 5, 4), (6, 4)), S=6, L=13, S_ui=4, L_ui=9, mates=3):
    """(alone, batch) for the full model under the REFERENCE's GRU permutation, i.e. without --unsort_gru: one sample padded to its own size (S0 = 4, L0 = 10, S_ui0 = 2, L_ui0 = 6 with the defaults),
    and the same sample as row 0 of a batch of 1 + `mates` padded to S x L and S_ui x L_ui, on all three review inputs.
    masked_attention_reference.invariance_batch says why the batch has to be built: the reference's ImprovedRnn hands row n the
    states of the sentence at n's rank in the descending sort of the batch's lengths, so a sample keeps its own states only while
    its real sentences are the batch's longest, in strictly descending lengths.  The batch-mates therefore have MORE sentences,
    each shorter than every one of sample 0's on that input, and the larger L / L_ui is padding width.  Row 0's padded sentences
    (length 1) do receive other sentences' states in the batch - live states behind an all-invalid mask, which is what the
    ControlNet's mask has to ignore.  Photos: one seeded 3 x 224 x 224 image per (sample, view)."""
    g = torch.Generator().manual_seed(seed)
    tok = lambda n: torch.randint(3, vocab, (n,), generator=g)

    def side(own_lens, S_):
        rows = [[tok(n) for n in own_lens]]
        for _ in range(mates):
            count = int(torch.randint(len(own_lens) + 1, S_ + 1, (1,), generator=g))
            rows.append([tok(int(torch.randint(1, min(own_lens), (1,), generator=g))) for _ in range(count)])
        return rows

    def pad(rows, S_, L_):
        ids, lengths = torch.zeros(len(rows), S_, L_, dtype=torch.int64), torch.ones(len(rows), S_, dtype=torch.int64)
        for b_, ss in enumerate(rows):
            for s_, t in enumerate(ss):
                ids[b_, s_, :len(t)] = t
                lengths[b_, s_] = len(t)
        return ids, lengths

    u, i, ui = side(own[0], S), side(own[1], S), side(own[2], S_ui)
    labels = torch.randint(1, 6, (1 + mates,), generator=g).float()
    photos = torch.rand(1 + mates, V, 1, 3, 224, 224, generator=g)
    S0, L0 = max(len(own[0]), len(own[1])), max(own[0] + own[1])
    out = []
    for n, (S_, L_, Su_, Lu_) in ((1, (S0, L0, len(own[2]), max(own[2]))), (1 + mates, (S, L, S_ui, L_ui))):
        (a, al), (b, bl), (c, cl) = pad(u[:n], S_, L_), pad(i[:n], S_, L_), pad(ui[:n], Su_, Lu_)
        out.append((a, b, c, al, bl, cl, photos[:n], labels[:n]))
    return out[0], out[1]
