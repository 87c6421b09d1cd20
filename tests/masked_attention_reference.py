"""Key-padding mask of the ReviewNet's softmaxes, restated on the CPU (test helper, not a test module).

`--mask_padding True` (umpr_token_mask, umpr_coattention_fwd_masked, umpr_snet_fwd_masked, umpr_review_net_fwd_masked) changes
three softmaxes of the reference; the definition the kernels are held to is written out here with torch, so that autograd
differentiates it, in whatever dtype the inputs have:

  token validity   valid[n][l] = l < min(max(len[n], 0), L) and ids[n][l] != pad_id                        (token_valid)
  co-attention     colmax[k] = max over VALID j of A[j, k], defined when k is valid and some j is; soft_u = softmax of colmax
                   over the defined k and +0.0 elsewhere; a sample without a defined k has soft_u = 0 and atte_u = 0.  Rows
                   alike.                                                                                     (coattention)
  S-Net            P[s][l] = softmax of the word scores over the valid l of sentence s, +0.0 elsewhere; a sentence without a
                   valid token has P = 0 and self_atte = 0; wsum and senti keep their formulas.                       (s_net)

With an all-valid mask every function performs the operations of oracle/umpr_ref.py in the same order and returns the same
bits (tests/test_masked_attention_reference.py), and the compaction identity of that test pins the definition without
trusting this file: at the valid positions the masked result equals the reference's formulas on the inputs with the masked
positions removed.  coattention_backward64 and snet_backward64 are hand-written float64 backwards with the argmax decisions
given, the counterparts of coattn_decisions.backward64 with the -1 / +0.0 conventions for undefined positions.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import umpr_ref as R

PAD_ID = 0


def token_valid(ids, lengths, pad_id=PAD_ID):
    """bool [N][L] from ids [N][L] and lengths [N] (numpy or torch in, numpy out)"""
    ids, lengths = np.asarray(ids), np.asarray(lengths).reshape(-1)
    N, L = ids.shape
    n = np.minimum(np.maximum(lengths.astype(np.int64), 0), L)
    return (np.arange(L)[None, :] < n[:, None]) & (ids != pad_id)


def _masked_softmax(x, ok):
    """softmax of x over the last axis restricted to `ok`; +0.0 outside, and all zero where no position is ok.  Neither a -inf
    minus -inf nor a 0 / 0 is formed, in the forward or in autograd's backward."""
    some = ok.any(-1, keepdim=True)
    x = torch.where(some, x.masked_fill(~ok, float("-inf")), torch.zeros_like(x))
    return torch.where(ok, torch.softmax(x, dim=-1), torch.zeros_like(x))


def coattention(gru_u, gru_i, M, vu, vi, keep=None):
    """oracle r_net lines model.py:50-55 with validity vu [B][SL] (user positions, columns k) and vi (item positions, rows j)."""
    A = torch.tanh(gru_i @ M @ gru_u.transpose(-1, -2))                         # [B][j][k]
    pair = vi.unsqueeze(-1) & vu.unsqueeze(-2)
    Am = A.masked_fill(~pair, float("-inf"))
    col, row = torch.max(Am, dim=-2), torch.max(Am, dim=-1)
    def_u, def_i = vu & vi.any(-1, keepdim=True), vi & vu.any(-1, keepdim=True)
    soft_u, soft_i = _masked_softmax(col.values, def_u), _masked_softmax(row.values, def_i)
    atte_u = (gru_u.transpose(-1, -2) @ soft_u.unsqueeze(-1)).squeeze(-1)
    atte_i = (gru_i.transpose(-1, -2) @ soft_i.unsqueeze(-1)).squeeze(-1)
    if keep is not None:
        zero = torch.zeros_like(col.values)
        keep.update(A=A, colmax=torch.where(def_u, col.values, zero), rowmax=torch.where(def_i, row.values, zero),
                    argcol=torch.where(def_u, col.indices, torch.full_like(col.indices, -1)),
                    argrow=torch.where(def_i, row.indices, torch.full_like(row.indices, -1)))
    return soft_u, soft_i, atte_u, atte_i


def r_net(user_emb, item_emb, u_lengths, i_lengths, P, vu, vi, prefix="review_net.r_net.", aten=False):
    """oracle r_net with the mask; vu, vi bool [B][S*L]"""
    B, S, L, E = user_emb.shape
    gru_u = R.improved_rnn(user_emb.reshape(B * S, L, E), u_lengths.reshape(-1), P, prefix + "gru.module.", aten)
    gru_i = R.improved_rnn(item_emb.reshape(B * S, L, E), i_lengths.reshape(-1), P, prefix + "gru.module.", aten)
    gru_u = gru_u.reshape(B, S * L, -1)
    gru_i = gru_i.reshape(B, S * L, -1)
    return (gru_u, gru_i) + coattention(gru_u, gru_i, P[prefix + "M"], vu, vi)


def s_net(gru_repr, word_soft, sent_length, P, prefix, valid, keep=None):
    """oracle s_net with valid bool [B][S*L] (or [B*S][L])"""
    B = gru_repr.shape[0]
    S = gru_repr.shape[1] // sent_length
    X = gru_repr.reshape(B * S, sent_length, -1).transpose(-1, -2)             # [BS, 2u, L]
    scores = P[prefix + "Ws"] @ torch.tanh(P[prefix + "Ms"] @ X)               # [BS, 1, L]
    sent_soft = _masked_softmax(scores, valid.reshape(B * S, 1, sent_length))
    self_atte = X @ sent_soft.transpose(-1, -2)                                 # [BS, 2u, 1]
    senti = word_soft.reshape(B * S, -1).sum(dim=-1, keepdim=True) * self_atte.squeeze(-1)
    senti = senti.view(B, S, -1).sum(dim=-2)
    if keep is not None:
        keep.update(P=sent_soft.reshape(B, S, sent_length))
    return self_atte.view(B, S, -1), senti


def review_net(user_emb, item_emb, u_lengths, i_lengths, P, vu, vi, aten=False, keep=None):
    """oracle review_net with the mask"""
    pre = "review_net."
    L = user_emb.shape[-2]
    gru_u, gru_i, soft_u, soft_i, atte_u, atte_i = r_net(user_emb, item_emb, u_lengths, i_lengths, P, vu, vi, pre + "r_net.", aten)
    _, senti_u = s_net(gru_u, soft_u, L, P, pre + "s_net_u.", vu)
    _, senti_i = s_net(gru_i, soft_i, L, P, pre + "s_net_i.", vi)
    repr_u = torch.cat([atte_u, senti_u], dim=-1)
    repr_i = torch.cat([atte_i, senti_i], dim=-1)
    out = torch.tanh(F.linear(repr_u, P[pre + "linear_u.weight"]) + F.linear(repr_i, P[pre + "linear_i.weight"]))
    if keep is not None:
        keep.update(gru_u=gru_u, gru_i=gru_i, soft_u=soft_u, soft_i=soft_i, atte_u=atte_u, atte_i=atte_i, senti_u=senti_u,
                    senti_i=senti_i, review_repr=out)
    return out


def batch_valid(batch, pad_id=PAD_ID):
    """(vu, vi) bool [B][S*L] of a batch tuple (user_reviews, item_reviews, ui_reviews, u_len, i_len, ...)"""
    user_reviews, item_reviews, _, u_len, i_len = batch[:5]
    B, S, L = user_reviews.shape
    vu = torch.from_numpy(token_valid(user_reviews.reshape(B * S, L).numpy(), u_len.reshape(-1).numpy(), pad_id)).reshape(B, S * L)
    vi = torch.from_numpy(token_valid(item_reviews.reshape(B * S, L).numpy(), i_len.reshape(-1).numpy(), pad_id)).reshape(B, S * L)
    return vu, vi


def umpr_r_forward(P, batch, mask=True, aten=False, keep=None):
    """UMPR-R (oracle umpr_forward(review_net_only=True)) with the masked ReviewNet; mask=False is the oracle itself"""
    if not mask:
        return R.umpr_forward(P, batch, review_net_only=True, aten=aten, keep=keep)
    user_reviews, item_reviews, _, u_len, i_len, _, _, labels = batch
    emb = P["embedding.weight"]
    vu, vi = batch_valid(batch)
    rr = review_net(F.embedding(user_reviews, emb), F.embedding(item_reviews, emb), u_len, i_len, P, vu, vi, aten, keep)
    pred = F.relu(F.linear(rr, P["linear_fusion.0.weight"], P["linear_fusion.0.bias"])).squeeze(-1)
    return pred, F.mse_loss(pred, labels, reduction="mean")


def invariance_batch(seed, vocab=900, lens_u=(9, 8, 7), lens_i=(10, 6, 5, 4), S=6, L=13, mates=3):
    """(alone, batch): one UMPR-R sample padded to its own size (S0 = 4, L0 = 10 with the defaults), and the same sample as row 0
    of a batch of 1 + `mates` padded to S x L, whose other samples have up to S sentences.
    The reference's ImprovedRnn hands row n the GRU states of the sentence that stands at n's rank in the descending sort of
    the batch's lengths (SURVEY.md header fact 1), across samples: whatever the mask, a sample keeps its own states only while
    its real sentences are the batch's longest, strictly, in distinct lengths.  So the batch-mates' sentences are shorter than
    every one of sample 0's (they force the larger S), and the larger L is padding width: no sentence may be longer than sample
    0's longest without changing the states sample 0 is handed."""
    g = torch.Generator().manual_seed(seed)
    tok = lambda n: torch.randint(3, vocab, (n,), generator=g)
    shortest = min(lens_u + lens_i)

    def side(own):
        rows = [[tok(n) for n in own]]
        for _ in range(mates):
            count = int(torch.randint(len(own) + 1, S + 1, (1,), generator=g))
            rows.append([tok(int(torch.randint(1, shortest, (1,), generator=g))) for _ in range(count)])
        return rows

    def pad(rows, S_, L_):
        ids, lengths = torch.zeros(len(rows), S_, L_, dtype=torch.int64), torch.ones(len(rows), S_, dtype=torch.int64)
        for b, ss in enumerate(rows):
            for s, t in enumerate(ss):
                ids[b, s, :len(t)] = t
                lengths[b, s] = len(t)
        return ids, lengths

    u, i = side(lens_u), side(lens_i)
    labels = torch.randint(1, 6, (1 + mates,), generator=g).float()
    S0, L0 = max(len(lens_u), len(lens_i)), max(lens_u + lens_i)
    out = []
    for rows_u, rows_i, S_, L_, lab in ((u[:1], i[:1], S0, L0, labels[:1]), (u, i, S, L, labels)):
        (ui, ul), (ii, il) = pad(rows_u, S_, L_), pad(rows_i, S_, L_)
        n = len(rows_u)
        out.append((ui, ii, torch.zeros(n, 1, 1, dtype=torch.int64), ul, il, torch.ones(n, 1, dtype=torch.int64), torch.zeros(0), lab))
    return out[0], out[1]


# ---- hand-written float64 backwards with the decisions given ---------------------------------------------------------------
def coattention_backward64(Gu, Gi, M, argcol, argrow, d_atte_u, d_atte_i, d_soft_u=None, d_soft_i=None, dtype=torch.float64):
    """(dGu, dGi, dM) of the masked co-attention with the saved decisions: argcol / argrow [B][SL] with -1 at undefined
    positions (those get soft = 0, take no gradient and are nobody's partner).  The maxima are read at the decisions:
        cm[k] = A[argcol[k], k]        soft_u = softmax of cm over the defined k        ds_u[k] = d_soft_u[k] + Gu[k] . d_atte_u
        dS_col[k] = soft_u[k] (ds_u[k] - sum soft_u ds_u) (1 - cm[k]^2)                                 (0 at undefined k)
        dGu[k] = soft_u[k] d_atte_u + dS_col[k] T[argcol[k]] + sum_{j: argrow[j] = k} dS_row[j] T[j]
        dT[j]  = dS_row[j] Gu[argrow[j]] + sum_{k: argcol[k] = j} dS_col[k] Gu[k]
        dGi    = soft_i (x) d_atte_i + dT M^T          dM = Gi^T dT"""
    Gu, Gi, M = Gu.to(dtype), Gi.to(dtype), M.to(dtype)
    dau, dai = d_atte_u.to(dtype), d_atte_i.to(dtype)
    T = Gi @ M
    A = torch.tanh(T @ Gu.transpose(-1, -2))
    ac, ar = argcol.long(), argrow.long()
    du, di = ac >= 0, ar >= 0
    acc, arc = ac.clamp(min=0), ar.clamp(min=0)
    cm = torch.where(du, A.gather(1, acc.unsqueeze(1)).squeeze(1), torch.zeros((), dtype=dtype))
    rm = torch.where(di, A.gather(2, arc.unsqueeze(2)).squeeze(2), torch.zeros((), dtype=dtype))
    soft_u, soft_i = _masked_softmax(cm, du), _masked_softmax(rm, di)
    ds_u = (Gu @ dau.unsqueeze(-1)).squeeze(-1)
    ds_i = (Gi @ dai.unsqueeze(-1)).squeeze(-1)
    if d_soft_u is not None:
        ds_u = ds_u + d_soft_u.to(dtype)
    if d_soft_i is not None:
        ds_i = ds_i + d_soft_i.to(dtype)
    dS_col = soft_u * (ds_u - (soft_u * ds_u).sum(-1, keepdim=True)) * (1 - cm * cm)     # soft = 0 at undefined: exactly 0
    dS_row = soft_i * (ds_i - (soft_i * ds_i).sum(-1, keepdim=True)) * (1 - rm * rm)
    Dm = Gu.shape[-1]
    ace, are = acc.unsqueeze(-1).expand(-1, -1, Dm), arc.unsqueeze(-1).expand(-1, -1, Dm)
    dGu = soft_u.unsqueeze(-1) * dau.unsqueeze(1) + dS_col.unsqueeze(-1) * T.gather(1, ace)
    dGu.scatter_add_(1, are, dS_row.unsqueeze(-1) * T)       # undefined rows add an exact zero to position 0
    dT = dS_row.unsqueeze(-1) * Gu.gather(1, are)
    dT.scatter_add_(1, ace, dS_col.unsqueeze(-1) * Gu)
    dGi = soft_i.unsqueeze(-1) * dai.unsqueeze(1) + dT @ M.t()
    dM = torch.einsum("bjc,bjd->cd", Gi, dT)
    return dGu, dGi, dM


def snet_forward(X, Ms, Ws, word_soft, valid, dtype=torch.float64):
    """X [B][S][L][D], Ms [AT][D], Ws [AT], word_soft [B][S][wl], valid bool [B][S][L] -> dict(U, P, wsum, self_atte, senti)"""
    X, Ms, Ws, word_soft = X.to(dtype), Ms.to(dtype), Ws.to(dtype), word_soft.to(dtype)
    U = torch.tanh(X @ Ms.t())
    P = _masked_softmax(U @ Ws, valid)
    sa = (P.unsqueeze(-1) * X).sum(-2)
    wsum = word_soft.sum(-1)
    return dict(U=U, P=P, wsum=wsum, self_atte=sa, senti=(wsum.unsqueeze(-1) * sa).sum(1))


def snet_backward64(X, Ms, Ws, word_soft, valid, d_senti, d_self_atte=None, dtype=torch.float64):
    """(dX, dMs, dWs, d_word_soft) of snet_forward's (senti, self_atte) by hand:
        g[s] = wsum[s] d_senti (+ d_self_atte[s])      dp[l] = X[l] . g      de = P (dp - sum P dp)           (0 at masked l)
        dPre[l] = Ws de[l] (1 - U[l]^2)      dX[l] = P[l] g + dPre[l] Ms      dMs = dPre^T X      dWs = sum de[l] U[l]
        d_word_soft[s][:] = self_atte[s] . d_senti"""
    f = snet_forward(X, Ms, Ws, word_soft, valid, dtype)
    X, Ms, Ws, ds = X.to(dtype), Ms.to(dtype), Ws.to(dtype), d_senti.to(dtype)
    g = f["wsum"].unsqueeze(-1) * ds.unsqueeze(1)
    if d_self_atte is not None:
        g = g + d_self_atte.to(dtype)
    dp = (X * g.unsqueeze(-2)).sum(-1)
    de = f["P"] * (dp - (f["P"] * dp).sum(-1, keepdim=True))
    dPre = de.unsqueeze(-1) * Ws * (1 - f["U"] ** 2)
    dX = f["P"].unsqueeze(-1) * g.unsqueeze(-2) + dPre @ Ms
    dMs = torch.einsum("bsla,bsld->ad", dPre, X)
    dWs = (de.unsqueeze(-1) * f["U"]).sum((0, 1, 2))
    d_word_soft = (f["self_atte"] * ds.unsqueeze(1)).sum(-1, keepdim=True).expand_as(word_soft).clone()
    return dX, dMs, dWs, d_word_soft
