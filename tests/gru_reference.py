"""Float64 reference of the embedding + bidirectional GRU (test helper, not a test module; CPU only).

umpr_amd/csrc/gru.hip (gru_fwd16_kernel / gru_bwd16_kernel) and the GRU block of umpr_amd/csrc/api.hip take no discrete
decision: out, the gate records and all eight parameter gradients are smooth functions of the inputs.  The functions here
  * build the seeded inputs of the GPU tests with the length patterns at which a 16-sequence tile can go wrong (make_case),
  * run the recurrence as an explicit time loop per direction in float64 - or, for the yardstick, in float32 - and keep the
    gate records r, z, n, W_hn h + b_hn of every step (forward64),
  * run a hand-written backward through time over those records (backward64: no autograd, a second statement of the
    formulas next to oracle/umpr_ref.py), and
  * reuse the gate of tests/coattn_decisions.py: a HIP tensor may be K x as far from float64 as the float32 CPU evaluation of
    the same formula is.  Where the float64 reference is identically zero (dW_hh when no sequence has a second step: h_prev
    is 0 everywhere) C.distances demands an exactly zero HIP tensor instead.
tests/test_gru_reference.py checks them against autograd and nn.GRU on the CPU; tests/test_gpu_gru.py uses them on the GPU.
Layout: out [N][L][2H] (forward direction in columns 0..H-1) and gates [2][N][L][4][H], both indexed by INPUT row - the
permutation to output rows (`dst_row` of the C ABI) is the caller's; dgx [N][L][6H] = the gradient of the input projections,
forward direction first.  H = 64 in every kernel; the reference takes it from w_hh (the toy fixture has H = 4).
"""
from types import SimpleNamespace

import torch
import torch.nn.functional as F

from coattn_decisions import FLOOR, K_MAX, K_START, distances, gate   # noqa: F401  (shared, not copied)

H = 64                      # config.gru_size, the only width the kernels are built for
TILE = 16                   # sequences per workgroup of the default kernels (TS2 of gru.hip)
VOCAB = 200
# The factor the GPU tests use.  Worst measured ratio of a HIP distance to the floored float32 CPU distance:
# see profiles/r04_g_gru_gates.txt - 2.78 (dW_hh of the forward direction at (20, 70, 8): one float32 accumulator chain per
# element over 70 steps x 16 sequences, where the CPU sums step by step in blocks), 2.03 on the gate records, below 1.7 on
# everything else: K stays at its starting value.
K = K_START
# (N, L, E, kind) of the GPU tests: the smallest at which each mechanism of the 16-sequence tiles, the Ep = E rounded up to 4
# pitch and the split-K dW_ih product can fail (one sequence / one step / E = 1; a single partial tile; exactly one tile; a
# second tile of one sequence with zero lengths; every length 1; tiles of mixed and of all-1 lengths; fifteen idle rows beside
# one long one; lengths above L; sentences longer than a wave; GloVe-300d)
CASES = ((1, 1, 1, "full"), (15, 5, 3, "rand"), (16, 7, 4, "full"), (17, 6, 7, "zeros"), (32, 4, 5, "ones"),
         (33, 9, 50, "tail1"), (16, 12, 8, "one_long"), (48, 20, 52, "over"), (20, 70, 8, "rand"), (65, 12, 300, "rand"))
KINDS = ("full", "rand", "ones", "tail1", "one_long", "zeros", "over")
PARAMS = ("w_ih", "w_hh", "b_ih", "b_hh")
GRADS = tuple("d" + n + s for s in ("_f", "_r") for n in PARAMS)       # the order of the C ABI's eight gradient pointers
WRONG_FWD = ("bhn_outside", "reverse_from_L", "reset_at_length_change")
WRONG_BWD = ("hprev_own_output",)


def make_lengths(N, L, kind, g):
    """full: L.  rand: uniform in 1..L with row 0 = L (as _gru_case of test_gpu_parity).  ones: 1.  tail1: rand, second half
    (rows N//2 ..) all 1.  one_long: row 5 (0 if N < 6) = L, the rest 1.  zeros: rand with every fifth length 0, row 0
    among them.  over: rand with every fourth length L + 3, row 0 among them."""
    assert kind in KINDS, kind
    rand = torch.randint(1, L + 1, (N,), generator=g)
    rand[0] = L
    if kind == "full":
        return torch.full((N,), L, dtype=torch.int64)
    if kind == "ones":
        return torch.ones(N, dtype=torch.int64)
    if kind == "one_long":
        lengths = torch.ones(N, dtype=torch.int64)
        lengths[5 if N > 5 else 0] = L
        return lengths
    if kind == "tail1":
        rand[N // 2:] = 1
    elif kind == "zeros":
        rand[::5] = 0
    elif kind == "over":
        rand[::4] = L + 3
    return rand


def make_case(N, L, E, kind, seed=None):
    """The seeded inputs of one case: emb [200][E] = 0.4 randn with rows 0..2 zero, the eight nn.GRU parameters uniform in
    +-1/8, ids in 3..199 with 0 at and past each length, dout [N][L][128] = randn (indexed by input row, like out)."""
    g = torch.Generator().manual_seed(100000 * N + 1000 * L + E if seed is None else seed)
    emb = torch.randn(VOCAB, E, generator=g) * 0.4
    emb[:3] = 0
    lengths = make_lengths(N, L, kind, g)
    ids = torch.randint(3, VOCAB, (N, L), generator=g)
    ids[torch.arange(L).unsqueeze(0) >= lengths.unsqueeze(1)] = 0
    w = [(torch.rand(shape, generator=g) * 2 - 1) / 8 for _ in range(2) for shape in ((3 * H, E), (3 * H, H), (3 * H,), (3 * H,))]
    dout = torch.randn(N, L, 2 * H, generator=g)
    return SimpleNamespace(N=N, L=L, E=E, kind=kind, emb=emb, ids=ids, lengths=lengths, w=w, dout=dout,
                           x=F.embedding(ids, emb), tag=f"N{N} L{L} E{E} {kind}")


def case_of(x, lengths, w):
    """a case from already embedded inputs x [N][L][E] (the golden fixtures)"""
    N, L, E = x.shape
    return SimpleNamespace(N=N, L=L, E=E, kind="given", lengths=lengths.long(), w=list(w), x=x, tag=f"N{N} L{L} E{E} given")


def clamped(case):
    """min(max(len, 0), L): what the kernels and the reference treat a length as"""
    return case.lengths.clamp(0, case.L)


def valid(case):
    """[N][L] bool: t < min(len, L), the positions at which out is a GRU state and the gate records are defined"""
    return torch.arange(case.L).unsqueeze(0) < clamped(case).unsqueeze(1)


def sorted_order(case):
    """sorted_indices of pack_padded_sequence(enforce_sorted=False): the descending, non-stable torch.sort of the lengths"""
    return torch.sort(case.lengths, descending=True)[1]


def _direction(x, lens, w_ih, w_hh, b_ih, b_hh, reverse, wrong, order):
    N, L, _ = x.shape
    Hh = w_hh.shape[1]
    gx = x @ w_ih.t() + b_ih                                  # [N][L][3H], gate order r, z, n
    h = x.new_zeros(N, Hh)
    out = x.new_zeros(N, L, Hh)
    gates = x.new_zeros(N, L, 4, Hh)
    Wr, Wz, Wn = w_hh[:Hh], w_hh[Hh:2 * Hh], w_hh[2 * Hh:]
    br, bz, bn = b_hh[:Hh], b_hh[Hh:2 * Hh], b_hh[2 * Hh:]
    if wrong == "reset_at_length_change":
        tile_of = torch.empty(N, dtype=torch.int64)
        tile_of[order] = torch.arange(N) // TILE              # the tile each input row sits in
    for t in (range(L - 1, -1, -1) if reverse else range(L)):
        act = (lens > t).unsqueeze(1)
        if wrong == "reset_at_length_change" and not reverse and t > 0:
            # WRONG on purpose: a sequence that ended at t takes the state of its tile's running sequences with it
            ended = torch.zeros(N // TILE + 1, dtype=torch.bool)
            ended[tile_of[lens == t]] = True
            h = torch.where(ended[tile_of].unsqueeze(1), torch.zeros_like(h), h)
        r = torch.sigmoid(gx[:, t, :Hh] + h @ Wr.t() + br)
        z = torch.sigmoid(gx[:, t, Hh:2 * Hh] + h @ Wz.t() + bz)
        if wrong == "bhn_outside":                            # WRONG on purpose: b_hn outside r * (.)
            hn = h @ Wn.t()
            n = torch.tanh(gx[:, t, 2 * Hh:] + r * hn + bn)
        else:
            hn = h @ Wn.t() + bn
            n = torch.tanh(gx[:, t, 2 * Hh:] + r * hn)
        h_new = (1 - z) * n + z * h
        # WRONG on purpose (reverse_from_L): the reverse direction runs through the padding before the sentence's last token
        runs = torch.ones_like(act) if (wrong == "reverse_from_L" and reverse) else act
        h = torch.where(runs, h_new, h)
        out[:, t] = torch.where(act, h_new, torch.zeros_like(h_new))
        gates[:, t] = torch.where(act.unsqueeze(1), torch.stack([r, z, n, hn], 1), torch.zeros_like(gates[:, t]))
    return out, gates


def forward64(case, dtype=torch.float64, wrong=None):
    """(out [N][L][2H], gates [2][N][L][4][H]) in `dtype` (float64: the reference; float32: the yardstick), rows in input
    order.  Per direction, h_0 = 0 and for t < min(len, L), forward direction t ascending, reverse direction from
    t = min(len, L) - 1 descending:
        r = sigmoid(W_ir x + b_ir + W_hr h + b_hr)      z = sigmoid(W_iz x + b_iz + W_hz h + b_hz)
        hn = W_hn h + b_hn                              n = tanh(W_in x + b_in + r hn)          h' = (1 - z) n + z h
    out and gates are zero at t >= min(len, L).  `wrong` names one of WRONG_FWD: a deliberately wrong variant, for the
    tests that show the gate rejects it."""
    assert wrong is None or wrong in WRONG_FWD, wrong
    x, lens = case.x.to(dtype), clamped(case)
    w = [p.to(dtype) for p in case.w]
    order = sorted_order(case)
    of, gf = _direction(x, lens, *w[:4], False, wrong, order)
    orv, gr = _direction(x, lens, *w[4:], True, wrong, order)
    return torch.cat([of, orv], -1), torch.stack([gf, gr])


def backward64(case, fwd, dout, dtype=torch.float64, wrong=None):
    """The eight parameter gradients (a dict in GRADS order) and dgx [N][L][6H] of sum(out * dout), by hand, in `dtype`, over
    the (out, gates) of forward64 in the same dtype.  Per direction, against the forward's order, dh = 0 at the start:
        dtot = dh + dout[t]              h_prev = out[t -+ 1] (0 at the sequence's first step)
        dn' = dtot (1 - z)(1 - n^2)      dz' = dtot (h_prev - n) z (1 - z)      dr' = dn' hn r (1 - r)
        dgx[t] = (dr', dz', dn')         dgh = (dr', dz', dn' r)                dh = dtot z + dgh W_hh
        dW_hh += dgh^T h_prev            db_hh += dgh       db_ih += dgx[t]     dW_ih += dgx[t]^T x[t]
    Nothing at t >= min(len, L) contributes.  `wrong` = "hprev_own_output" reads h_prev from the step's own output."""
    assert wrong is None or wrong in WRONG_BWD, wrong
    out, gates = fwd
    assert out.dtype == dtype and gates.dtype == dtype, (out.dtype, gates.dtype, dtype)
    x, lens, dout = case.x.to(dtype), clamped(case), dout.to(dtype)
    N, L, _ = x.shape
    grads, dgx_dirs = {}, []
    for d, suf in enumerate(("_f", "_r")):
        w_hh = case.w[4 * d + 1].to(dtype)
        Hh = w_hh.shape[1]
        o, do = out[..., d * Hh:(d + 1) * Hh], dout[..., d * Hh:(d + 1) * Hh]
        dh = x.new_zeros(N, Hh)
        dgx = x.new_zeros(N, L, 3 * Hh)
        dW_hh = x.new_zeros(3 * Hh, Hh)
        db_hh = x.new_zeros(3 * Hh)
        for t in (range(L - 1, -1, -1) if d == 0 else range(L)):
            tp = t - 1 if d == 0 else t + 1
            act = (lens > t).unsqueeze(1)
            if wrong == "hprev_own_output":
                hp = o[:, t]
            elif 0 <= tp < L:
                hp = torch.where((lens > tp).unsqueeze(1), o[:, tp], torch.zeros_like(dh))
            else:
                hp = torch.zeros_like(dh)
            r, z, n, hn = gates[d, :, t].unbind(1)
            dtot = dh + do[:, t]
            dn = dtot * (1 - z) * (1 - n * n)
            dz = dtot * (hp - n) * z * (1 - z)
            dr = dn * hn * r * (1 - r)
            zero = torch.zeros_like(dn)
            dgx_t = torch.where(act, torch.cat([dr, dz, dn], 1), torch.cat([zero, zero, zero], 1))
            dgh = torch.where(act, torch.cat([dr, dz, dn * r], 1), torch.cat([zero, zero, zero], 1))
            dgx[:, t] = dgx_t
            dW_hh += dgh.t() @ hp
            db_hh += dgh.sum(0)
            dh = torch.where(act, dtot * z + dgh @ w_hh, dh)
        grads["dw_ih" + suf] = torch.einsum("ntg,nte->ge", dgx, x)
        grads["dw_hh" + suf] = dW_hh
        grads["db_ih" + suf] = dgx.sum((0, 1))
        grads["db_hh" + suf] = db_hh
        dgx_dirs.append(dgx)
    return {k: grads[k] for k in GRADS}, torch.cat(dgx_dirs, -1)


def reference(case, dtype=torch.float64, dout=None, wrong_fwd=None, wrong_bwd=None):
    """forward64 and backward64 of one case in `dtype`: a namespace with out, gates, grads (dict), dgx"""
    out, gates = forward64(case, dtype, wrong_fwd)
    grads, dgx = backward64(case, (out, gates), case.dout if dout is None else dout, dtype, wrong_bwd)
    return SimpleNamespace(out=out, gates=gates, grads=grads, dgx=dgx)


def whh_is_zero(case):
    """True where no sequence has a second step: h_prev = 0 at every step, so dW_hh of both directions is identically zero"""
    return int(clamped(case).max()) <= 1


def dropped_dout_element(case):
    """(n, t, column) of the one dout element the gate tests drop: the LAST sequence (the partial tile), its first step, the
    first reverse-direction unit whose upstream gradient is at least 0.5 in magnitude"""
    n = case.N - 1
    assert int(clamped(case)[n]) >= 1
    col = H + int(torch.nonzero(case.dout[n, 0, H:].abs() >= 0.5)[0])
    return n, 0, col


def gate_abs(got, ref, ref32, name, K=K, log=None, tag=""):
    """The gate for a tensor whose values are bounded by 1 (out): the largest absolute distance of `got` from the float64
    `ref` must be within K x that of `ref32`, floored at 2^-22.  Logged before it is judged; returns a row as C.gate does."""
    assert K <= K_MAX, K
    ref = ref.double()
    finite = bool(torch.isfinite(got).all())
    d = float((got.double().cpu() - ref).abs().max()) if finite else float("inf")
    r = float((ref32.double() - ref).abs().max())
    ratio = d / max(r, FLOOR)
    row = {"name": name, "d_max": d, "r_max": r, "ratio": ratio, "over": ratio / K, "ok": finite and ratio <= K}
    if log is not None:
        log(f"{tag} {name}: max_abs={d:.3e} | ref32 max_abs={r:.3e} | ratio={ratio:.2f} K={K:g} "
            f"ref_max={float(ref.abs().max()):.3e}{'' if row['ok'] else '  OUTSIDE'}")
    return row
