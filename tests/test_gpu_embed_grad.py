"""The trainable embedding table (`--train_embedding True`) on the GPU: umpr_embed_grad alone against the float64 scatter of
tests/embed_grad_reference.py, its determinism, the token gradient dx of umpr_embed_gru_bidir_bwd_dx against the float64 recurrence
of tests/gru_reference.py, the whole model against the oracle with a trainable `embedding.weight`, four Adam steps (with and
without clipping), the checkpoint round trip, and the default (frozen table) against the reference's fixtures.

Gate (the project's own, coattn_decisions.gate): a HIP tensor may be K = 4 x as far from float64 as the float32 CPU evaluation of
the same formula is, floor 2^-22; rows of the table no token names must be +0.0 to the bit.  Every output buffer is prefilled with
a NaN sentinel and followed by a guard band that must come back untouched; workspaces are NaN bytes with a guard band too.
"""
import ctypes
import os

import numpy as np
import pytest
import torch

import embed_grad_reference as EG
import gru_reference as G
from test_gpu_gru import _case, _g0, _i32, _nan, _ws
from test_gpu_parity import LOG as PARITY_LOG
from test_gpu_parity import L, check, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "embed_grad.log")
GUARD = 4096                       # floats behind d_emb / dx, bytes x 4 behind the workspace
SENTINEL = 0x7FC12345              # a NaN with a payload
VOCAB = 1000
H = G.H


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def _chunk(L):
    return int(L.fn["umpr_embed_grad_chunk"]())


def _sentinel(dev, n, off=0):
    """(int32 bits of off + n + GUARD sentinels, the float view of [off, off + n))"""
    bits = torch.full((off + n + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    return bits, bits.view(torch.float32)[off:off + n]


def _scatter(L, dev, sources, vocab, E, off=0, stream=None, n_src=None):
    """umpr_embed_grad on the device: sources [(ids int64 numpy, dx float32 numpy)].  d_emb is sentinel-filled (based `off` floats
    past the allocation) with a guard band; the workspace is exactly umpr_embed_grad_ws_bytes long, NaN bytes, with a guard band;
    sorted_pos comes from torch.sort(stable=True) on the device, as the model makes it.  Returns the table's int32 bits (CPU)."""
    ids = [torch.from_numpy(np.ascontiguousarray(i, dtype=np.int64)).to(dev) for i, _ in sources]
    dxs = [torch.from_numpy(np.ascontiguousarray(d, dtype=np.float32)).reshape(-1, E).to(dev) for _, d in sources]
    T = sum(int(i.numel()) for i in ids)
    pos = torch.sort(torch.cat(ids), stable=True).indices.to(torch.int32) if T else torch.zeros(1, dtype=torch.int32, device=dev)
    assert np.array_equal(pos.cpu().numpy()[:T], EG.sorted_positions([i for i, _ in sources]))
    bits, d_emb = _sentinel(dev, vocab * E, off)
    wsb = L.size("umpr_embed_grad_ws_bytes", T, E)
    ws = torch.full((wsb + 4 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    k = max(len(ids), 1)
    iarr = (ctypes.c_void_p * k)(*[t.data_ptr() for t in ids])
    darr = (ctypes.c_void_p * k)(*[t.data_ptr() for t in dxs])
    counts = (ctypes.c_long * k)(*[int(t.numel()) for t in ids])
    args = (ctypes.addressof(iarr), ctypes.addressof(darr), ctypes.addressof(counts), len(ids) if n_src is None else n_src, E, vocab,
            pos, d_emb, ws, wsb)
    if stream is None:
        L.call("umpr_embed_grad", *args, st())
    else:
        with torch.cuda.stream(stream):
            L.call("umpr_embed_grad", *args, stream.cuda_stream)
    torch.cuda.synchronize()
    assert bool((bits[:off] == SENTINEL).all()) and bool((bits[off + vocab * E:] == SENTINEL).all()), "written outside d_emb"
    assert bool((ws[wsb:] == 0xFF).all()), "written behind ws_bytes"
    return bits[off:off + vocab * E].cpu().view(vocab, E)


def _judge(tag, bits, sources, vocab, E):
    """the table under the gate against the float64 scatter, untouched rows +0.0 to the bit, nothing left of the sentinel"""
    got = bits.view(torch.float32)
    assert bool(torch.isfinite(got).all()), f"{tag}: a row was not written"
    ref = EG.scatter_reference(sources, vocab, E)
    ref32 = EG.scatter_reference(sources, vocab, E, np.float32)
    untouched = torch.from_numpy(~EG.touched_rows(sources, vocab))
    assert bool((bits[untouched] == 0).all()), f"{tag}: a row no token names is not +0.0"
    if not ref.any():
        assert bool((got == 0).all()), tag
        return
    ok, rows = EG.gate([got], [EG.as_tensor(ref)], [EG.as_tensor(ref32)], names=["d_emb"], K=EG.K, log=log, tag=tag)
    assert ok, (tag, rows)


def _make(pattern, T, E, vocab=VOCAB, seed=0):
    rng = np.random.default_rng(1000 * T + 10 * E + len(pattern) + seed)
    ids = EG.make_ids(pattern, T, vocab, rng)
    dx = rng.standard_normal((T, E)).astype(np.float32)
    return ids, dx


def _sizes(L):
    c = _chunk(L)
    return sorted({0, 1, 255, 256, 257, c - 1, c, c + 1, 2 * c, 2 * c + 77})


# ------------------------------------------------------------------------------------------------ umpr_embed_grad alone
@pytest.mark.parametrize("E", [1, 49, 50, 300])
@pytest.mark.parametrize("pattern", EG.PATTERNS)
def test_scatter_vs_float64(L, dev, pattern, E):
    """every T at which the kernels take another path (none, one position, both sides of 256 and of the window of
    umpr_embed_grad_chunk() sorted positions, beyond two windows)"""
    for T in _sizes(L):
        ids, dx = _make(pattern, T, E)
        src = [(ids, dx)]
        _judge(f"{pattern} T{T} E{E}", _scatter(L, dev, src, VOCAB, E), src, VOCAB, E)


def test_long_runs_at_every_offset(L, dev):
    """runs longer than a window (umpr_embed_grad_chunk() sorted positions) that start anywhere in one, end on and off a window
    edge and follow each other directly: the pieces of two runs must never share a workspace slot"""
    c = _chunk(L)
    for lens in ([c + 1, 3, 2 * c, 2 * c + 5, 1, c, c + 2], [5, 3 * c + 1, c + 1, c + 1, 7], [c - 1, c + 1, c + 1], [4 * c + 3]):
        ids = np.concatenate([np.full(n, 11 * k + (k % 2) * 500, dtype=np.int64) for k, n in enumerate(lens)])
        rng = np.random.default_rng(sum(lens))
        ids = ids[rng.permutation(ids.size)]                    # the sort brings the runs back together, in position order
        dx = rng.standard_normal((ids.size, 50)).astype(np.float32)
        for E in (50, 300):
            src = [(ids, np.ascontiguousarray(np.resize(dx, (ids.size, E))))]
            _judge(f"runs {lens} E{E}", _scatter(L, dev, src, VOCAB, E), src, VOCAB, E)


@pytest.mark.parametrize("counts", [(1,), (200, 389), (300, 0, 289), (0, 589), (17, 250, 1, 321), (589, 0, 0, 0)],
                         ids=lambda c: "-".join(map(str, c)))
def test_one_to_four_sources_of_unequal_length(L, dev, counts):
    T = sum(counts)
    ids, dx = _make("zipf", T, 50, seed=len(counts))
    src = EG.split_sources(ids, dx, counts)
    bits = _scatter(L, dev, src, VOCAB, 50)
    _judge(f"sources {counts}", bits, src, VOCAB, 50)
    if len(counts) > 1:                                           # the same tokens as ONE source: the same bits
        assert torch.equal(bits, _scatter(L, dev, [(ids, dx)], VOCAB, 50))


def test_no_source_gives_a_zero_table(L, dev):
    assert bool((_scatter(L, dev, [], 37, 5) == 0).all())
    assert bool((_scatter(L, dev, [(np.zeros(0, np.int64), np.zeros((0, 5), np.float32))], 37, 5) == 0).all())


def test_full_vocabulary_touched_rows_and_exact_zeros_elsewhere(L, dev):
    """GloVe's 400 003 rows at E = 50: 3000 tokens (ids 0 and vocab - 1 among them, a run of 700 of id 0 beyond two chunks)"""
    vocab, E, T = 400003, 50, 3000
    rng = np.random.default_rng(5)
    ids = rng.integers(0, vocab, size=T, dtype=np.int64)
    ids[:700] = 0
    ids[700:710] = vocab - 1
    ids = ids[rng.permutation(T)]
    dx = rng.standard_normal((T, E)).astype(np.float32)
    src = [(ids[:1000], dx[:1000]), (ids[1000:], dx[1000:])]
    _judge("vocab 400003", _scatter(L, dev, src, vocab, E), src, vocab, E)


def test_unaligned_table_and_small_vocabularies(L, dev):
    """d_emb one float past a 16-byte boundary (no float4 stores), vocabularies below / at / above one 64-row group"""
    for vocab in (1, 63, 64, 65, 130):
        for E, off in ((50, 1), (49, 0), (3, 3)):
            ids, dx = _make("ends", 300, E, vocab=vocab, seed=vocab)
            src = [(ids, dx)]
            _judge(f"vocab {vocab} E{E} off{off}", _scatter(L, dev, src, vocab, E, off=off), src, vocab, E)


def test_ids_outside_the_table_are_dropped(L, dev):
    ids, dx = _make("zipf", 600, 50)
    ids[::7] = -5
    ids[2::17] = -2 ** 40
    ids[3::7] = VOCAB
    ids[5::11] = 2 ** 40
    ids[6::13] = VOCAB + 7
    src = [(ids, dx)]
    _judge("ids outside", _scatter(L, dev, src, VOCAB, 50), src, VOCAB, 50)     # the guard bands are checked in _scatter


def test_scatter_is_deterministic(L, dev):
    """the same call twice, and once from a stream that is busy with another kernel: equal bits"""
    c = _chunk(L)
    ids, dx = _make("zipf", 4 * c + 9, 50)
    src = EG.split_sources(ids, dx, (c, 3 * c + 9))
    first = _scatter(L, dev, src, VOCAB, 50)
    assert torch.equal(first, _scatter(L, dev, src, VOCAB, 50))
    side = torch.cuda.Stream(dev)
    a = torch.randn(2048, 2048, device=dev)
    torch.cuda.synchronize()
    with torch.cuda.stream(side):
        for _ in range(4):
            a = a @ a * 1e-3                                      # keeps the stream busy while the call is enqueued behind it
    assert torch.equal(first, _scatter(L, dev, src, VOCAB, 50, stream=side))


# ------------------------------------------------------------------------------------------------ dx of the GRU backward
DX_CASES = [(1, 1, 1, "full"), (15, 5, 3, "rand"), (16, 7, 4, "full"), (17, 6, 7, "zeros"), (48, 20, 52, "over"),
            (65, 12, 300, "rand")]


def _bwd_dx(L, dev, c, dx, dx_acc=0, b16=False, w_ih=True):
    """umpr_embed_gru_bidir_bwd_dx on the case's own HIP forward (test_gpu_gru._case): NaN-filled gradients and workspace"""
    case = c.case
    N, Lm, E = case.N, case.L, case.E
    d = case.dout.clone()
    d[~G.valid(case)] = float("nan")
    dout = _nan(dev, N, Lm, 2 * H)
    dout[c.order.to(dev)] = d.to(dev)
    g = [_nan(dev, *p.shape) for p in case.w]
    ws, wsb = _ws(L, dev, case)
    out, saved = c.fwd
    wf, wr = (case.w[0].to(dev), case.w[4].to(dev)) if w_ih else (None, None)
    L.call("umpr_set_gemm_bf16", int(b16))
    try:
        L.call("umpr_embed_gru_bidir_bwd_dx", case.ids.to(dev), case.emb.to(dev), E, case.w[1].to(dev), case.w[5].to(dev),
               _i32(case.lengths, dev), _i32(c.order, dev), _i32(c.order, dev), N, Lm, dout, out, saved, *g, 0, wf, wr, dx, dx_acc,
               ws, wsb, st())
    finally:
        L.call("umpr_set_gemm_bf16", 0)
    torch.cuda.synchronize()
    return [t.cpu() for t in g]


def _dx_refs(c):
    case = c.case
    w = lambda i, dt: case.w[i].to(dt).numpy()                  # noqa: E731
    r64 = EG.dx_reference(c.ref.dgx.reshape(-1, 6 * H).numpy(), w(0, torch.float64), w(4, torch.float64))
    r32 = EG.dx_reference(c.ref32.dgx.reshape(-1, 6 * H).numpy(), w(0, torch.float32), w(4, torch.float32), np.float32)
    return EG.as_tensor(r64), EG.as_tensor(r32)


@pytest.mark.parametrize("shape", DX_CASES, ids=lambda s: "-".join(map(str, s)))
def test_token_gradient_of_the_gru_backward(L, dev, shape):
    """dx against the float64 recurrence's input gradient, exact zeros past each length; the eight parameter gradients bit-equal
    to umpr_embed_gru_bidir_bwd_acc on the same inputs, with and without dx; fp32 products under umpr_set_gemm_bf16(1)"""
    c = _case(L, dev, shape)
    case = c.case
    T, E = case.N * case.L, case.E
    g0 = _g0(L, dev, c)
    bits, dx = _sentinel(dev, T * E)
    g = _bwd_dx(L, dev, c, dx)
    assert bool((bits[T * E:] == SENTINEL).all()), "written behind dx"
    for name, a, b in zip(G.GRADS, g, g0):
        assert torch.equal(a, b), (c.tag, name)
    got = dx.cpu().view(T, E)
    assert bool(torch.isfinite(got).all())
    assert bool((got.view(case.N, case.L, E)[~G.valid(case)] == 0).all()), "dx is not zero past a length"
    r64, r32 = _dx_refs(c)
    ok, rows = EG.gate([got], [r64], [r32], names=["dx"], K=EG.K, log=log, tag=c.tag)
    assert ok, rows
    for name, a, b in zip(G.GRADS, _bwd_dx(L, dev, c, None, w_ih=False), g0):          # dx = NULL: today's call
        assert torch.equal(a, b), (c.tag, name, "dx = NULL")
    # accumulate onto a finite prefill
    pre = torch.randn(T, E, generator=torch.Generator().manual_seed(T))
    bits2, dx2 = _sentinel(dev, T * E)
    dx2.copy_(pre.reshape(-1).to(dev))
    _bwd_dx(L, dev, c, dx2, dx_acc=1)
    ok, rows = EG.gate([dx2.cpu().view(T, E)], [pre.double() + r64], [pre + r32], names=["dx accumulate"], K=EG.K, log=log, tag=c.tag)
    assert ok and bool((bits2[T * E:] == SENTINEL).all()), rows
    # the token-gradient products stay fp32 while the library's GEMM mode is bf16
    bits3, dx3 = _sentinel(dev, T * E)
    gb = _bwd_dx(L, dev, c, dx3, b16=True)
    assert torch.equal(dx3.cpu(), dx.cpu()), "dx changed under umpr_set_gemm_bf16(1)"
    if E >= 50:
        assert not torch.equal(gb[0], g0[0]), "the bf16 switch did not take effect on dW_ih"


# ------------------------------------------------------------------------------------------------ whole model vs the oracle
def _cfg(**kw):
    from umpr_amd.config import Config
    cfg = Config(argv=[])
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _model(dev, P, **kw):
    from umpr_amd.model import UMPR
    m = UMPR(_cfg(**kw), P["embedding.weight"].numpy())
    m.load_state_dict(P)
    return m.to(dev)


def _calls(monkeypatch_target, names):
    """record the library entry points a step calls"""
    orig = monkeypatch_target.call

    def call(name, *a):
        names.append(name)
        return orig(name, *a)
    return call


MODEL_CASES = {
    "umpr_r": dict(ronly=True, B=3, kw={}, gru=64),
    "full_V1_B2": dict(ronly=False, B=2, kw={}, gru=64),
    "gru32": dict(ronly=True, B=3, kw=dict(gru_size=32), gru=32),
    "bf16": dict(ronly=True, B=3, kw=dict(dtype="bf16"), gru=64),
}


@pytest.mark.parametrize("name", list(MODEL_CASES))
def test_model_table_gradient_vs_oracle(L, dev, name, monkeypatch):
    """embedding.weight.grad against the oracle with P["embedding.weight"].requires_grad_(True), at the bound the parity tests put on
    the other text-path gradients (2e-3 of the tensor's maximum; bf16: 3e-2 relative L2 of the fp32 oracle); prediction, loss and
    every other gradient bit-equal to a train_embedding=False model on the same inputs.  S = 5, L <= 6.  The full model's oracle
    takes the HIP VGG's own output for the same photos through vgg_fn (the VGG is not under test)."""
    from oracle import umpr_ref as R
    from umpr_amd.synthetic import make_batch, make_param_state
    mc = MODEL_CASES[name]
    ronly = mc["ronly"]
    P = make_param_state(81, 50, 600, 1, ronly, gru_size=mc["gru"], m_scale=0.05)
    batch = make_batch(82, mc["B"], 600, 1, max_sent_count=5, min_sent_count=5, max_ui_sent_count=2, max_sent_length=6,
                       review_net_only=ronly)
    assert tuple(batch[0].shape)[1] == 5 and tuple(batch[0].shape)[2] <= 6
    kw = dict(review_net_only=ronly, views=["unknown"], **mc["kw"])
    res = {}
    for on in (False, True):
        m = _model(dev, P, train_embedding=on, **kw).eval()
        assert m.embedding.weight.requires_grad is on
        vgg_out = []
        if not ronly:
            m.visual_net.vgg16[0].register_forward_hook(lambda mod, i, o: vgg_out.append(o.detach().cpu()))
        names = []
        monkeypatch.setattr(L, "call", _calls(L, names))
        pred, loss = m(*batch)
        loss.backward()
        torch.cuda.synchronize()
        monkeypatch.undo()
        new = [n for n in names if n.endswith("_dx") or n == "umpr_embed_grad"]
        assert (new == []) if not on else (names.count("umpr_embed_grad") == 1 and len(new) == (2 if ronly else 3)), new
        res[on] = (pred.detach().cpu(), loss.detach().cpu(), {k: p.grad.cpu() for k, p in m.named_parameters() if p.grad is not None},
                   vgg_out)
    off, onr = res[False], res[True]
    assert torch.equal(off[0], onr[0]) and torch.equal(off[1], onr[1])
    assert "embedding.weight" not in off[2] and set(onr[2]) == set(off[2]) | {"embedding.weight"}
    for k, g in off[2].items():
        assert torch.equal(g, onr[2][k]), k
    Pr = {k: v.clone() for k, v in P.items()}
    for p in Pr.values():
        p.requires_grad_(True)
    vgg_fn = (lambda flat: onr[3][0]) if not ronly else None
    rp, rl = R.umpr_forward(Pr, batch, review_net_only=ronly, aten=True, vgg_fn=vgg_fn)
    rl.backward()
    if name != "bf16":       # (bf16 predictions have bounds of their own, tests/test_gpu_bf16.py; here they equal the frozen model's)
        check(f"table {name} pred", onr[0], rp, atol=1e-4)
        check(f"table {name} loss", onr[1], rl, atol=1e-4)
    got, ref = onr[2]["embedding.weight"], Pr["embedding.weight"].grad
    assert float(ref.abs().max()) > 0
    touched = torch.zeros(600, dtype=torch.bool)
    for t in batch[:2] if ronly else batch[:3]:
        touched[t.reshape(-1)] = True
    assert bool((got[~touched] == 0).all()) and bool((~touched).any())
    if name == "bf16":
        e = float((got.double() - ref.double()).norm() / ref.double().norm())
        log(f"table bf16: relL2 vs the fp32 oracle {e:.3e}")
        assert e <= 3e-2, e
    else:
        check(f"table {name} grad embedding.weight", got, ref, atol=1e-6, rel_to_max=2e-3)


# ------------------------------------------------------------------------------------------------ Adam, clipping, checkpoints
def _small_batches(n, B=3, vocab=1000):
    from umpr_amd.synthetic import make_batch
    return [make_batch(700 + s, B, vocab, review_net_only=True, max_sent_count=5, min_sent_count=5, max_sent_length=6)
            for s in range(n)]


def _oracle_steps(P, batches, lr, l2, max_norm=None):
    """n Adam steps of the oracle with a trainable table (torch.optim.Adam, the reference's two groups; clip_grad_norm_ when asked).
    Returns (final parameters, per parameter the mask of elements whose gradient was above 1e-4 of its maximum in every step - see
    test_hidden_sizes_below_the_kernel_width_vs_oracle: Adam's first steps are lr * sign(g), so noise-level gradients are left out -, the
    float64 norm of each step's gradient with and without the table, the table rows some step touched)."""
    from oracle import umpr_ref as R
    Pr = {k: v.clone().requires_grad_(True) for k, v in P.items()}
    opt = R.adam_reference(Pr, lr, l2)
    mask = {k: torch.ones_like(v, dtype=torch.bool) for k, v in Pr.items()}
    norms, norms_wo = [], []
    touched = torch.zeros(P["embedding.weight"].shape[0], dtype=torch.bool)
    for b in batches:
        _, loss = R.umpr_forward(Pr, b, review_net_only=True, aten=True, train=True)
        opt.zero_grad()
        loss.backward()
        for k, p in Pr.items():
            big = p.grad.abs() > 1e-4 * p.grad.abs().max()
            if k == "embedding.weight":
                # a table row no token of this step names has a gradient of exactly zero on both sides (the kernel writes +0.0,
                # autograd a zero row): there is no rounding noise whose sign Adam could amplify, so such steps do not exclude it
                big |= (p.grad == 0).all(1, keepdim=True).expand_as(big)
            mask[k] &= big
        sq = {k: float(p.grad.double().pow(2).sum()) for k, p in Pr.items()}
        norms.append(sum(sq.values()) ** 0.5)
        norms_wo.append((sum(sq.values()) - sq["embedding.weight"]) ** 0.5)
        touched[b[0].reshape(-1)] = True
        touched[b[1].reshape(-1)] = True
        if max_norm is not None:
            torch.nn.utils.clip_grad_norm_(list(Pr.values()), max_norm)
        opt.step()
    return {k: v.detach() for k, v in Pr.items()}, mask, norms, norms_wo, touched


def _trajectory_check(model, ref, mask):
    """the tolerance of the trajectory tests (test_train_trajectory_golden, test_gpu_grad_clip._worst_ratio): 2e-5 + 1e-4 |oracle|
    on the elements whose oracle gradient was above 1e-4 of its maximum in every step - the table included"""
    worst = {}
    for k, p in model.named_parameters():
        assert p.requires_grad and mask[k].any(), k
        d = (p.detach().cpu() - ref[k]).abs() / (2e-5 + 1e-4 * ref[k].abs())
        worst[k] = float(d[mask[k]].max())
    log("trajectory error / tolerance: " + ", ".join(f"{k} {v:.3f}" for k, v in worst.items()))
    assert max(worst.values()) <= 1.0, worst
    assert "embedding.weight" in worst


@pytest.mark.parametrize("clip", [False, True])
def test_four_adam_steps_with_a_trainable_table_vs_oracle(dev, clip):
    from oracle.umpr_ref import adam_step_numpy
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_param_state
    from umpr_amd.train import train_step
    lr, l2 = 1e-3, 1e-3
    P = make_param_state(31, 50, 1000, 1, True, m_scale=0.05)
    batches = _small_batches(4)
    _, _, free_norms, _, _ = _oracle_steps(P, batches[:1], lr, l2)
    max_norm = 0.5 * free_norms[0] if clip else None            # half the first step's float64 norm: that step clips for certain
    ref, mask, norms, norms_wo, touched = _oracle_steps(P, batches, lr, l2, max_norm)
    model = _model(dev, P, review_net_only=True, train_embedding=True)
    opt = FusedAdam(model, lr, l2, max_grad_norm=max_norm or 0.0)
    g0 = opt.groups[0]
    assert g0.names[0] == "embedding.weight" and model.embedding.weight in g0.direct     # (UMPR-R has no classifier slice)
    for s, b in enumerate(batches):
        train_step(model, opt, b)
        if clip:
            stats = opt.clip_stats()
            log(f"clip step {s + 1}: norm {stats['norm']:.6f} float64 {norms[s]:.6f} (without the table {norms_wo[s]:.6f})")
            assert abs(stats["norm"] - norms[s]) <= 1e-3 * norms[s], (s, stats, norms[s])
            assert abs(stats["norm"] - norms[s]) < abs(stats["norm"] - norms_wo[s]), "the table's gradient is not in the norm"
            assert (stats["coef"] < 1.0) == (norms[s] > max_norm)
    if clip:
        assert stats["clipped"] >= 1 and stats["skipped"] == 0 and stats["seen"] == 4
    _trajectory_check(model, ref, mask)
    # a row no step touched moves by weight decay alone: closed form, Adam on g = l2 * p
    table = model.embedding.weight.detach().cpu()
    rows = torch.nonzero(~touched & (P["embedding.weight"].abs().sum(1) > 0)).reshape(-1)
    assert rows.numel() > 0
    r = int(rows[0])
    p = P["embedding.weight"][r].double()
    m, v = torch.zeros_like(p), torch.zeros_like(p)
    for step in (1, 2, 3, 4):
        p, m, v = adam_step_numpy(p, torch.zeros_like(p), m, v, step, lr, l2)
    assert bool(((table[r].double() - p).abs() <= 2e-5 + 1e-4 * p.abs()).all()), (r, table[r], p)
    assert float((table[r] - P["embedding.weight"][r]).abs().max()) > 1e-3          # it did move: 4 steps of lr * sign


def test_checkpoint_round_trip_and_refusal_under_the_other_setting(dev, tmp_path):
    """save after 2 steps, resume, step: bit-equal to 3 uninterrupted steps (parameters - the table among them - and moments);
    resuming under the other --train_embedding setting raises before anything is loaded, both ways"""
    from umpr_amd.checkpoint import load_checkpoint, save_checkpoint
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_param_state
    from umpr_amd.train import train_step
    P = make_param_state(101, 50, 500, 1, True, m_scale=0.05)
    batches = _small_batches(3, vocab=500)

    def fresh(on=True):
        m = _model(dev, P, review_net_only=True, train_embedding=on)
        return m, FusedAdam(m, 1e-3, 1e-3, lr_decay=0.99)

    m1, o1 = fresh()
    for b in batches:
        train_step(m1, o1, b)
    m2, o2 = fresh()
    for b in batches[:2]:
        train_step(m2, o2, b)
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, m2, o2, epoch=0, batch_counter=2)
    m3, o3 = fresh()
    assert load_checkpoint(path, m3, o3, map_location=dev)["batch_counter"] == 2
    train_step(m3, o3, batches[2])
    assert not torch.equal(m1.embedding.weight.cpu(), P["embedding.weight"])
    for (k, a), (_, c) in zip(m1.state_dict().items(), m3.state_dict().items()):
        assert torch.equal(a, c), k
    for ga, gc in zip(o1.groups, o3.groups):
        assert torch.equal(ga.m, gc.m) and torch.equal(ga.v, gc.v)
    m4, o4 = fresh(on=False)
    before = {k: v.clone() for k, v in m4.state_dict().items()}
    with pytest.raises(ValueError, match="written with the embedding table trainable, this run has it frozen"):
        load_checkpoint(path, m4, o4, map_location=dev)
    assert all(torch.equal(v, before[k]) for k, v in m4.state_dict().items()) and o4.step_count == 0
    train_step(m4, o4, batches[0])
    frozen_path = str(tmp_path / "frozen.pt")
    save_checkpoint(frozen_path, m4, o4, epoch=0, batch_counter=1)
    m5, o5 = fresh()
    with pytest.raises(ValueError, match="written with the embedding table frozen, this run has it trainable"):
        load_checkpoint(frozen_path, m5, o5, map_location=dev)
    assert torch.equal(m5.embedding.weight.cpu(), P["embedding.weight"])


# ------------------------------------------------------------------------------------------------ default: off
@pytest.mark.parametrize("gname", ["umpr_r_B4", "umpr_r_B3_fullpad"])
def test_default_is_a_frozen_table_and_the_reference_fixtures_hold(L, dev, gname, monkeypatch):
    """A model built without the option: the table takes no gradient, the step calls none of the new entry points, and prediction,
    loss and every gradient stay inside the bounds of the reference's fixtures (test_gpu_parity._compare_golden).  The fixtures hold
    the reference's fp32 CPU results, so this is their bound, not a bit comparison; that the frozen path issues the very calls it
    issued before is what the recorded call names show."""
    from test_gpu_parity import _build, _compare_golden
    g, model, batch = _build(gname, dev)
    assert model.train_embedding is False and not model.embedding.weight.requires_grad
    model.eval()
    names = []
    monkeypatch.setattr(L, "call", _calls(L, names))
    pred, loss = model(*batch)
    loss.backward()
    torch.cuda.synchronize()
    monkeypatch.undo()
    assert model.embedding.weight.grad is None
    assert "umpr_review_net_bwd" in names and not [n for n in names if n.endswith("_dx") or n == "umpr_embed_grad"]
    _compare_golden(g, model, pred, loss, gname)
