"""Frozen conv base (UMPR(freeze_conv=True)): the classifier backward without d_pool5 against the same call with it, bit for bit;
the mode against the unfrozen model and the oracle; the pool5 store (umpr_amd/photos.py::Pool5Store) cold, warm and mixed on the
tiny JPEG set with the files deleted once resident; the refusals; bf16; main.py."""
import os

import numpy as np
import pytest
import torch

import classifier_reference as CR
from test_gpu_classifier import _POOL, F_IN, F_OUT, HID, _Buf, _dev_weights, _gate, _judge, _regions
from test_gpu_feature_store import _state
from test_gpu_parity import L, check, st  # noqa: F401  (fixture: the library)
from test_gpu_parity import log as plog
from test_gpu_photos import _cfg, _model, dev  # noqa: F401  (module fixture)
from test_photo_pack import photo_set, samples_for  # noqa: F401  (module fixture)
from test_photo_store import own_copy
from umpr_amd.data import batch_loader
from umpr_amd.photos import FeatureStore, Pool5Store, conv_fingerprint

pytestmark = pytest.mark.gpu

F = 25088
SLOT = 4 * F
PRE = "visual_net.vgg16.0."


def _bits(t):
    return t.contiguous().view(torch.int32)


@pytest.fixture(scope="module", autouse=True)
def _release_pooled_buffers():
    yield
    _POOL.clear()
    torch.cuda.empty_cache()


# ---- 1. the classifier backward without d_pool5 -------------------------------------------------------------------------------
ENTRIES = {"full": "", "compact": "_compact", "compact_bf16": "_compact_bf16"}


@pytest.mark.parametrize("mode", ["eval", "masks"])
@pytest.mark.parametrize("n", [1, 32, 33, 128, 129])
@pytest.mark.parametrize("entry", list(ENTRIES))
def test_classifier_backward_without_d_pool5(L, dev, entry, n, mode):
    """n = 32 / 33 and 128 / 129 straddle a row tile of fc_small.hip and its hand-over to the generic GEMM.  One forward, then the
    backward twice on NaN-filled gradient buffers and a NaN-filled workspace of exactly the queried size, each with a guard band:
    the six gradients of the call with d_pool5 = NULL equal those of the call with a d_pool5 bit for bit."""
    from umpr_amd.model import _ptr_array
    case = CR.make_case(n, mode, "dense")
    params, _, parr = _dev_weights(dev)
    form = "full" if entry == "full" else "compact"
    nb = L.size("umpr_vgg16_act_bytes" if form == "full" else "umpr_vgg16_cls_arena_bytes", n)
    arena = _Buf(dev, nb // 4, "arena", pooled="full arena" if form == "full" else "compact arena")
    pool5, fc, drop = _regions(arena.t, n, form)
    pool5.copy_(case.pool5.to(dev))
    masks = case.masks.to(dev) if case.masks is not None else torch.full((2, n, HID), 0xFF, dtype=torch.uint8, device=dev)
    out = _Buf(dev, n * F_OUT, "out")
    wsb = L.size("umpr_vgg16_fwd_ws_bytes", n)
    ws = _Buf(dev, wsb // 4, "fwd ws", pooled="ws")
    L.call("umpr_vgg16_classifier_fwd" + ENTRIES[entry], parr, n, case.train, case.use_masks, case.seed, arena.t, masks, out.t, ws.t,
           wsb, st())
    torch.cuda.synchronize()
    assert ws.guard_ok() and arena.guard_ok() and out.guard_ok() and not bool(torch.isnan(out.t).any())
    d_out = case.d_out.to(dev)
    wsb = L.size("umpr_vgg16_classifier_bwd_ws_bytes", n)
    unused = _Buf(dev, 64, "convolution gradients")
    runs = []
    for with_dx in (True, False):
        grads = [_Buf(dev, p.numel(), nm, pooled=f"{nm} {with_dx}") for nm, p in zip(CR.GRAD_NAMES, params)]
        d_pool5 = _Buf(dev, n * F_IN, "d_pool5", pooled="d_pool5") if with_dx else None
        ws = _Buf(dev, wsb // 4, "bwd ws", pooled="ws")
        keep, garr = _ptr_array([unused.t] * 26 + [g.t for g in grads])
        L.call("umpr_vgg16_classifier_bwd" + ENTRIES[entry], parr, n, int(case.dropout), arena.t, masks, d_out, garr,
               d_pool5.t if with_dx else None, ws.t, wsb, st())       # None: a NULL pointer
        torch.cuda.synchronize()
        assert ws.guard_ok() and unused.untouched() and all(g.guard_ok() for g in grads), with_dx
        assert not any(bool(torch.isnan(g.t).any()) for g in grads), with_dx
        if with_dx:
            assert d_pool5.guard_ok() and not bool(torch.isnan(d_pool5.t).any())
        runs.append(grads)
    for a, b in zip(*runs):
        assert torch.equal(_bits(a.t), _bits(b.t)), a.name
    assert float(runs[1][0].t.abs().max()) > 0 and torch.equal(pool5.cpu(), case.pool5)


# ---- models -------------------------------------------------------------------------------------------------------------------
VIEWS = ["food", "inside", "outside", "drink"]


def _conv_frozen(V, dev, dtype="fp32", **kw):
    kw.setdefault("freeze_conv", True)
    return _model(_cfg(review_net_only=False, views=VIEWS[:V], dtype=dtype, **kw), _state(V), dev)


@pytest.fixture(scope="module")
def model1(dev):
    """freeze_conv, one view: shared by the store tests, which never write a conv parameter"""
    return _conv_frozen(1, dev)


def _masks(n, seed, dev):
    g = torch.Generator().manual_seed(seed)
    return (torch.rand(2, n, HID, generator=g) < 0.5).to(torch.uint8).to(dev)


def _reset_trainable(model, V):
    """The trainable parameters back to their initial values; no conv parameter is written (that would empty a store)."""
    P = _state(V)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if p.requires_grad:
                p.copy_(P[k])


# ---- 2. the mode --------------------------------------------------------------------------------------------------------------
def test_mode_trains_the_classifier_only(dev):
    from umpr_amd.synthetic import make_batch
    model = _conv_frozen(1, dev)
    plain = _conv_frozen(1, dev, freeze_conv=False)
    vgg, ref = model.visual_net.vgg16[0], plain.visual_net.vgg16[0]
    batch = make_batch(171, 2, 500, 1)
    model.train()
    calls = vgg._calls
    with torch.enable_grad():
        pred, loss = model(*batch)
        assert vgg._calls == calls + 1
        loss.backward()
        model(*batch)
        assert vgg._calls == calls + 2                                     # once per training forward: the dropout masks follow it
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    feats = [k for k in named if k.startswith(PRE + "features.")]
    cls = [k for k in named if k.startswith(PRE + "classifier.")]
    assert len(feats) == 26 and all(named[k].grad is None for k in feats)
    assert len(cls) == 6
    for k in cls:
        g = named[k].grad
        assert g is not None and bool(torch.isfinite(g).all()) and float(g.abs().max()) > 0, k
    # eval, as evaluate_mse runs it: the unfrozen model's eval output on the same weights, bit for bit
    images = batch[6].reshape(-1, 3, 224, 224).to(dev)
    model.eval(), plain.eval()
    with torch.no_grad():
        a, b = vgg(images), ref(images)
        p5 = vgg.conv_base(images)
    assert torch.equal(a, b) and a.shape == (2, 1000) and bool(torch.isfinite(a).all()) and float(a.abs().max()) > 0
    assert p5.shape == (2, F) and p5.dtype == torch.float32 and not p5.requires_grad
    # training output: a function of the classifier, which carries the graph; the conv stage kept nothing
    model.train()
    with torch.enable_grad():
        out = vgg(images)
    assert out.requires_grad and out.grad_fn is not None


# ---- 3. against the oracle ----------------------------------------------------------------------------------------------------
def _oracle(P, batch, masks):
    """R.umpr_forward in training mode with the injected masks, the features.* entries of P not requiring grad: exactly the
    freeze_conv model.  Returns (P, pred, loss)."""
    from oracle import umpr_ref as R
    Pr = {k: (v if ".features." in k else v.clone()) for k, v in P.items()}
    for k, p in Pr.items():
        if k != "embedding.weight" and ".features." not in k:
            p.requires_grad_(True)
    rp, rl = R.umpr_forward(Pr, batch, review_net_only=False, train=True, dropout_masks=[m.float() for m in masks.cpu()], aten=True)
    rl.backward()
    return Pr, rp.detach(), rl.detach()


def _step_slack(g, p0, lr, wd, eps=1e-8):
    """What the gradient bound of this test allows a parameter to differ by after Adam's FIRST step.  That step is
    p - lr h(g + wd p) with h(x) = x / (|x| + eps), and the HIP gradient may be delta = 1e-6 + 2e-3 max|g| away from the oracle's:
    the stepped value may then differ by lr (h(x + delta) - h(x - delta)) - next to nothing where |x| >> delta, up to 2 lr where the
    sign of x is within the gradient's own tolerance.  test_frozen_model_vs_oracle compares with 2e-5 + 1e-4 |p| alone, which holds
    only while no compared element has |x| near delta; here one of 9 499 compared elements of control_net.c_net.gru.module.
    weight_ih_l0_reverse came out 3.87e-5 off against 3.2e-5, with every gradient inside its bound."""
    x = (g + wd * p0).double()
    delta = 1e-6 + 2e-3 * float(g.abs().max())
    h = lambda v: v / (v.abs() + eps)       # noqa: E731
    return (lr * (h(x + delta) - h(x - delta))).float()


def _capture_classifier(monkeypatch):
    """Every (pool5, arena) pair _VGGClassifier is given while the test runs."""
    import umpr_amd.model as M
    runs = []
    orig = M._VGGClassifier.apply

    def apply(pool5, arena, *rest):
        runs.append((pool5, arena))
        return orig(pool5, arena, *rest)

    monkeypatch.setattr(M._VGGClassifier, "apply", apply)
    return runs


@pytest.mark.parametrize("V,Pc", [(1, 1), (2, 2)])
def test_freeze_conv_vs_oracle(dev, monkeypatch, V, Pc):
    """Training mode, injected dropout masks on both sides.  Predictions and loss to 1e-4; every non-VGG gradient to atol 1e-6 +
    2e-3 of its maximum (test_gpu_feature_store.py::_compare's bounds); the six classifier gradients as tests/test_gpu_classifier.py
    judges them: against the float64 backward fed the HIP arena's pool5 / fc / drop regions, the masks and the d_out that reached the
    VGG output, to CR.k_of(name) x the distance the float32 CPU evaluation has from it.  At V = 1 also one Adam step: every stepped
    parameter against R.adam_reference at the elements test_frozen_model_vs_oracle compares, to 2e-5 + 1e-4 |p| plus _step_slack
    (which see); the conv weights stay bit-equal to their initial values."""
    from oracle import umpr_ref as R
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_batch
    from umpr_amd.train import train_step
    P = _state(V)
    n = 2 * V * Pc
    batch = make_batch(180 + V, 2, 500, V, Pc)
    model = _conv_frozen(V, dev)
    vgg = model.visual_net.vgg16[0]
    masks = _masks(n, 190 + V, dev)
    vgg.dropout_masks = masks
    model.train()
    runs = _capture_classifier(monkeypatch)
    d_outs = []
    hook = vgg.register_forward_hook(lambda mod, inp, out: out.register_hook(lambda gr: d_outs.append(gr.detach().clone())) and None)
    try:
        pred, loss = model(*batch)
        loss.backward()
        torch.cuda.synchronize()
    finally:
        hook.remove()
    assert len(runs) == 1 and len(d_outs) == 1
    tag = f"freeze_conv V{V} P{Pc}"
    Pr, rp, rl = _oracle(P, batch, masks)
    check(f"{tag} pred", pred, rp, atol=1e-4)
    check(f"{tag} loss", loss, rl, atol=1e-4)
    named = dict(model.named_parameters())
    seen = 0
    for k, p in named.items():
        if p.requires_grad and ".vgg16." not in k:
            check(f"{tag} grad {k}", p.grad, Pr[k].grad, atol=1e-6, rel_to_max=2e-3)
            seen += 1
    assert seen == 37
    assert all(named[k].grad is None for k in named if ".features." in k)
    # the classifier gradients, conditioned on the decisions the HIP forward took
    pool5, arena = runs[0]
    p5, fc, drop = _regions(arena, n, "compact")
    assert pool5.data_ptr() == p5.data_ptr()
    cls = vgg.param_list()[26:]
    p64 = [p.detach().double() for p in cls]
    p32 = [P[PRE + f"classifier.{i}.{w}"] for i in (0, 3, 6) for w in ("weight", "bias")]
    assert all(torch.equal(a.detach().cpu(), b) for a, b in zip(cls, p32))
    d_out = d_outs[0]
    g64, _ = CR.classifier_backward(p5, fc, drop, p64, d_out, masks, device=dev)
    g32, _ = CR.classifier_backward(p5.cpu(), [t.cpu() for t in fc], [t.cpu() for t in drop], p32, d_out.cpu(), masks.cpu(), torch.float32)
    rows = []
    for nm, p, r, r32 in zip(CR.GRAD_NAMES, cls, g64, g32):
        rows += _gate(tag, nm, p.grad, r, r32)
    del g64, g32, p64
    _judge(tag, rows)
    if V == 1:
        first = {k: p.detach().clone() for k, p in named.items() if ".features." in k}
        opt = FusedAdam(model, 1e-3, 1e-3)
        ropt = R.adam_reference(Pr, 1e-3, 1e-3)
        assert sum(len(g["params"]) for g in ropt.param_groups) == sum(len(g.params) for g in opt.groups) == 43
        train_step(model, opt, batch)
        ropt.step()                   # on the gradients of the backward above: P has not moved since
        torch.cuda.synchronize()
        for k, p in model.named_parameters():
            if k == "visual_net.linear.bias":
                continue              # its gradient is identically zero (test_gpu_feature_store.py::test_frozen_model_vs_oracle)
            if p.requires_grad:
                gr = Pr[k].grad
                big = gr.abs() > 1e-4 * gr.abs().max()
                got, want = p.detach().cpu()[big], Pr[k].detach()[big]
                err = (got - want).abs()
                tol = 2e-5 + 1e-4 * want.abs() + _step_slack(gr, P[k], 1e-3, 0.0 if "bias" in k else 1e-3)[big]
                bad = int((err > tol).sum())
                plog(f"{tag} stepped {k}: max_err={float(err.max()):.3e} bad={bad}/{got.numel()} "
                     f"(outside the plain 2e-5 + 1e-4 |p|: {int((err > 2e-5 + 1e-4 * want.abs()).sum())})")
                assert bad == 0 and bool(torch.isfinite(got).all()), (k, bad, float(err.max()))
            elif ".features." in k:
                assert torch.equal(p, first[k]) and torch.equal(p.detach().cpu(), P[k]) and p.grad is None, k


# ---- 4. the store -------------------------------------------------------------------------------------------------------------
def _collate(store, samples, host=False):
    return batch_loader(samples, resize_on_gpu=not host, store=None if host else store.index)


def _row(store, path):
    s = store.slot_of(path)
    assert 0 <= s < store.slots
    return store.buffer[s * F:(s + 1) * F]


def _rows(arena, n):
    return arena[:n * F].view(n, F)


def _count_conv_base(vgg, monkeypatch):
    calls = []
    orig = vgg.conv_base
    monkeypatch.setattr(vgg, "conv_base", lambda images: calls.append(images.shape[0]) or orig(images))
    return calls


def test_cold_then_warm_pass(L, dev, photo_set, model1, tmp_path, monkeypatch):
    paths = own_copy(photo_set[:3] + photo_set[7:8], tmp_path)              # 500x375, 224x224, 100x80, grey
    samples = samples_for(paths, 3, 1, 2)                                  # 6 photos: p0 p1 p2 p3 p0 p1 (model1 has one view)
    flat = [p for s in samples for v in s[3] for p in v]
    vgg = model1.visual_net.vgg16[0]
    store = Pool5Store(dev, capacity_bytes=8 * SLOT + 100).register(paths)
    assert store.slots == 8 and store.slot_bytes == SLOT == 100352 and store.buffer.numel() == 9 * F
    assert Pool5Store.find(store.key) is store and FeatureStore.find(store.key) is None
    host = batch_loader(samples)[6].reshape(-1, 3, 224, 224).to(dev)
    want = vgg.conv_base(host[:4]).clone()                                 # the compacted miss batch: same images, same order
    calls = _count_conv_base(vgg, monkeypatch)
    raw = _collate(store, samples)[6]
    assert not raw.hits.any()
    arena = store.features(raw, vgg)
    assert calls == [4] and arena.dtype == torch.float32 and not arena.requires_grad
    assert arena.numel() * 4 == L.size("umpr_vgg16_cls_arena_bytes", 6)
    cold = _rows(arena, 6).clone()
    for k, p in enumerate(paths):
        assert torch.equal(_row(store, p), want[k]), p
    assert torch.equal(cold, want[[0, 1, 2, 3, 0, 1]]) and float(cold.abs().max()) > 0
    s = store.stats()
    assert (s["used"], s["inserts"], s["computed"], s["shared"], s["hits"], s["vgg_calls"]) == (4, 4, 4, 2, 0, 1)
    assert s["bytes"] == 9 * SLOT
    model1.eval()
    with torch.no_grad():
        ref_vgg = vgg(host)                                                # the host form of all six photos
    for p in paths:
        os.remove(p)
    raw = _collate(store, samples)[6]                                      # no file is there to be opened
    assert raw.hits.all() and not (raw.descriptors()["rows"] > 0).any() and raw.data.numel() == 6 * 24
    warm = _rows(store.features(raw, vgg), 6)
    assert calls == [4] and store.stats()["vgg_calls"] == 1 and store.stats()["hits"] == 6
    assert torch.equal(warm, torch.stack([_row(store, p) for p in flat])) and torch.equal(warm, cold)
    # the fetch on another stream than the fill waits for the fill's event
    second = torch.cuda.Stream(dev)
    with torch.cuda.stream(second):
        other = _rows(store.features(_collate(store, samples)[6], vgg), 6)
    second.synchronize()
    assert torch.equal(other, cold) and calls == [4]
    # the classifier on the stored rows is the classifier on the photos.  The host form runs six photos through the conv stage in
    # one batch, the store ran four: the kernels may tile another batch another way.  tests/test_gpu_parity.py holds the VGG output
    # to 1e-4 of its maximum against float64 at every batch size, so two batch sizes are within twice that of each other
    with torch.no_grad():
        through = vgg.classify(store.features(_collate(store, samples)[6], vgg), 6)
        pred, loss = model1(*_collate(store, samples))
    check("the classifier on stored rows", through, ref_vgg, atol=1e-6, rel_to_max=2e-4)
    assert calls == [4] and pred.shape == (3,) and bool(torch.isfinite(pred).all()) and bool(torch.isfinite(loss))


def test_mixed_pass_and_the_zero_row(dev, photo_set, model1, monkeypatch):
    """One batch with hits, first misses, the same id twice, and missing photos."""
    p = photo_set
    vgg = model1.visual_net.vgg16[0]
    store = Pool5Store(dev, capacity_bytes=8 * SLOT).register(p[:3] + p[7:10])
    first = _collate(store, samples_for(p[:3], 1, 3, 1))[6]
    store.features(first, vgg)
    held = {q: _row(store, q).clone() for q in p[:3]}
    order = [p[0], p[7], p[1], p[8], p[7], p[2], "unknown", p[11]]         # p[11] does not exist
    samples = samples_for(order, 2, 1, 4)                                   # one view, as model1 has: the same eight in this order
    host = batch_loader(samples)[6].reshape(-1, 3, 224, 224).to(dev)
    fresh = vgg.conv_base(host[[1, 3]]).clone()
    zero = vgg.conv_base(torch.zeros(1, 3, 224, 224, device=dev)).clone()
    calls = _count_conv_base(vgg, monkeypatch)
    batch = _collate(store, samples)
    assert batch[6].hits.tolist() == [1, 0, 1, 0, 0, 1, 0, 0]
    got = _rows(store.features(batch[6], vgg), 8).clone()
    assert calls == [1, 2]                                                  # the zero image in one call, the two new photos in one
    want = torch.stack([held[p[0]], fresh[0], held[p[1]], fresh[1], fresh[0], held[p[2]], zero[0], zero[0]])
    assert torch.equal(got, want)
    assert torch.equal(_row(store, p[7]), fresh[0]) and torch.equal(_row(store, p[8]), fresh[1])
    assert torch.equal(store.buffer[store.zero_slot * F:], zero[0]) and all(torch.equal(_row(store, q), held[q]) for q in held)
    s = store.stats()
    assert (s["used"], s["inserts"], s["hits"], s["computed"], s["shared"], s["missing"], s["vgg_calls"]) == (5, 5, 3, 5, 1, 2, 3)
    batch = _collate(store, samples)
    assert batch[6].hits.tolist() == [1] * 6 + [0, 0]
    assert torch.equal(_rows(store.features(batch[6], vgg), 8), want) and calls == [1, 2]      # the zero row is computed once
    model1.eval()
    with torch.no_grad():
        pred, loss = model1(*batch)
    assert calls == [1, 2] and pred.shape == (2,) and bool(torch.isfinite(pred).all())


def test_one_slot_three_photos(dev, photo_set, model1, monkeypatch):
    p = photo_set[:3]
    vgg = model1.visual_net.vgg16[0]
    store = Pool5Store(dev, capacity_bytes=SLOT + SLOT - 1).register(p)
    assert store.slots == 1
    samples = samples_for(p, 1, 3, 1)
    calls = _count_conv_base(vgg, monkeypatch)
    outs = []
    for k in range(3):
        raw = _collate(store, samples)[6]
        assert raw.hits.tolist() == ([0, 0, 0] if k == 0 else [1, 0, 0])
        outs.append(_rows(store.features(raw, vgg), 3).clone())
    assert calls == [3, 2, 2]
    s = store.stats()
    assert (s["slots"], s["used"], s["inserts"], s["hits"], s["decoded_while_full"], s["computed"]) == (1, 1, 1, 2, 6, 7)
    assert torch.equal(outs[1], outs[2]) and torch.equal(outs[0][0], outs[1][0])
    # two misses per call instead of three: the conv kernels may tile another batch another way.  tests/test_gpu_parity.py holds the
    # conv stack to 1e-4 of the output's maximum against float64 at every batch size, so two batch sizes are within twice that
    check("recomputed rows", outs[1], outs[0], atol=1e-6, rel_to_max=2e-4)


def test_warm_training_steps_repeat_and_leave_the_store_alone(dev, photo_set, tmp_path, monkeypatch):
    from umpr_amd._lib import UmprHipError
    from umpr_amd.optim import FusedAdam
    from umpr_amd.train import train_step
    paths = own_copy(photo_set[:2], tmp_path)
    samples = samples_for(paths, 2, 1, 1, seed=31)
    model = _conv_frozen(1, dev)
    vgg = model.visual_net.vgg16[0]
    vgg.dropout_masks = _masks(2, 41, dev)
    store = Pool5Store(dev, capacity_bytes=4 * SLOT).register(paths)
    model.train()
    model(*_collate(store, samples))                                       # the cold pass
    for p in paths:
        os.remove(p)
    calls = _count_conv_base(vgg, monkeypatch)
    fp = conv_fingerprint(vgg)
    cls = [k for k, _ in model.named_parameters() if k.startswith(PRE + "classifier.")]
    runs = []
    for _ in range(2):
        _reset_trainable(model, 1)
        torch.manual_seed(5)
        vgg._calls = 7
        opt = FusedAdam(model, 1e-3, 1e-3)
        batch = _collate(store, samples)
        assert batch[6].hits.all()
        pred, loss = train_step(model, opt, batch)
        torch.cuda.synchronize()
        named = dict(model.named_parameters())
        runs.append((pred.detach().clone(), loss.detach().clone(), {k: named[k].grad.detach().clone() for k in cls},
                     {k: v.detach().clone() for k, v in model.state_dict().items()}))
        assert vgg._calls == 8
    assert calls == [] and conv_fingerprint(vgg) == fp
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in cls:
        assert torch.equal(_bits(runs[0][2][k]), _bits(runs[1][2][k])) and float(runs[0][2][k].abs().max()) > 0, k
    for k in runs[0][3]:
        assert torch.equal(runs[0][3][k], runs[1][3][k]), k
    assert not torch.equal(runs[0][3][PRE + "classifier.0.weight"], _state(1)[PRE + "classifier.0.weight"].to(dev))
    # the steps moved the classifier and left the store as it is: the next batch hits
    s = store.stats()
    assert s["flushes"] == 0 and s["used"] == 2 and s["vgg_calls"] == 1
    batch = _collate(store, samples)
    assert batch[6].hits.all()
    model(*batch)
    assert calls == [] and store.stats()["flushes"] == 0
    # a reload of the same values is a write to the conv parameters: empty, and a batch collated before it is refused
    stale = _collate(store, samples)
    model.load_state_dict({k: v.clone() for k, v in model.state_dict().items()})
    assert conv_fingerprint(vgg) != fp
    with pytest.raises(UmprHipError, match="left to the store, which does not hold it"):
        model(*stale)
    s = store.stats()
    assert s["flushes"] == 1 and s["used"] == 0 and not store.index.resident.any()


# ---- 5. refusals --------------------------------------------------------------------------------------------------------------
def test_refusals(dev, photo_set, model1):
    from umpr_amd._lib import UmprHipError
    from umpr_amd.model import VGG16
    p = photo_set[:2]
    samples = samples_for(p, 2, 1, 1)
    store = Pool5Store(dev, capacity_bytes=4 * SLOT).register(p)
    plain = _conv_frozen(1, dev, freeze_conv=False)
    with pytest.raises(UmprHipError, match="pool5 store reached a model without freeze_conv"):
        plain(*_collate(store, samples))
    del plain
    fstore = FeatureStore(dev, capacity_bytes=4 * 4000).register(p)
    with pytest.raises(UmprHipError, match="feature store reached a model whose VGG trains"):
        model1(*_collate(fstore, samples))
    with torch.device("meta"):
        trainable = VGG16()
    trainable.classifier.requires_grad_(False)                              # a conv parameter that trains is enough
    with pytest.raises(UmprHipError, match="Pool5Store: the conv base has trainable parameters"):
        store.features(_collate(store, samples)[6], trainable)
    # two views for a model of one: the head is told no sizes and would read behind pos_v_emb, the gates and the fusion weight
    with pytest.raises(RuntimeError, match="photos of 2 views, the model was built for 1"):
        model1(*_collate(store, samples_for(p, 2, 2, 1)))
    assert store.stats()["used"] == 0 and store.stats()["vgg_calls"] == 0
    assert fstore.stats()["used"] == 0 and fstore.stats()["vgg_calls"] == 0


# ---- 6. bf16 ------------------------------------------------------------------------------------------------------------------
def test_bf16_warm_equals_cold_and_evaluate_mse_uses_the_store(dev, photo_set, tmp_path, monkeypatch):
    from umpr_amd.train import evaluate_mse
    paths = own_copy(photo_set[:3] + photo_set[7:8], tmp_path)
    samples = samples_for(paths, 2, 2, 1, seed=33)                         # four photos, each once: the miss batch is the batch
    model = _conv_frozen(2, dev, dtype="bf16").eval()
    vgg = model.visual_net.vgg16[0]
    store = Pool5Store(dev, capacity_bytes=4 * SLOT).register(paths)
    on_host = evaluate_mse(model, [_collate(store, samples, host=True)])
    calls = _count_conv_base(vgg, monkeypatch)
    through = evaluate_mse(model, [_collate(store, samples)])
    assert calls == [4] and through == on_host and np.isfinite(on_host)
    with torch.no_grad():
        cold = model(*_collate(store, samples))
        assert store.stats()["hits"] == 4 and calls == [4]
        rows = torch.stack([_row(store, q) for q in paths])
        for q in paths:
            os.remove(q)
        batch = _collate(store, samples)
        assert batch[6].hits.all()
        warm = model(*batch)
        feats = _rows(store.features(_collate(store, samples)[6], vgg), 4)
    assert calls == [4] and torch.equal(feats, rows)
    assert torch.equal(cold[0], warm[0]) and torch.equal(cold[1], warm[1])
    assert evaluate_mse(model, [_collate(store, samples)]) == on_host
    # and it trains: the bf16 classifier backward without d_pool5 through the module
    model.train()
    pred, loss = model(*_collate(store, samples))
    loss.backward()
    torch.cuda.synchronize()
    named = dict(model.named_parameters())
    assert all(named[k].grad is None for k in named if ".features." in k) and calls == [4]
    for k in named:
        if ".classifier." in k:
            assert bool(torch.isfinite(named[k].grad).all()) and float(named[k].grad.abs().max()) > 0, k


# ---- 7. main.py ---------------------------------------------------------------------------------------------------------------
def test_main_cli_with_a_frozen_conv_base_and_the_pool5_store(tmp_path, capsys, monkeypatch):
    """main.py --freeze_conv True --pool5_store_gb X on the tiny CSV corpus, in-process as tests/test_gpu_e2e.py runs the CLI: the
    store is built instead of the photo store, fills in the first validation pass and serves training, validation and the test;
    without --freeze_conv True the option is refused before anything is built."""
    import importlib
    import json
    import shutil
    import sys
    from PIL import Image
    corpus = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "tiny_corpus")
    d = tmp_path / "music"
    (d / "photos").mkdir(parents=True)
    for split in ("train", "valid", "test"):
        shutil.copy(os.path.join(corpus, "train.csv"), d / f"{split}.csv")
    shutil.copy(os.path.join(corpus, "photos.json"), d / "photos.json")
    g = np.random.default_rng(9)
    ids = [json.loads(line)["photo_id"] for line in open(d / "photos.json")]
    for pid in ids[::2]:                                                   # every other photo exists; the rest are missing photos
        Image.fromarray(g.integers(0, 256, (60, 80, 3), dtype=np.uint8)).save(d / "photos" / f"{pid}.jpg", quality=90)
    argv = ["main.py", "--data_dir", str(d), "--word2vec_file", os.path.join(corpus, "glove.txt"), "--train_epochs", "1",
            "--batch_size", "3", "--max_sent_count", "6", "--min_sent_count", "2", "--max_ui_sent_count", "3", "--max_sent_length", "10",
            "--views", "inside", "--learning_rate", "1e-3", "--model_path", str(tmp_path / "m.pt"), "--pool5_store_gb", "0.01",
            "--photo_store_gb", "0.01"]
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main")
    monkeypatch.setattr(sys, "argv", argv)
    with pytest.raises(SystemExit, match="--pool5_store_gb needs --freeze_conv True"):
        main.main()
    monkeypatch.setattr(sys, "argv", argv + ["--freeze_conv", "True"])
    main.main()
    out = capsys.readouterr().out
    assert "Pool5 store: 99 slots of 100352 B" in out and "it replaces the photo store" in out
    assert "Photo store" not in out and "Feature store" not in out
    assert "Initial validation mse is" in out and "Test end, test mse is" in out, out[-2000:]
    stats = [eval(line.split(": ", 1)[1]) for line in out.splitlines() if "Pool5 store after" in line]
    assert len(stats) == 2
    train, test = stats
    assert 0 < train["used"] == train["inserts"] == train["computed"] <= len(ids[::2])      # every photo went through the conv base once
    assert train["hits"] > 0 and train["missing"] > 0 and train["flushes"] == 0             # the Adam steps emptied nothing
    assert test["hits"] > train["hits"]
    mse = float(out.strip().split("test mse is")[-1].split()[0])
    assert mse == mse and mse < 100.0
