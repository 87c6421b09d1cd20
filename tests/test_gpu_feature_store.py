"""Frozen VGG (UMPR(freeze_vgg=True)) and the device-resident feature store (umpr_amd/photos.py::FeatureStore, csrc/photos.hip::
umpr_feature_fetch_f32): the kernel against a numpy gather bit for bit, the frozen stack against its own eval output and the
oracle, and cold / warm / mixed passes through the store on the tiny JPEG set, with the files deleted once resident."""
import os

import numpy as np
import pytest
import torch

from test_gpu_parity import check
from test_gpu_photos import _cfg, _model, dev  # noqa: F401  (module fixture)
from test_photo_pack import photo_set, samples_for  # noqa: F401  (module fixture)
from test_photo_store import own_copy
from umpr_amd.data import batch_loader
from umpr_amd.photos import FeatureStore, vgg_fingerprint

pytestmark = pytest.mark.gpu

F = 1000
NAN = np.float32(np.nan).view(np.int32)         # the bit pattern the buffers are filled with


# ---- the kernel --------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32)


class _Buffers:
    """`store` [n_slots][F] and `out` [n][F], all NaN, each with a NaN guard band behind it; `fresh` [n_fresh][F] of random bit
    patterns (NaNs, infinities and denormals among them: the copy must not look at the values)."""

    GUARD = 4096

    def __init__(self, dev, n, n_fresh, n_slots, Fk, seed):
        g = np.random.default_rng(seed)
        self.Fk, self.n, self.n_slots = Fk, n, n_slots
        self.fresh_host = g.integers(-2 ** 31, 2 ** 31, (max(n_fresh, 1), Fk), dtype=np.int64).astype(np.int32)
        self.fresh = torch.from_numpy(self.fresh_host).to(dev).view(torch.float32)
        self.store_all = torch.full((n_slots * Fk + self.GUARD,), float("nan"), device=dev)
        self.out_all = torch.full((n * Fk + self.GUARD,), float("nan"), device=dev)
        self.store, self.out = self.store_all[:n_slots * Fk], self.out_all[:n * Fk]
        assert self.store.data_ptr() % 16 == 0 and self.out.data_ptr() % 16 == 0 and self.fresh.data_ptr() % 16 == 0

    def fill_store(self, seed):
        g = np.random.default_rng(seed)
        host = g.integers(-2 ** 31, 2 ** 31, (self.n_slots, self.Fk), dtype=np.int64).astype(np.int32)
        _bits(self.store).copy_(torch.from_numpy(host).reshape(-1))
        return host

    def call(self, row, src, dst, n_fresh, dev, n_slots=None, Fk=None, out=None):
        from umpr_amd._lib import lib
        row, src, dst = (np.ascontiguousarray(a, dtype=np.int32) for a in (row, src, dst))
        lib().call("umpr_feature_fetch_f32", self.fresh, n_fresh, row.ctypes.data, src.ctypes.data, dst.ctypes.data, len(row),
                   self.Fk if Fk is None else Fk, self.store, self.n_slots if n_slots is None else n_slots,
                   self.out if out is None else out, torch.cuda.current_stream(dev).cuda_stream)
        torch.cuda.synchronize()

    def host(self):
        return (_bits(self.store).cpu().numpy().reshape(self.n_slots, self.Fk), _bits(self.out).cpu().numpy().reshape(self.n, self.Fk))

    def guards_intact(self):
        return bool((_bits(self.store_all[self.n_slots * self.Fk:]) == int(NAN)).all()
                    and (_bits(self.out_all[self.n * self.Fk:]) == int(NAN)).all())

    def untouched(self):
        return bool((_bits(self.store_all) == int(NAN)).all() and (_bits(self.out_all) == int(NAN)).all())


@pytest.mark.parametrize("Fk", [1000, 4])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 129])
def test_kernel_equals_a_numpy_gather_bit_for_bit(dev, n, Fk):
    """64 photos travel per launch: n = 63 / 64 / 65 / 129 fall on both sides of one and of two argument chunks."""
    g = np.random.default_rng(1000 * n + Fk)
    n_slots = n + 7
    # all fresh, every row its own, and every one fills a slot (in a scattered order)
    b = _Buffers(dev, n, n, n_slots, Fk, seed=n)
    row, src = np.arange(n), np.full(n, -1)
    dst = g.permutation(n_slots)[:n]
    b.call(row, src, dst, n, dev)
    store, out = b.host()
    assert np.array_equal(out, b.fresh_host[:n]) and np.array_equal(store[dst], b.fresh_host[:n])
    rest = np.setdiff1d(np.arange(n_slots), dst)
    assert (store[rest] == NAN).all() and b.guards_intact()
    # all hits: the store is only read
    b = _Buffers(dev, n, 0, n_slots, Fk, seed=n + 1)
    held = b.fill_store(n + 2)
    src = g.integers(0, n_slots, n)
    b.call(np.full(n, -1), src, np.full(n, -1), 0, dev)
    store, out = b.host()
    assert np.array_equal(out, held[src]) and np.array_equal(store, held) and b.guards_intact()
    # mixed: hits, fresh rows shared by several photos, fills (never of a slot the call reads)
    n_fresh = max(1, n // 3)
    b = _Buffers(dev, n, n_fresh, n_slots, Fk, seed=n + 3)
    held = b.fill_store(n + 4)
    is_hit = g.random(n) < 0.4
    if n > 1:
        is_hit[0], is_hit[-1] = True, False
    read = np.arange(0, n_slots // 2)
    src = np.where(is_hit, g.choice(read, n), -1)
    row = np.where(is_hit, -1, g.integers(0, n_fresh, n))
    free = g.permutation(np.arange(n_slots // 2, n_slots))
    dst = np.full(n, -1)
    fills = np.flatnonzero(~is_hit)[:len(free)][::2]
    dst[fills] = free[:len(fills)]
    b.call(row, src, dst, n_fresh, dev)
    store, out = b.host()
    want = np.where(is_hit[:, None], held[np.maximum(src, 0)], b.fresh_host[np.maximum(row, 0)])
    assert np.array_equal(out, want)
    after = held.copy()
    after[dst[fills]] = want[fills]
    assert np.array_equal(store, after) and b.guards_intact()


def test_kernel_refusals_leave_both_buffers_untouched(dev):
    from umpr_amd._lib import UmprHipError
    n_slots, n_fresh = 4, 2
    b = _Buffers(dev, 3, n_fresh, n_slots, F, seed=5)
    cases = [([0, 1, -1], [-1, -1, n_slots], [-1] * 3, {}),          # src_slot outside the store
             ([0, 1, 0], [-1] * 3, [-1, n_slots, -1], {}),          # dst_slot outside the store
             ([0, 1, 0], [-1, 2, -1], [-1] * 3, {}),                # both a src_slot and a fresh_row
             ([0, -1, 1], [-1] * 3, [-1] * 3, {}),                  # neither
             ([0, n_fresh, 1], [-1] * 3, [-1] * 3, {}),             # fresh_row outside [0, n_fresh)
             ([0, 1, 0], [-1] * 3, [3, -1, 3], {}),                 # one dst_slot twice
             ([0, -1, 1], [-1, 2, -1], [2, -1, -1], {}),            # a dst_slot that the same call reads
             ([0, 1, 0], [-1] * 3, [-1] * 3, dict(Fk=998)),         # F no multiple of 4
             ([0, 1, 0], [-1] * 3, [-1] * 3, dict(out=b.out_all[1:])),   # out 4 bytes off a 16-byte boundary
             ([0, 1, 0], [-1] * 3, [0, -1, -1], dict(n_slots=0))]
    for row, src, dst, kw in cases:
        with pytest.raises(UmprHipError):
            b.call(row, src, dst, n_fresh, dev, **kw)
        torch.cuda.synchronize()
        assert b.untouched(), (row, src, dst, kw)
    b.call([0, 1, 0], [-1] * 3, [3, -1, -1], n_fresh, dev)          # and the buffers do work
    store, out = b.host()
    assert np.array_equal(out, b.fresh_host[[0, 1, 0]]) and np.array_equal(store[3], b.fresh_host[0]) and (store[:3] == NAN).all()


# ---- models ------------------------------------------------------------------------------------------------------------------
_STATES = {}


def _state(V):
    """One parameter set per number of views (138 M random VGG weights take seconds to draw)."""
    from umpr_amd.synthetic import make_param_state
    if V not in _STATES:
        _STATES[V] = make_param_state(140 + V, 50, 500, V, False, m_scale=0.05)
    return _STATES[V]


def _frozen(V, dev, dtype="fp32", freeze=True):
    cfg = _cfg(review_net_only=False, views=["food", "inside", "outside", "drink"][:V], freeze_vgg=freeze, dtype=dtype)
    return _model(cfg, _state(V), dev)


def _vgg_names(model):
    return [k for k, _ in model.named_parameters() if k.startswith("visual_net.vgg16.")]


@pytest.fixture(scope="module")
def model2(dev):
    """Frozen, two views: shared by the tests that do not change a parameter."""
    return _frozen(2, dev)


def _reset(model, V):
    """The trainable parameters back to their initial values, the VGG left alone (reloading it would empty a store)."""
    P = _state(V)
    with torch.no_grad():
        for k, p in model.named_parameters():
            if p.requires_grad:
                p.copy_(P[k])


# ---- the frozen VGG ---------------------------------------------------------------------------------------------------------------
def test_frozen_vgg_runs_the_inference_path_in_training_mode(dev):
    from umpr_amd.synthetic import make_batch
    frozen, plain = _frozen(1, dev), _frozen(1, dev, freeze=False)
    vgg, ref = frozen.visual_net.vgg16[0], plain.visual_net.vgg16[0]
    images = make_batch(151, 3, 500, 1)[6].reshape(3, 3, 224, 224).to(dev)
    frozen.train()
    calls = vgg._calls
    with torch.enable_grad():
        a = vgg(images)
        b = vgg(images)
    assert not a.requires_grad and a.grad_fn is None and a.dtype == torch.float32 and a.shape == (3, F)
    assert vgg._calls == calls and vgg.forward_calls == 2               # no dropout counter consumed
    frozen.eval()
    with torch.no_grad():
        c = vgg(images)
    plain.eval()
    with torch.no_grad():
        d = ref(images)                                              # the unfrozen stack's eval output, same weights
    assert torch.equal(a, b) and torch.equal(a, c) and torch.equal(a, d)
    assert torch.isfinite(a).all() and float(a.abs().max()) > 0


def test_frozen_backward_and_train_step_leave_the_vgg_alone(dev):
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_batch
    from umpr_amd.train import train_step
    model = _frozen(1, dev)
    batch = make_batch(152, 2, 500, 1)
    model.train()
    pred, loss = model(*batch)
    loss.backward()
    named = dict(model.named_parameters())
    vgg = _vgg_names(model)
    assert len(vgg) == 32 and all(named[k].grad is None for k in vgg)
    trainable = [k for k, p in named.items() if p.requires_grad]
    assert all(named[k].grad is not None and torch.isfinite(named[k].grad).all() for k in trainable)
    before = {k: p.detach().clone() for k, p in named.items()}
    opt = FusedAdam(model, 1e-3, 1e-3)
    train_step(model, opt, batch)
    torch.cuda.synchronize()
    for k, p in model.named_parameters():
        if k in vgg:
            assert torch.equal(p, before[k]) and p.grad is None, k
        elif k == "visual_net.linear.bias":
            # the one trainable parameter no step can move: it cancels in pos_emb - img_emb and neg_emb - img_emb (src/model.py:
            # 221-226), so its gradient is identically zero, and a bias carries no L2 term
            assert float(p.grad.abs().max()) <= 1e-6 * float(named["visual_net.linear.weight"].grad.abs().max())
        elif p.requires_grad:
            assert not torch.equal(p, before[k]), k
    # clipping runs on the shrunken arenas
    clipped = FusedAdam(model, 1e-3, 1e-3, max_grad_norm=0.01)
    train_step(model, clipped, batch)
    st = clipped.clip_stats()
    assert st["seen"] == 1 and st["clipped"] == 1 and st["skipped"] == 0 and np.isfinite(st["norm"]) and st["norm"] > 0.01
    assert all(torch.equal(named[k], before[k]) for k in vgg)


# ---- against the oracle -------------------------------------------------------------------------------------------------------
def _oracle(P, batch, vgg_fn=None):
    """R.umpr_forward with the VGG entries of P not requiring grad: exactly the frozen model.  Returns (P, pred, loss, VGG output)."""
    from oracle import umpr_ref as R
    Pr = {k: (v if ".vgg16." in k else v.clone()) for k, v in P.items()}
    for k, p in Pr.items():
        if k != "embedding.weight" and ".vgg16." not in k:
            p.requires_grad_(True)
    keep = {}
    rp, rl = R.umpr_forward(Pr, batch, review_net_only=False, train=False, aten=True, keep=keep, vgg_fn=vgg_fn)
    rl.backward()
    return Pr, rp.detach(), rl.detach(), keep["vgg_out"].detach()


def _compare(tag, model, pred, loss, Pr, rp, rl):
    check(f"{tag} pred", pred, rp, atol=1e-4)
    check(f"{tag} loss", loss, rl, atol=1e-4)
    seen = 0
    for k, p in model.named_parameters():
        if p.requires_grad:
            check(f"{tag} grad {k}", p.grad, Pr[k].grad, atol=1e-6, rel_to_max=2e-3)
            seen += 1
    assert seen == len([k for k, p in Pr.items() if p.requires_grad]) and seen == 37


@pytest.mark.parametrize("V,Pc", [(1, 1), (2, 2)])
def test_frozen_model_vs_oracle(dev, V, Pc):
    """Predictions and loss to 1e-4, every non-VGG gradient to atol 1e-6 + 2e-3 of its maximum (the bounds test_gpu_parity.py::check
    applies to the full model's text-path gradients): against the oracle's own VGG, and against the oracle fed the HIP VGG's
    output, which judges the head's gradients apart from the VGG's rounding.  At V = 1 also one Adam step."""
    from oracle import umpr_ref as R
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_batch
    from umpr_amd.train import train_step
    P = _state(V)
    batch = make_batch(160 + V, 2, 500, V, Pc)
    model = _frozen(V, dev)
    model.train()
    pred, loss = model(*batch)
    loss.backward()
    Pr, rp, rl, _ = _oracle(P, batch)
    _compare(f"frozen V{V} P{Pc}", model, pred, loss, Pr, rp, rl)
    hip_vgg = model.visual_net.vgg16[0](batch[6].reshape(-1, 3, 224, 224).to(dev)).cpu()
    Ph, hp, hl, fed = _oracle(P, batch, vgg_fn=lambda flat: hip_vgg)
    assert torch.equal(fed, hip_vgg)
    _compare(f"frozen V{V} P{Pc}, HIP VGG output", model, pred, loss, Ph, hp, hl)
    if V == 1:
        opt = FusedAdam(model, 1e-3, 1e-3)
        ropt = R.adam_reference(Pr, 1e-3, 1e-3)
        assert sum(len(g["params"]) for g in ropt.param_groups) == sum(len(g.params) for g in opt.groups)
        train_step(model, opt, batch)
        ropt.step()                   # on the gradients of the backward above: P has not moved since
        for k, p in model.named_parameters():
            if k == "visual_net.linear.bias":
                continue              # its gradient is identically zero (it cancels in pos_emb - img_emb): both sides hold only
                                      # rounding noise, which Adam's first step turns into +-lr at random
            if p.requires_grad:
                # Adam's first step is lr * sign(g): compare where the oracle's gradient is above rounding noise, as
                # test_hidden_sizes_below_the_kernel_width_vs_oracle does
                gr = Pr[k].grad
                big = gr.abs() > 1e-4 * gr.abs().max()
                check(f"frozen stepped {k}", p.detach().cpu()[big], Pr[k].detach()[big], atol=2e-5, rtol=1e-4)
            else:
                assert torch.equal(p.detach().cpu(), P[k]), k


# ---- the store ----------------------------------------------------------------------------------------------------------------
def _collate(store, samples, host=False):
    return batch_loader(samples, resize_on_gpu=not host, store=None if host else store.index)


def _row(store, path):
    s = store.slot_of(path)
    assert 0 <= s < store.slots
    return store.buffer[s * F:(s + 1) * F]


def test_cold_then_warm_pass(dev, photo_set, model2, tmp_path):
    paths = own_copy(photo_set[:3] + photo_set[7:8], tmp_path)              # 500x375, 224x224, 100x80, grey
    samples = samples_for(paths, 3, 2, 1)                                  # 6 photos: p0 p1 p2 p3 p0 p1
    flat = [p for s in samples for v in s[3] for p in v]
    vgg = model2.visual_net.vgg16[0]
    store = FeatureStore(dev, capacity_bytes=8 * 4000 + 100).register(paths)
    assert store.slots == 8 and store.buffer.numel() == 9 * F
    host = batch_loader(samples)[6].reshape(-1, 3, 224, 224).to(dev)
    calls = vgg.forward_calls
    raw = _collate(store, samples)[6]
    assert not raw.hits.any()
    cold = store.features(raw, vgg)
    assert vgg.forward_calls == calls + 1 and cold.shape == (6, F) and cold.dtype == torch.float32 and not cold.requires_grad
    want = vgg(host[:4])                                                   # the compacted miss batch: same images, same order
    for k, p in enumerate(paths):
        assert torch.equal(_row(store, p), want[k]), p
    assert torch.equal(cold, want[[0, 1, 2, 3, 0, 1]])
    s = store.stats()
    assert (s["used"], s["inserts"], s["computed"], s["shared"], s["hits"], s["vgg_calls"]) == (4, 4, 4, 2, 0, 1)
    for p in paths:
        os.remove(p)
    calls = vgg.forward_calls
    raw = _collate(store, samples)[6]                                      # no file is there to be opened
    assert raw.hits.all() and not (raw.descriptors()["rows"] > 0).any() and raw.data.numel() == 6 * 24
    warm = store.features(raw, vgg)
    assert vgg.forward_calls == calls and store.stats()["vgg_calls"] == 1 and store.stats()["hits"] == 6
    assert torch.equal(warm, torch.stack([_row(store, p) for p in flat])) and torch.equal(warm, cold)
    # through the model, and on another stream than the fill
    model2.eval()
    with torch.no_grad():
        second = torch.cuda.Stream(dev)
        with torch.cuda.stream(second):
            pred, loss = model2(*_collate(store, samples))
        second.synchronize()
    assert vgg.forward_calls == calls and torch.isfinite(pred).all() and torch.isfinite(loss)


def test_warm_training_steps_repeat_and_meet_the_oracle(dev, photo_set, tmp_path):
    from umpr_amd.optim import FusedAdam
    from umpr_amd.train import train_step
    paths = own_copy(photo_set[:2], tmp_path)
    samples = samples_for(paths, 2, 1, 1, seed=31)
    model = _frozen(1, dev)
    vgg = model.visual_net.vgg16[0]
    store = FeatureStore(dev, capacity_bytes=4 * 4000).register(paths)
    host = _collate(store, samples, host=True)
    model.train()
    model(*_collate(store, samples))                                       # the cold pass
    for p in paths:
        os.remove(p)
    calls = vgg.forward_calls
    runs = []
    for _ in range(2):
        _reset(model, 1)
        opt = FusedAdam(model, 1e-3, 1e-3)
        batch = _collate(store, samples)
        assert batch[6].hits.all()
        pred, loss = train_step(model, opt, batch)
        torch.cuda.synchronize()
        runs.append((pred.detach().clone(), loss.detach().clone(), {k: v.detach().clone() for k, v in model.state_dict().items()}))
    assert vgg.forward_calls == calls
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k
    assert not torch.equal(runs[0][2]["linear_fusion.0.weight"], _state(1)["linear_fusion.0.weight"].to(dev))
    # a warm forward / backward against the oracle on the host form of the same batch
    _reset(model, 1)
    for p in model.parameters():
        p.grad = None
    pred, loss = model(*_collate(store, samples))
    loss.backward()
    assert vgg.forward_calls == calls
    Pr, rp, rl, _ = _oracle(_state(1), host)
    _compare("warm store", model, pred, loss, Pr, rp, rl)


def test_mixed_pass(dev, photo_set, model2):
    """One batch with hits, first misses, the same id twice, and missing photos."""
    p = photo_set
    vgg = model2.visual_net.vgg16[0]
    store = FeatureStore(dev, capacity_bytes=8 * 4000).register(p[:3] + p[7:10])
    first = _collate(store, samples_for(p[:3], 1, 3, 1))[6]
    store.features(first, vgg)
    held = {q: _row(store, q).clone() for q in p[:3]}
    order = [p[0], p[7], p[1], p[8], p[7], p[2], "unknown", p[11]]         # p[11] does not exist
    samples = samples_for(order, 2, 2, 2)
    calls = vgg.forward_calls
    batch = _collate(store, samples)
    assert batch[6].hits.tolist() == [1, 0, 1, 0, 0, 1, 0, 0]
    got = store.features(batch[6], vgg)
    assert vgg.forward_calls == calls + 2                                  # the two new photos in one call, the zero image in one
    host = batch_loader(samples)[6].reshape(-1, 3, 224, 224).to(dev)
    fresh = vgg(host[[1, 3]])
    zero = vgg(torch.zeros(1, 3, 224, 224, device=dev))
    want = torch.stack([held[p[0]], fresh[0], held[p[1]], fresh[1], fresh[0], held[p[2]], zero[0], zero[0]])
    assert torch.equal(got, want)
    assert torch.equal(_row(store, p[7]), fresh[0]) and torch.equal(_row(store, p[8]), fresh[1])
    assert torch.equal(store.buffer[store.zero_slot * F:], zero[0]) and all(torch.equal(_row(store, q), held[q]) for q in held)
    s = store.stats()
    assert (s["used"], s["inserts"], s["hits"], s["computed"], s["shared"], s["missing"], s["vgg_calls"]) == (5, 5, 3, 5, 1, 2, 3)
    calls = vgg.forward_calls
    batch = _collate(store, samples)
    assert batch[6].hits.tolist() == [1] * 6 + [0, 0]
    assert torch.equal(store.features(batch[6], vgg), want) and vgg.forward_calls == calls     # the zero row is computed once
    model2.eval()
    with torch.no_grad():
        pred, loss = model2(*batch)
    assert vgg.forward_calls == calls and pred.shape == (2,) and torch.isfinite(pred).all()


def test_one_slot_three_photos(dev, photo_set, model2):
    p = photo_set[:3]
    vgg = model2.visual_net.vgg16[0]
    store = FeatureStore(dev, capacity_bytes=4000 + 3999).register(p)
    assert store.slots == 1
    samples = samples_for(p, 1, 3, 1)
    outs = []
    for k in range(3):
        raw = _collate(store, samples)[6]
        assert raw.hits.tolist() == ([0, 0, 0] if k == 0 else [1, 0, 0])
        calls = vgg.forward_calls
        outs.append(store.features(raw, vgg))
        assert vgg.forward_calls == calls + 1
    s = store.stats()
    assert (s["slots"], s["used"], s["inserts"], s["hits"], s["decoded_while_full"], s["computed"]) == (1, 1, 1, 2, 6, 7)
    assert torch.equal(outs[1], outs[2]) and torch.equal(outs[0][0], outs[1][0])
    # two misses per call instead of three: other tiles, other rounding.  tests/test_gpu_parity.py holds the classifier to 1e-4 of
    # the output's maximum against float64 at every row count, so two row counts are within twice that of each other
    check("recomputed rows", outs[1], outs[0], atol=1e-6, rel_to_max=2e-4)


def test_other_vgg_weights_empty_the_store(dev, photo_set):
    from umpr_amd._lib import UmprHipError
    p = photo_set[:2]
    model = _frozen(1, dev)
    vgg = model.visual_net.vgg16[0]
    store = FeatureStore(dev, capacity_bytes=4 * 4000).register(p)
    samples = samples_for(p, 2, 1, 1)
    cold = store.features(_collate(store, samples)[6], vgg)
    stale = _collate(store, samples)[6]
    assert stale.hits.all()
    sd = {k: v.clone() for k, v in model.state_dict().items()}
    sd["visual_net.vgg16.0.classifier.6.bias"] += 1.0
    f0 = vgg_fingerprint(vgg)
    model.load_state_dict(sd)
    assert vgg_fingerprint(vgg) != f0
    with pytest.raises(UmprHipError, match="left to the store, which does not hold it"):
        store.features(stale, vgg)                                         # collated while the old rows were resident
    assert store.stats()["flushes"] == 1 and store.stats()["used"] == 0 and not store.index.resident.any()
    raw = _collate(store, samples)[6]
    assert not raw.hits.any()
    again = store.features(raw, vgg)
    assert not torch.equal(again, cold) and store.stats()["used"] == 2
    assert float((again - cold - 1.0).abs().max()) < 1e-4 * (1.0 + float(cold.abs().max()))     # the bias moved by one
    f1 = vgg_fingerprint(vgg)
    vgg.to("cpu")
    assert vgg_fingerprint(vgg) != f1


def test_refusals(dev, photo_set):
    from umpr_amd._lib import UmprHipError
    from umpr_amd.model import VGG16
    from umpr_amd.synthetic import make_batch
    p = photo_set[:2]
    store = FeatureStore(dev, capacity_bytes=4 * 4000).register(p)
    samples = samples_for(p, 2, 1, 1)
    raw = _collate(store, samples)[6]
    with torch.device("meta"):
        trainable = VGG16()
    with pytest.raises(UmprHipError, match="trainable parameters"):
        store.features(raw, trainable)
    plain = _frozen(1, dev, freeze=False)
    with pytest.raises(UmprHipError, match="feature store reached a model whose VGG trains"):
        plain(*_collate(store, samples))
    assert store.stats()["used"] == 0 and store.stats()["vgg_calls"] == 0
    with pytest.raises(RuntimeError, match="no CPU path"):
        FeatureStore("cpu")


def test_bf16_warm_equals_cold(dev, photo_set, tmp_path):
    paths = own_copy(photo_set[:3], tmp_path)
    samples = samples_for(paths, 3, 1, 1, seed=33)
    model = _frozen(1, dev, dtype="bf16").eval()
    vgg = model.visual_net.vgg16[0]
    store = FeatureStore(dev, capacity_bytes=4 * 4000).register(paths)
    with torch.no_grad():
        cold = model(*_collate(store, samples))
        rows = torch.stack([_row(store, q) for q in paths])
        for q in paths:
            os.remove(q)
        calls = vgg.forward_calls
        batch = _collate(store, samples)
        assert batch[6].hits.all()
        warm = model(*batch)
        feats = store.features(_collate(store, samples)[6], vgg)
    assert vgg.forward_calls == calls
    assert torch.equal(cold[0], warm[0]) and torch.equal(cold[1], warm[1]) and torch.equal(feats, rows)


def test_worker_dataloader_feeds_a_warm_epoch(dev, photo_set, model2):
    from torch.utils.data import DataLoader
    from main import _Collate
    data = samples_for(photo_set, 6, 2, 1, seed=34)
    vgg = model2.visual_net.vgg16[0]
    model2.eval()
    store = FeatureStore(dev, capacity_bytes=16 * 4000).register(photo_set)
    dl = DataLoader(data, batch_size=3, collate_fn=_Collate(False, store=store.index), num_workers=2, pin_memory=True,
                    persistent_workers=True)
    readable = [p for p in photo_set[:10]]
    preds = [[], []]
    with torch.no_grad():
        for epoch in range(2):
            calls = vgg.forward_calls
            for batch in dl:
                raw = batch[6]
                assert raw.is_pinned() and raw.store_key == store.key
                flat = [p for s in data[3 * len(preds[epoch]):3 * len(preds[epoch]) + 3] for v in s[3] for p in v]
                assert raw.hits.tolist() == [int(epoch == 1 and p in readable) for p in flat]
                preds[epoch].append(model2(*batch)[0])
            assert len(preds[epoch]) == 2
            if epoch == 1:
                assert vgg.forward_calls == calls                          # nothing left to compute
    del dl
    assert all(torch.equal(a, b) for a, b in zip(*preds))
    assert store.stats()["inserts"] == 10 and store.stats()["missing"] == 4


def test_evaluate_mse_uses_the_store(dev, photo_set, model2):
    from umpr_amd.train import evaluate_mse
    p = photo_set[:4]
    samples = samples_for(p, 2, 2, 1, seed=35)
    vgg = model2.visual_net.vgg16[0]
    store = FeatureStore(dev, capacity_bytes=8 * 4000).register(p)
    cold = evaluate_mse(model2, [_collate(store, samples)])
    calls = vgg.forward_calls
    warm = evaluate_mse(model2, [_collate(store, samples)])
    assert vgg.forward_calls == calls and store.stats()["hits"] == 4 and store.stats()["used"] == 4
    assert warm == cold and np.isfinite(cold)


def test_main_cli_with_a_frozen_vgg_and_the_feature_store(tmp_path, capsys, monkeypatch):
    """main.py --freeze_vgg True --feature_store_gb X on the tiny CSV corpus, in-process as tests/test_gpu_e2e.py runs the CLI:
    the store is built instead of the photo store, fills in the first validation pass, and serves training, validation and the
    test from then on; without --freeze_vgg True the flag is refused before anything is built."""
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
            "--views", "inside", "--learning_rate", "1e-3", "--model_path", str(tmp_path / "m.pt"), "--feature_store_gb", "0.001",
            "--photo_store_gb", "0.01"]
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main")
    monkeypatch.setattr(sys, "argv", argv)
    with pytest.raises(SystemExit, match="--feature_store_gb needs --freeze_vgg True"):
        main.main()
    monkeypatch.setattr(sys, "argv", argv + ["--freeze_vgg", "True"])
    main.main()
    out = capsys.readouterr().out
    assert "Feature store: 250 slots of 4000 B" in out and "it replaces the photo store" in out and "Photo store" not in out
    assert "Initial validation mse is" in out and "Test end, test mse is" in out, out[-2000:]
    stats = [eval(line.split(": ", 1)[1]) for line in out.splitlines() if "Feature store after" in line]
    assert len(stats) == 2
    train, test = stats
    assert 0 < train["used"] == train["inserts"] == train["computed"] <= len(ids[::2])      # every photo went through the VGG once
    assert train["hits"] > 0 and train["missing"] > 0 and train["flushes"] == 0
    assert test["computed"] == train["computed"] and test["hits"] > train["hits"]            # the test pass computed nothing
    mse = float(out.strip().split("test mse is")[-1].split()[0])
    assert mse == mse and mse < 100.0
