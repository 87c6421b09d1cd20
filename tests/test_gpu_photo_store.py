"""Device-resident photo store (umpr_amd/photos.py::PhotoStore, umpr_photo_fetch_u8 in csrc/photos.hip) against the host form of
the loader: cold, mixed and warm passes, a full store, a training step, the bf16 eval forward and a worker DataLoader are all
bit-identical, with the photo files deleted once they are resident; bad slot arrays are argument errors."""
import os

import numpy as np
import pytest
import torch

from test_gpu_photos import _cfg, _model, dev  # noqa: F401  (module fixture)
from test_photo_pack import photo_set, samples_for  # noqa: F401  (module fixture)
from test_photo_store import LUT, own_copy, slot_bytes
from umpr_amd.data import batch_loader
from umpr_amd.photos import PhotoStore, RawPhotos, decode_for_gpu

pytestmark = pytest.mark.gpu


def _through(store, samples, size=(224, 224)):
    raw = batch_loader(samples, photo_size=size, resize_on_gpu=True, store=store.index)[6]
    return raw, raw.to(store.device)


def _slot_image(store, path):
    s, n = store.slot_of(path), 3 * store.size[0] * store.size[1]
    assert s >= 0
    return store.buffer[s * store.slot_bytes:s * store.slot_bytes + n].cpu().numpy()


@pytest.mark.parametrize("B,size", [(3, (224, 224)), (9, (224, 224)), (3, (37, 23))])
def test_passes_through_the_store_equal_the_host_form(dev, photo_set, tmp_path, B, size):
    """Pass 1 decodes (and fills the store), pass 2 runs with the files gone.  B = 9 at V = 4, P = 2 is 72 photos, two chunks of
    kernel arguments; there every other photo is resident before pass 1, so hits and misses fall on both sides of photo 64."""
    V, P = 4, 2
    set_ = photo_set if size[0] == size[1] else photo_set[:-3]     # the host form cannot stack non-square missing photos
    if B == 9:
        set_ = set_[:6] + set_[7:]                                 # without the 4000 x 3000 photo, to stay quick
    paths = own_copy(set_, tmp_path)
    readable = [p for p in paths if os.path.exists(p) and not p.endswith("truncated.jpg")]
    samples = samples_for(paths, B, V, P, seed=B)
    flat = [p for s in samples for view in s[3] for p in view]
    want = batch_loader(samples, photo_size=size)[6].to(dev)
    store = PhotoStore(dev, size, capacity_bytes=16 * slot_bytes(size)).register(paths)
    assert store.slots == 16 and store.slot_bytes == slot_bytes(size)
    primed = readable[::2] if B == 9 else []
    if primed:
        _through(store, samples_for(primed, 1, len(primed), 1), size)
        assert store.stats()["used"] == len(primed)
    raw, got = _through(store, samples, size)
    assert raw.hits.tolist() == [int(p in primed) for p in flat]
    if B == 9:
        for side in (flat[:64], flat[64:]):
            assert any(p in primed for p in side) and any(p in readable and p not in primed for p in side)
    assert got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
    assert torch.equal(got, want)
    assert store.stats()["used"] == len(readable) and store.stats()["inserts"] == len(readable)
    for p in readable:
        os.remove(p)
    raw2, got2 = _through(store, samples, size)
    assert raw2.hits.tolist() == [int(p in readable) for p in flat]
    assert torch.equal(got2, want)
    pinned = raw2.pin_memory()
    assert pinned.is_pinned() and torch.equal(pinned.hits, raw2.hits) and pinned.store_key == store.key
    got3 = pinned.to(dev, non_blocking=True)
    torch.cuda.synchronize()
    assert torch.equal(got3, want)
    host = want.cpu().numpy().reshape(len(flat), -1)
    for p in readable:                # the store holds the host resize's bytes, planar
        k = flat.index(p)
        byte = np.searchsorted(LUT, host[k])
        assert np.array_equal(LUT[byte], host[k]) and np.array_equal(_slot_image(store, p), byte), p


def test_mixed_pass(dev, photo_set):
    """Half the photos resident, half new, one of the new ones twice in the batch."""
    p = photo_set[:6]
    store = PhotoStore(dev, capacity_bytes=8 * slot_bytes((224, 224))).register(p)
    _through(store, samples_for(p[:3], 1, 3, 1))
    order = [p[0], p[3], p[1], p[4], p[3], p[2], p[5], "unknown"]
    samples = samples_for(order, 1, 4, 2)
    raw, got = _through(store, samples)
    assert raw.hits.tolist() == [1, 0, 1, 0, 0, 1, 0, 0]
    assert torch.equal(got, batch_loader(samples)[6].to(dev))
    assert store.stats() == dict(slots=8, used=6, hits=3, inserts=6, decoded_while_full=0, unregistered=0,
                                 bytes=8 * slot_bytes((224, 224)))
    raw, got2 = _through(store, samples)
    assert raw.hits.tolist() == [1] * 7 + [0] and torch.equal(got2, got)


def test_full_store(dev, photo_set):
    p = photo_set[:5]
    size = (224, 224)
    store = PhotoStore(dev, size, capacity_bytes=2 * slot_bytes(size) + 100).register(p)
    samples = samples_for(p, 5, 1, 1)
    want = batch_loader(samples)[6].to(dev)
    for k in range(3):
        raw, got = _through(store, samples)
        assert raw.hits.tolist() == ([0] * 5 if k == 0 else [1, 1, 0, 0, 0])
        assert torch.equal(got, want)
    s = store.stats()
    assert (s["slots"], s["used"], s["inserts"], s["hits"], s["decoded_while_full"]) == (2, 2, 2, 4, 9)


def test_bad_slot_arrays_are_argument_errors(dev, photo_set):
    from umpr_amd._lib import UmprHipError, lib
    size, n_slots = (224, 224), 4
    dec = [decode_for_gpu(p) for p in photo_set[:3]]
    full = RawPhotos.pack(dec, (1, 1, 3), size)
    holed = RawPhotos.pack([dec[0], None, dec[2]], (1, 1, 3), size)
    buf = torch.zeros(n_slots * slot_bytes(size), dtype=torch.uint8, device=dev)
    want = full.to(dev)

    def fetch(raw, src, dst, store=buf):
        src, dst = np.asarray(src, dtype=np.int32), np.asarray(dst, dtype=np.int32)
        out = torch.empty(raw.shape, dtype=torch.float32, device=dev)
        packed = raw.data.to(dev)
        lib().call("umpr_photo_fetch_u8", packed, packed.numel(), raw.data, src.ctypes.data, dst.ctypes.data, 3, 224, 224, store,
                   n_slots, out, torch.cuda.current_stream(dev).cuda_stream)
        return out

    assert torch.equal(fetch(full, [-1] * 3, [2, -1, 0]), want)
    assert torch.equal(fetch(holed, [-1, 0, -1], [-1] * 3)[0, 0, 1], want[0, 0, 2])       # slot 0 holds photo 2
    cases = [(full, [-1] * 3, [-1, n_slots, -1]),        # dst_slot out of range
             (holed, [-1, n_slots, -1], [-1] * 3),       # src_slot out of range
             (full, [-1] * 3, [1, -1, 1]),               # one dst_slot twice
             (holed, [-1, 1, -1], [1, -1, -1]),          # a dst_slot that is read in the same call
             (full, [0, -1, -1], [-1] * 3),              # a hit with a non-empty descriptor
             (holed, [-1] * 3, [-1, 3, -1]),             # a dst_slot on a 0 x 0 descriptor
             (full, [-1] * 3, [1, -1, -1], None),        # null store, slots in use
             (holed, [-1, 0, -1], [-1] * 3, None)]
    for case in cases:
        with pytest.raises(UmprHipError):
            fetch(*case)
    torch.cuda.synchronize()
    assert torch.equal(fetch(full, [-1] * 3, [-1] * 3, None), want)          # no slot in use: no store needed
    got = fetch(holed, [-1, 2, -1], [-1, -1, 1])
    assert torch.equal(got[0, 0, 1], want[0, 0, 0]) and torch.equal(got[0, 0, 0], want[0, 0, 0])
    assert torch.equal(got[0, 0, 2], want[0, 0, 2])


def test_full_model_train_step_on_hits_is_identical(dev, photo_set):
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_param_state
    from umpr_amd.train import train_step
    V, Pc = 2, 1
    samples = samples_for(photo_set, 3, V, Pc, seed=21)
    cfg = _cfg(review_net_only=False, views=["food", "inside"], photo_count=Pc)
    P = make_param_state(131, 50, 500, V, False, m_scale=0.05)
    store = PhotoStore(dev, capacity_bytes=8 * slot_bytes((224, 224))).register(p for s in samples for v in s[3] for p in v)
    _through(store, samples)
    runs = []
    for warm in (False, True):
        batch = batch_loader(samples, resize_on_gpu=warm, store=store.index if warm else None)
        if warm:
            assert batch[6].hits.all() and not (batch[6].descriptors()["rows"] > 0).any()
        m = _model(cfg, P, dev)
        opt = FusedAdam(m, 1e-3, 1e-3)
        pred, loss = train_step(m, opt, batch)
        torch.cuda.synchronize()
        runs.append((pred.detach().clone(), loss.detach().clone(), {k: v.detach().clone() for k, v in m.state_dict().items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def test_bf16_eval_forward_on_hits_is_identical(dev, photo_set):
    from umpr_amd.synthetic import make_param_state
    V, Pc = 1, 2
    samples = samples_for(photo_set, 3, V, Pc, seed=22)
    cfg = _cfg(review_net_only=False, views=["food"], photo_count=Pc, dtype="bf16")
    P = make_param_state(132, 50, 500, V, False, m_scale=0.05)
    m = _model(cfg, P, dev).eval()
    store = PhotoStore(dev, capacity_bytes=8 * slot_bytes((224, 224))).register(p for s in samples for v in s[3] for p in v)
    _through(store, samples)
    outs = []
    with torch.no_grad():
        for warm in (False, True):
            batch = batch_loader(samples, resize_on_gpu=warm, store=store.index if warm else None)
            assert not warm or batch[6].hits.all()
            pred, loss = m(*batch)
            outs.append((pred.clone(), loss.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_worker_dataloader_with_the_store_feeds_model(dev, photo_set):
    """main.py's collate with a store, DataLoader(num_workers=2, pin_memory=True, persistent_workers=True): the second epoch's
    batches arrive as hits (the workers see the bytes the first epoch set) and the eval outputs equal the host form's."""
    from torch.utils.data import DataLoader
    from main import _Collate
    from umpr_amd.synthetic import make_param_state
    V, Pc = 1, 1
    data = samples_for(photo_set, 8, V, Pc, seed=23)
    cfg = _cfg(review_net_only=False, views=["food"], photo_count=Pc)
    P = make_param_state(133, 50, 500, V, False, m_scale=0.05)
    m = _model(cfg, P, dev).eval()
    store = PhotoStore(dev, capacity_bytes=8 * slot_bytes((224, 224))).register(photo_set)
    dl = DataLoader(data, batch_size=3, collate_fn=_Collate(False, store=store.index), num_workers=2, pin_memory=True,
                    persistent_workers=True)
    ref = []
    with torch.no_grad():
        for k in range(3):
            ref.append(m(*batch_loader(data[3 * k:3 * k + 3])))
        for epoch in range(2):
            n = 0
            for k, batch in enumerate(dl):
                raw = batch[6]
                assert isinstance(raw, RawPhotos) and raw.is_pinned() and raw.store_key == store.key
                assert raw.hits.tolist() == [epoch] * len(raw.hits)
                pred, loss = m(*batch)
                assert torch.equal(pred, ref[k][0]) and torch.equal(loss, ref[k][1])
                n += 1
            assert n == 3
    del dl
    assert store.stats()["inserts"] == 8 and store.stats()["hits"] == 8


def test_fetch_on_a_second_stream_right_after_an_insert(dev, photo_set):
    p = photo_set[:6] + photo_set[7:10]
    samples = samples_for(p, 1, 3, 3)
    want = batch_loader(samples)[6].to(dev)
    store = PhotoStore(dev, capacity_bytes=9 * slot_bytes((224, 224))).register(p)
    warm_up = batch_loader(samples, resize_on_gpu=True, store=store.index)[6]
    second = torch.cuda.Stream(dev)
    cold = warm_up.to(dev)                                   # fills nine slots on the current stream ...
    warm = batch_loader(samples, resize_on_gpu=True, store=store.index)[6]
    assert warm.hits.all()
    with torch.cuda.stream(second):                          # ... which the other stream reads at once
        got = warm.to(dev)
    second.synchronize()
    torch.cuda.synchronize()
    assert torch.equal(got, want) and torch.equal(cold, want)
