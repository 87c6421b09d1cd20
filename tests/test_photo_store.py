"""Device-resident photo store (umpr_amd/photos.py::PhotoStore, csrc/photos.hip::umpr_photo_fetch_u8), host half: ids, the
collate that leaves resident photos undecoded, and the planning of which photo reads or fills which slot.  `fetch_in_numpy`
restates umpr_photo_fetch_u8 reading nothing but the packed buffer, the slot arrays and a uint8 store; no GPU needed."""
import functools
import os
import pickle
import shutil

import numpy as np
import pytest
import torch

from test_photo_pack import kernel_in_numpy, photo_set, samples_for  # noqa: F401  (module fixture)
from umpr_amd.data import batch_loader, resize_bilinear_u8
from umpr_amd.photos import PhotoTable, RawPhotos

LUT = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


def slot_bytes(size):
    return -(-3 * size[0] * size[1] // 16) * 16


def fetch_in_numpy(raw, src, dst, store, n_slots):
    """What umpr_photo_fetch_u8 computes and leaves in `store` (uint8 [n_slots * slot_bytes], updated in place)."""
    dw, dh = raw.size
    n, sb = 3 * dh * dw, slot_bytes(raw.size)
    desc = raw.descriptors()
    assert len(src) == len(dst) == len(desc) and store.dtype == np.uint8 and store.shape == (n_slots * sb,)
    used = np.concatenate([src[src >= 0], dst[dst >= 0]])
    assert used.size == 0 or used.max() < n_slots
    assert len(set(dst[dst >= 0])) == (dst >= 0).sum() and not set(dst[dst >= 0]) & set(src[src >= 0])
    out = kernel_in_numpy(raw).reshape(len(desc), n)                  # the misses; zeros where the descriptor is 0 x 0
    for i in range(len(desc)):
        if src[i] >= 0:
            assert desc["rows"][i] == 0 and desc["cols"][i] == 0 and dst[i] < 0
            out[i] = LUT[store[src[i] * sb:src[i] * sb + n]]
        elif dst[i] >= 0:
            assert desc["rows"][i] > 0
            byte = np.searchsorted(LUT, out[i])                       # the uint8 behind each float: LUT is strictly increasing
            assert np.array_equal(LUT[byte], out[i])
            store[dst[i] * sb:dst[i] * sb + n] = byte
    return out.reshape(raw.shape)


def own_copy(paths, tmp_path):
    """The readable photos of `paths` copied to tmp_path (tests that delete files never touch the shared set)."""
    return [shutil.copy(p, tmp_path) if p != "unknown" and not p.endswith("does_not_exist.jpg") else p for p in paths]


def test_ids_are_dense_and_stable():
    t = PhotoTable(max_photos=5)
    t.register(["a.jpg", "b.jpg", "unknown", "a.jpg"])
    assert [t.id_of(p) for p in ("a.jpg", "b.jpg", "unknown", "c.jpg")] == [0, 1, -1, -1]
    t.register(["c.jpg", "b.jpg", "d.jpg", "e.jpg", "f.jpg", "g.jpg", "unknown"])       # later call, e.g. the test set
    assert [t.id_of(p) for p in ("a.jpg", "b.jpg", "c.jpg", "d.jpg", "e.jpg")] == [0, 1, 2, 3, 4]
    assert t.id_of("f.jpg") == -1 and t.id_of("g.jpg") == -1 and t.id_of("unknown") == -1      # past max_photos
    assert t.stats()["unregistered"] == 2
    ids, hits = t.index.lookup(["b.jpg", "unknown", "g.jpg", "e.jpg"])
    assert ids.dtype == np.int32 and list(ids) == [1, -1, -1, 4] and not hits.any()
    assert t.index.resident.is_shared() and t.index.resident.numel() == 5
    assert t.slot_of("a.jpg") == -1


def test_collate_with_nothing_resident_is_the_gpu_form(photo_set):
    samples = samples_for(photo_set, 2, 4, 2)
    t = PhotoTable().register(photo_set)
    plain = batch_loader(samples, resize_on_gpu=True)
    with_store = batch_loader(samples, resize_on_gpu=True, store=t.index)
    assert plain[6].ids is None and plain[6].hits is None and plain[6].store_key is None
    raw = with_store[6]
    assert torch.equal(raw.data, plain[6].data) and raw.shape == plain[6].shape
    flat = [p for s in samples for view in s[3] for p in view]
    assert raw.ids.dtype == torch.int32 and raw.ids.tolist() == [t.id_of(p) for p in flat]
    assert raw.hits.dtype == torch.uint8 and not raw.hits.any() and raw.store_key == t.key
    for a, b in zip(plain[:6] + plain[7:], with_store[:6] + with_store[7:]):
        assert torch.equal(a, b)


def test_collate_leaves_resident_photos_unopened(photo_set, tmp_path):
    paths = own_copy(photo_set[:6], tmp_path)
    samples = samples_for(paths, 2, 3, 1)
    t = PhotoTable().register(paths)
    before = batch_loader(samples, resize_on_gpu=True, store=t.index)[6]
    gone = [paths[1], paths[4]]
    for p in gone:
        t.index.resident[t.id_of(p)] = 1
        os.remove(p)
    raw = batch_loader(samples, resize_on_gpu=True, store=t.index)[6]
    flat = [p for s in samples for view in s[3] for p in view]
    assert raw.hits.tolist() == [int(p in gone) for p in flat] and torch.equal(raw.ids, before.ids)
    d, d0 = raw.descriptors(), before.descriptors()
    tap_bytes = 16 * (224 + 224)
    for k, p in enumerate(flat):
        if p in gone:
            assert d["rows"][k] == 0 and d["cols"][k] == 0
        else:       # same photo, same bytes (the offsets moved up)
            assert (d["rows"][k], d["cols"][k]) == (d0["rows"][k], d0["cols"][k]) and d["rows"][k] > 0
            nb = 3 * int(d["rows"][k]) * int(d["cols"][k])
            assert torch.equal(raw.data[d["pixels"][k]:d["pixels"][k] + nb], before.data[d0["pixels"][k]:d0["pixels"][k] + nb])
            assert torch.equal(raw.data[d["taps"][k]:d["taps"][k] + tap_bytes], before.data[d0["taps"][k]:d0["taps"][k] + tap_bytes])
    # a deleted photo that is NOT marked resident is opened, fails, and is a missing photo
    os.remove(paths[2])
    raw = batch_loader(samples, resize_on_gpu=True, store=t.index)[6]
    assert not raw.hits[flat.index(paths[2])] and raw.descriptors()["rows"][flat.index(paths[2])] == 0


@pytest.mark.parametrize("size", [(224, 224), (37, 23)])
def test_two_passes_in_numpy_equal_the_host_form(photo_set, size):
    """Pass 1 decodes and fills the store, pass 2 reads it; both equal the host form.  3*37*23 = 2553 is no multiple of 16."""
    V, P = 4, 2
    set_ = photo_set if size[0] == size[1] else photo_set[:-3]     # the host form cannot stack non-square missing photos
    B = -(-len(set_) // (V * P))
    samples = samples_for(set_, B, V, P)
    flat = [p for s in samples for view in s[3] for p in view]
    host = batch_loader(samples, photo_size=size)[6].numpy()
    n_slots, sb = 12, slot_bytes(size)
    assert sb % 16 == 0 and 0 <= sb - 3 * size[0] * size[1] < 16 and (sb == 3 * size[0] * size[1]) == (size == (224, 224))
    t = PhotoTable(size, n_slots).register(set_)
    store = np.full(n_slots * sb, 0xA5, dtype=np.uint8)
    raw = batch_loader(samples, photo_size=size, resize_on_gpu=True, store=t.index)[6]
    src, dst, full = t.plan(raw)
    assert (src < 0).all() and full == 0
    readable = [p for p in set_ if p not in photo_set[-3:]]
    assert sorted(dst[dst >= 0]) == list(range(len(readable)))
    assert np.array_equal(fetch_in_numpy(raw, src, dst, store, n_slots), host)
    assert t.commit(raw, src, dst, full) == len(readable)
    from PIL import Image
    for p in readable:
        with Image.open(p) as im:
            want = resize_bilinear_u8(np.asarray(im.convert("RGB"), dtype=np.uint8), size).transpose(2, 0, 1)
        s = t.slot_of(p)
        assert 0 <= s < len(readable)
        assert np.array_equal(store[s * sb:s * sb + want.size], want.reshape(-1)), p
        assert (store[s * sb + want.size:(s + 1) * sb] == 0xA5).all()            # the padding is never written
    raw2 = batch_loader(samples, photo_size=size, resize_on_gpu=True, store=t.index)[6]
    assert raw2.hits.tolist() == [int(p in readable) for p in flat]
    assert raw2.data.numel() == -(-len(flat) * 24 // 16) * 16                   # descriptors only: no pixels, no tables
    src2, dst2, full2 = t.plan(raw2)
    assert (dst2 < 0).all() and full2 == 0 and [s >= 0 for s in src2] == [p in readable for p in flat]
    kept = store.copy()
    assert np.array_equal(fetch_in_numpy(raw2, src2, dst2, store, n_slots), host)
    assert np.array_equal(store, kept)
    t.commit(raw2, src2, dst2, full2)
    assert t.stats() == dict(slots=n_slots, used=len(readable), hits=int(raw2.hits.sum()), inserts=len(readable),
                             decoded_while_full=0, unregistered=0)


def test_two_slots_five_photos(photo_set):
    paths = photo_set[:5]
    size, n_slots = (37, 23), 2
    t = PhotoTable(size, n_slots).register(paths)
    store = np.zeros(n_slots * slot_bytes(size), dtype=np.uint8)
    samples = samples_for(paths, 5, 1, 1)
    host = batch_loader(samples, photo_size=size)[6].numpy()
    for k in range(3):
        raw = batch_loader(samples, photo_size=size, resize_on_gpu=True, store=t.index)[6]
        src, dst, full = t.plan(raw)
        assert list(dst) == ([0, 1, -1, -1, -1] if k == 0 else [-1] * 5)
        assert list(src) == ([-1] * 5 if k == 0 else [0, 1, -1, -1, -1]) and full == 3
        assert raw.hits.tolist() == ([0] * 5 if k == 0 else [1, 1, 0, 0, 0])
        assert np.array_equal(fetch_in_numpy(raw, src, dst, store, n_slots), host)
        t.commit(raw, src, dst, full)
    assert t.stats() == dict(slots=2, used=2, hits=4, inserts=2, decoded_while_full=9, unregistered=0)
    assert t.index.resident[:5].tolist() == [1, 1, 0, 0, 0]


def test_duplicate_in_a_batch_gets_one_slot(photo_set):
    size = (37, 23)
    order = [photo_set[0], photo_set[2], photo_set[0], "unknown", photo_set[2], photo_set[11]]     # [11]: does not exist
    t = PhotoTable(size, 4).register(order)
    samples = samples_for(order, 1, 3, 2)
    raw = batch_loader(samples, photo_size=size, resize_on_gpu=True, store=t.index)[6]
    assert raw.ids.tolist() == [0, 1, 0, -1, 1, 2]
    src, dst, full = t.plan(raw)
    assert list(dst) == [0, 1, -1, -1, -1, -1] and (src < 0).all() and full == 0     # unreadable photos are not cached
    store = np.zeros(4 * slot_bytes(size), dtype=np.uint8)
    got = fetch_in_numpy(raw, src, dst, store, 4)
    assert np.array_equal(got, kernel_in_numpy(raw)) and np.array_equal(got[0, 0, 0], got[0, 1, 0])
    t.commit(raw, src, dst, full)
    # a batch decoded by a worker whose view lagged: resident meanwhile, arrives with pixels, is only resized
    src, dst, full = t.plan(raw)
    assert (src < 0).all() and (dst < 0).all() and full == 0
    assert t.stats()["used"] == 2 and t.index.resident[:3].tolist() == [1, 1, 0]


def test_workers_see_resident_bytes_set_by_the_parent(photo_set):
    """DataLoader workers (persistent: started once, before the bytes are set) read the shared-memory bytes."""
    from torch.utils.data import DataLoader
    paths = photo_set[:4]
    size = (37, 23)
    t = PhotoTable(size, 3).register(paths)
    data = samples_for(paths, 4, 1, 1)
    dl = DataLoader(data, batch_size=2, num_workers=2, persistent_workers=True,
                    collate_fn=functools.partial(batch_loader, photo_size=size, resize_on_gpu=True, store=t.index))
    store = np.zeros(3 * slot_bytes(size), dtype=np.uint8)
    host = [batch_loader(data[k:k + 2], photo_size=size)[6].numpy() for k in (0, 2)]
    first = []
    for k, batch in enumerate(dl):
        raw = batch[6]
        assert isinstance(raw, RawPhotos) and raw.store_key == t.key and raw.ids.tolist() == [2 * k, 2 * k + 1]
        assert not raw.hits.any() and np.array_equal(kernel_in_numpy(raw), host[k])
        first.append(raw)
    src, dst, full = t.plan(first[0])                 # between the epochs the parent makes the first batch's photos resident
    assert list(dst) == [0, 1] and np.array_equal(fetch_in_numpy(first[0], src, dst, store, 3), host[0])
    assert t.commit(first[0], src, dst, full) == 2
    for k, batch in enumerate(dl):
        raw = batch[6]
        assert raw.hits.tolist() == ([1, 1] if k == 0 else [0, 0])
        assert (raw.descriptors()["rows"] == 0).all() == (k == 0)
        src, dst, full = t.plan(raw)
        assert list(src) == ([0, 1] if k == 0 else [-1, -1]) and list(dst) == ([-1, -1] if k == 0 else [2, -1])
        assert np.array_equal(fetch_in_numpy(raw, src, dst, store, 3), host[k])
    del dl


def test_pickling_keeps_ids_hits_and_key(photo_set):
    t = PhotoTable().register(photo_set[:4])
    t.index.resident[1] = 1
    raw = batch_loader(samples_for(photo_set[:4], 2, 1, 2), resize_on_gpu=True, store=t.index)[6]
    back = pickle.loads(pickle.dumps(raw))
    assert back.shape == raw.shape and torch.equal(back.data, raw.data)
    assert torch.equal(back.ids, raw.ids) and torch.equal(back.hits, raw.hits) and back.hits.tolist() == [0, 1, 0, 0]
    assert back.store_key == raw.store_key == t.key
    index = pickle.loads(pickle.dumps(t.index))
    assert index.ids == t.index.ids and index.key == t.key and index.size == t.index.size
    assert torch.equal(index.resident, t.index.resident)


def test_store_batches_refuse_the_cpu(photo_set):
    t = PhotoTable().register(photo_set[:2])
    raw = batch_loader(samples_for(photo_set[:2], 1, 1, 2), resize_on_gpu=True, store=t.index)[6]
    with pytest.raises(RuntimeError, match="no CPU path"):
        raw.to("cpu")


def test_hits_without_a_registered_store_raise(photo_set):
    from umpr_amd._lib import UmprHipError
    t = PhotoTable().register(photo_set[:2])                   # a table alone is no store: nothing holds the pixels
    t.index.resident[0] = 1
    raw = batch_loader(samples_for(photo_set[:2], 1, 1, 2), resize_on_gpu=True, store=t.index)[6]
    assert raw.hits.tolist() == [1, 0]
    with pytest.raises(UmprHipError, match="not registered"):
        raw.to("cuda:0")
