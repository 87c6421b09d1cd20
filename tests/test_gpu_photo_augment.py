"""Augmented photo fetch (umpr_photo_fetch_augment_u8 in csrc/photos.hip, photos.PhotoAugment, UMPR(photo_flip=, photo_crop=)) bit
for bit against tests/photo_augment_reference.py: explicit windows through the C ABI at the smallest sizes that take every path,
store and scratch slots, refusals before any launch, and the model - a training step, evaluation, an exact resume."""
import numpy as np
import pytest
import torch

from photo_augment_reference import LUT, augment_batch
from test_gpu_photos import _cfg, _model, dev  # noqa: F401  (module fixture)
from test_photo_pack import photo_set, samples_for  # noqa: F401  (module fixture)
from test_photo_store import slot_bytes
from umpr_amd.data import batch_loader, resize_bilinear_u8
from umpr_amd.photos import PhotoAugment, PhotoStore, RawPhotos, tap_tables

pytestmark = pytest.mark.gpu

GUARD = 4096          # sentinel bytes behind every device buffer
SENTINEL = 0xA5


def _sources(n, size, seed):
    """n random source photos (sizes around `size`, some smaller, some larger) as decode_for_gpu would hand them over, with the
    resized uint8 image U of each."""
    from umpr_amd.data import _column_taps, _row_taps
    g = np.random.default_rng(seed)
    dw, dh = size
    dec, U = [], []
    for k in range(n):
        h, w = int(g.integers(1, 2 * dh + 2)), int(g.integers(1, 2 * dw + 2))
        rgb = g.integers(0, 256, (h, w, 3), dtype=np.uint8)
        x0, x1, a0, a1 = _column_taps(dw, w)
        y0, y1, b0, b1 = _row_taps(dh, h)
        rows, cols = np.unique(np.concatenate([y0, y1])), np.unique(np.concatenate([x0, x1]))
        taps = np.concatenate([np.searchsorted(cols, x0), np.searchsorted(cols, x1), a0, a1,
                               np.searchsorted(rows, y0), np.searchsorted(rows, y1), b0, b1]).astype(np.int32)
        dec.append((np.ascontiguousarray(rgb[rows][:, cols]), taps))
        U.append(resize_bilinear_u8(rgb, size))
    return dec, U


class _Rig:
    """Device buffers of one size with guard bands, and the call.  `out`, `store` and `scratch` start NaN / sentinel filled."""

    def __init__(self, dev, size, n, n_slots, n_scratch):
        self.dev, self.size, self.n, self.n_slots, self.n_scratch = dev, size, n, n_slots, n_scratch
        dw, dh = size
        self.sb = slot_bytes(size)
        self.per = 3 * dh * dw
        self._out = torch.full((n * self.per + GUARD // 4,), float("nan"), device=dev)
        self.out = self._out[:n * self.per]
        self._store = torch.full((n_slots * self.sb + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        self._scratch = torch.full((n_scratch * self.sb + GUARD,), SENTINEL, dtype=torch.uint8, device=dev)
        self.xt, self.yt = (torch.from_numpy(t).to(dev) for t in tap_tables(size))

    def slot(self, k):
        return self._store[k * self.sb:k * self.sb + self.per].cpu().numpy()

    def fill_slot(self, k, U):
        self._store[k * self.sb:k * self.sb + self.per] = torch.from_numpy(np.ascontiguousarray(U.transpose(2, 0, 1)).reshape(-1)).to(self.dev)

    def call(self, raw, src, dst, crop, fn="umpr_photo_fetch_augment_u8", **over):
        from umpr_amd._lib import lib
        dw, dh = self.size
        src, dst = np.asarray(src, dtype=np.int32), np.asarray(dst, dtype=np.int32)
        crop = None if crop is None else np.ascontiguousarray(np.asarray(crop, dtype=np.int32).reshape(-1, 5))
        packed = raw.data.to(self.dev)
        a = dict(store=self._store if self.n_slots else None, n_slots=self.n_slots, scratch=self._scratch if self.n_scratch else None,
                 n_scratch=self.n_scratch, xt=self.xt, yt=self.yt, out=self.out, crop=None if crop is None else crop.ctypes.data, n=self.n)
        a.update(over)
        st = torch.cuda.current_stream(self.dev).cuda_stream
        if fn == "umpr_photo_fetch_u8":
            lib().call(fn, packed, packed.numel(), raw.data, src.ctypes.data, dst.ctypes.data, a["n"], dh, dw, a["store"], a["n_slots"],
                       a["out"], st)
        else:
            lib().call(fn, packed, packed.numel(), raw.data, src.ctypes.data, dst.ctypes.data, a["crop"], a["n"], dh, dw, a["store"],
                       a["n_slots"], a["scratch"], a["n_scratch"], a["xt"], a["yt"], a["out"], st)
        torch.cuda.synchronize()
        return self.out.cpu().numpy().reshape(self.n, 3, dh, dw)

    def snapshot(self):
        torch.cuda.synchronize()
        return [t.clone() for t in (self._out, self._store, self._scratch)]

    def unchanged_since(self, snap):
        torch.cuda.synchronize()
        return all(torch.equal(a.view(torch.uint8), b.view(torch.uint8)) for a, b in zip(snap, (self._out, self._store, self._scratch)))

    def guards_intact(self, used_scratch):
        ok = bool(torch.isnan(self._out[self.n * self.per:]).all())
        ok &= bool((self._store[self.n_slots * self.sb:] == SENTINEL).all())
        ok &= bool((self._scratch[used_scratch * self.sb:] == SENTINEL).all())        # unused scratch slots and the band behind them
        for buf, k in ((self._store, self.n_slots), (self._scratch, used_scratch)):
            for s in range(k):                                                        # the padding of a slot is never written
                ok &= bool((buf[s * self.sb + self.per:(s + 1) * self.sb] == SENTINEL).all())
        return ok


def _windows(dw, dh):
    """whole; 1 x 1; 1 x dh; dw x 1; flush right and bottom; a one-pixel margin; odd and even widths - each plain and flipped"""
    w = [(0, 0, dw, dh), (dw // 2, dh // 2, 1, 1), (0, 0, 1, 1), (dw - 1, dh - 1, 1, 1), (dw // 3, 0, 1, dh), (0, dh // 3, dw, 1),
         (dw - 3, dh - 2, 3, 2), (dw - 4, dh - 3, 4, 3), (1, 1, dw - 2, dh - 2), (0, 1, dw - 1, dh - 1), (1, 0, dw - 1, dh - 2),
         (2, 1, 2, 3)]
    assert all(x >= 0 and y >= 0 and x + c <= dw and y + r <= dh for x, y, c, r in w) and {c % 2 for _, _, c, _ in w} == {0, 1}
    return [(*v, f) for v in w for f in (0, 1)]


@pytest.mark.parametrize("size,n_src", [((5, 7), 4), ((37, 23), 4), ((224, 224), 3), ((260, 9), 2), ((259, 10), 2)])
def test_windows_from_scratch_and_from_slots_equal_the_reference(dev, size, n_src):
    """Every window on photos that go through scratch (no store at all), then the same windows on the slots a first call filled.
    (5, 7) is 105 floats per photo - `out` of a photo is 4-byte aligned only, the slot is padded to 112 bytes.  (260, 9) and
    (259, 10) are two tiles of the kernel each way, with and without float4 stores; the whole window there makes the first tile
    stage 257 source columns, one more than the block has threads."""
    dw, dh = size
    dec, U = _sources(n_src, size, seed=dw)
    wins = _windows(dw, dh)
    n = len(wins)
    pick = [k % n_src for k in range(n)]
    raw = RawPhotos.pack([dec[k] for k in pick], (1, 1, n), size)
    want = augment_batch([U[k] for k in pick], wins, size)
    rig = _Rig(dev, size, n, 0, n)
    got = rig.call(raw, [-1] * n, [-1] * n, wins)
    assert np.array_equal(got, want)
    assert rig.guards_intact(n)
    # the first n_src photos fill slots (plain image, byte for byte); every window then reads the slots
    rig = _Rig(dev, size, n_src, n_src + 1, 0)
    first = RawPhotos.pack(dec, (1, 1, n_src), size)
    got = rig.call(first, [-1] * n_src, list(range(n_src)), wins[3:3 + n_src])
    assert np.array_equal(got, augment_batch(U, wins[3:3 + n_src], size))
    for k in range(n_src):
        assert np.array_equal(rig.slot(k), U[k].transpose(2, 0, 1).reshape(-1)), k
    assert (rig.slot(n_src) == SENTINEL).all() and rig.guards_intact(0)
    plain = rig.call(RawPhotos.pack([None] * n_src, (1, 1, n_src), size), list(range(n_src)), [-1] * n_src, None, fn="umpr_photo_fetch_u8")
    assert np.array_equal(plain, np.stack([LUT[u].transpose(2, 0, 1) for u in U]))
    hits = _Rig(dev, size, n, n_src, 0)
    for k in range(n_src):
        hits.fill_slot(k, U[k])
    got = hits.call(RawPhotos.pack([None] * n, (1, 1, n), size), pick, [-1] * n, wins)
    assert np.array_equal(got, want) and hits.guards_intact(0)


@pytest.mark.parametrize("n", [1, 64, 65])
def test_batches_of_one_sixty_four_and_sixty_five(dev, n):
    """65 photos are two launches; random windows, half the photos flipped, an unaligned first photo of `out` is refused elsewhere"""
    size = (8, 8)
    dec, U = _sources(5, size, seed=n)
    g = np.random.default_rng(n)
    cw, ch = g.integers(1, 9, n), g.integers(1, 9, n)
    rec = np.stack([g.integers(0, 9 - cw), g.integers(0, 9 - ch), cw, ch, g.integers(0, 2, n)], axis=1)
    pick = [k % 5 for k in range(n)]
    rig = _Rig(dev, size, n, 0, n)
    got = rig.call(RawPhotos.pack([dec[k] for k in pick], (n, 1, 1), size), [-1] * n, [-1] * n, rec)
    assert np.array_equal(got, augment_batch([U[k] for k in pick], rec, size)) and rig.guards_intact(n)


@pytest.mark.parametrize("size", [(37, 23), (5, 7)])
def test_one_call_mixes_hits_fills_scratch_missing_and_a_repeat(dev, size):
    dw, dh = size
    dec, U = _sources(4, size, seed=3)
    rig = _Rig(dev, size, 7, 4, 2)
    rig.fill_slot(2, U[0])
    #        hit    fill->0  scratch  missing  repeat of 1 (scratch)  fill->3  missing, with a record that would not matter
    photos = [None, dec[1],  dec[2],  None,    dec[1],                dec[3],  None]
    src = [2, -1, -1, -1, -1, -1, -1]
    dst = [-1, 0, -1, -1, -1, 3, -1]
    rec = [(1, 2, dw - 2, dh - 3, 1), (0, 0, dw, dh, 0), (2, 0, 3, dh, 1), (dw - 1, dh - 1, 1, 1, 1), (1, 1, 2, 2, 0),
           (0, 3, dw - 1, 2, 1), (0, 0, 1, 1, 0)]
    images = [U[0], U[1], U[2], None, U[1], U[3], None]
    got = rig.call(RawPhotos.pack(photos, (1, 7, 1), size), src, dst, rec)
    assert np.array_equal(got, augment_batch(images, rec, size))
    assert not got[3].any() and not got[6].any()
    for slot, k in ((0, 1), (2, 0), (3, 3)):                      # a store slot holds the PLAIN image, whatever the window was
        assert np.array_equal(rig.slot(slot), U[k].transpose(2, 0, 1).reshape(-1)), slot
    assert (rig.slot(1) == SENTINEL).all() and rig.guards_intact(2)
    # the plain fetch of the same store still is the host form
    plain = rig.call(RawPhotos.pack([None] * 7, (1, 7, 1), size), [0, 2, 3, 0, 2, 3, 0], [-1] * 7, None, fn="umpr_photo_fetch_u8")
    assert np.array_equal(plain, np.stack([LUT[U[k]].transpose(2, 0, 1) for k in (1, 0, 3, 1, 0, 3, 1)]))


@pytest.mark.parametrize("size", [(224, 224), (5, 7)])
def test_whole_window_is_the_plain_fetch_and_a_flip_is_torch_flip(dev, size):
    dw, dh = size
    dec, U = _sources(3, size, seed=8)
    photos = [dec[0], None, dec[2], dec[1]]
    raw = RawPhotos.pack(photos, (2, 2, 1), size)
    plain = _Rig(dev, size, 4, 0, 0)
    want = torch.from_numpy(plain.call(raw, [-1] * 4, [-1] * 4, None, fn="umpr_photo_fetch_u8").copy())
    assert np.array_equal(want.numpy(), raw.to(dev).cpu().numpy().reshape(4, 3, dh, dw))
    rig = _Rig(dev, size, 4, 0, 3)
    same = rig.call(raw, [-1] * 4, [-1] * 4, [(0, 0, dw, dh, 0)] * 4)
    assert np.array_equal(same.view(np.uint32), want.numpy().view(np.uint32))
    flipped = rig.call(raw, [-1] * 4, [-1] * 4, [(0, 0, dw, dh, 1)] * 4)
    assert np.array_equal(flipped.view(np.uint32), torch.flip(want, dims=[3]).numpy().view(np.uint32))


def test_refusals_name_their_cause_and_touch_nothing(dev):
    from umpr_amd._lib import UmprHipError
    size = (37, 23)
    dw, dh = size
    dec, U = _sources(3, size, seed=4)
    full = RawPhotos.pack(dec, (1, 1, 3), size)
    holed = RawPhotos.pack([dec[0], None, dec[2]], (1, 1, 3), size)
    rig = _Rig(dev, size, 3, 4, 3)
    whole = [(0, 0, dw, dh, 0)] * 3
    rig.fill_slot(1, U[1])
    snap = rig.snapshot()

    def bad_desc(field, value):
        raw = RawPhotos(full.data.clone(), full.geometry, full.size)
        raw.descriptors()[field][1] = value
        return raw

    def rec(k, r):
        out = list(whole)
        out[k] = r
        return out

    none = [-1] * 3
    cases = [  # (raw, src, dst, records, overrides, what the message names)
        (full, none, none, rec(1, (1, 0, dw, dh, 0)), {}, r"photo 1: window 37 x 23 at \(1, 0\) outside the 37 x 23 image"),
        (full, none, none, rec(2, (0, 1, dw, dh, 0)), {}, r"photo 2: window .* outside"),
        (full, none, none, rec(0, (-1, 0, 3, 3, 0)), {}, r"photo 0: window .* outside"),
        (full, none, none, rec(0, (0, -2, 3, 3, 1)), {}, r"photo 0: window .* outside"),
        (full, none, none, rec(0, (2**31 - 1, 0, 2, 2, 0)), {}, r"photo 0: window .* outside"),
        (full, none, none, rec(1, (0, 0, 0, 4, 0)), {}, r"photo 1: empty window 0 x 4"),
        (full, none, none, rec(1, (0, 0, 4, -1, 0)), {}, r"photo 1: empty window 4 x -1"),
        (full, none, none, rec(2, (0, 0, 4, 4, 2)), {}, r"photo 2: flip = 2"),
        (full, none, none, rec(2, (0, 0, 4, 4, -1)), {}, r"photo 2: flip = -1"),
        (holed, [-1, 1, -1], none, rec(1, (0, 0, dw + 1, dh, 0)), {}, r"photo 1: window"),          # a hit's window is checked too
        (full, none, none, whole, dict(n_scratch=2, scratch=rig._scratch), r"photo 2: decoded without a dst_slot, and all 2 scratch"),
        (full, none, [0, -1, -1], whole, dict(n_scratch=1), r"photo 2: decoded without a dst_slot, and all 1 scratch"),
        (full, none, none, whole, dict(n_scratch=3, scratch=None), r"scratch is null"),
        (full, none, none, whole, dict(xt=None), r"null tap table"),
        (full, none, none, whole, dict(yt=None), r"null tap table"),
        (full, none, none, None, {}, r"null crop records"),
        (full, none, [0, 2, 3], whole, dict(scratch=rig._scratch.data_ptr() + 8), r"scratch not 16-byte aligned"),
        (full, none, [0, 2, 3], whole, dict(out=rig.out.data_ptr() + 4), r"store or out not 16-byte aligned"),
        # everything umpr_photo_fetch_u8 refuses
        (full, none, [-1, 4, -1], whole, {}, r"photo 1: slot 4 outside the 4-slot store"),
        (holed, [-1, 4, -1], none, whole, {}, r"photo 1: slot 4 outside"),
        (full, none, [2, -1, 2], whole, {}, r"slot 2 is the dst_slot of two photos"),
        (holed, [-1, 1, -1], [1, -1, -1], whole, {}, r"photo 1 reads slot 1, which this call writes"),
        (full, [1, -1, -1], none, whole, {}, r"photo 0 is read from slot 1 but carries"),
        (holed, none, [-1, 3, -1], whole, {}, r"photo 1 has no source to fill slot 3"),
        (full, none, [0, -1, -1], whole, dict(store=None, n_slots=0), r"photo 0 uses a slot but the store is null"),
        (bad_desc("pixels", full.data.numel() - 10), none, [0, 2, 3], whole, {}, r"photo 1: .* pixels at byte .* outside"),
        (bad_desc("taps", int(full.descriptors()["taps"][1]) + 2), none, [0, 2, 3], whole, {}, r"photo 1: tap tables"),
        (bad_desc("cols", -3), none, [0, 2, 3], whole, {}, r"photo 1 has a .* source"),
        (full, none, none, whole, dict(n=-1), r"n_photos = -1"),
    ]
    for raw, src, dst, records, over, text in cases:
        with pytest.raises(UmprHipError, match="photo_fetch_augment_u8: .*" + text):
            rig.call(raw, src, dst, records, **over)
        assert rig.unchanged_since(snap), text
    # a side above 4096 (the kernel's staging bound holds below 7000): refused on the sizes alone, no table of that size is needed
    from umpr_amd._lib import lib
    one = np.asarray([-1], dtype=np.int32)
    empty = RawPhotos.pack([None], (1, 1, 1), (4097, 1))
    for dh_, dw_ in ((1, 4097), (4097, 1)):
        with pytest.raises(UmprHipError, match="photo_fetch_augment_u8: output size .* has a side above 4096"):
            lib().call("umpr_photo_fetch_augment_u8", None, 0, empty.data, one.ctypes.data, one.ctypes.data,
                       np.asarray([0, 0, 1, 1, 0], dtype=np.int32).ctypes.data, 1, dh_, dw_, None, 0, None, 0, rig.xt, rig.yt, rig.out, 0)
    assert rig.unchanged_since(snap)
    # and the same buffers still serve a good call
    got = rig.call(holed, [-1, 1, -1], [0, -1, -1], rec(0, (3, 2, 20, 11, 1)))
    assert np.array_equal(got, augment_batch([U[0], U[1], U[2]], rec(0, (3, 2, 20, 11, 1)), size)) and rig.guards_intact(1)


# ---- the module and the model -----------------------------------------------------------------------------------------------------
def _plain_u8(raw, dev):
    """uint8 [n][dh][dw][3] of a RawPhotos' plain photos (None where missing), read back from the plain GPU fetch, which the
    existing tests hold to the host form bit for bit."""
    dw, dh = raw.size
    f = RawPhotos(raw.data, raw.geometry, raw.size).to(dev).cpu().numpy().reshape(-1, 3, dh, dw)
    byte = np.searchsorted(LUT, f)
    assert np.array_equal(LUT[byte], f)
    rows = raw.descriptors()["rows"]
    return [np.ascontiguousarray(byte[k].transpose(1, 2, 0)).astype(np.uint8) if rows[k] > 0 else None for k in range(len(f))]


def test_module_with_and_without_a_store(dev, photo_set):
    """PhotoAugment on real decoded photos: no store, then a store cold (misses fill slots with the plain image) and warm (hits, the
    files no longer read), each the reference's photos for that call's draw; the draw does not depend on which of them it is."""
    torch.manual_seed(31)
    p = photo_set[:3] + photo_set[7:10] + ["unknown"]
    samples = samples_for(p, 2, 2, 2, seed=2)                    # 8 photos: the first repeats
    aug = PhotoAugment(flip=True, min_area=0.3)
    raw = batch_loader(samples, resize_on_gpu=True)[6]
    images = _plain_u8(raw, dev)
    got = aug(raw, dev)
    assert aug._calls == 1 and got.shape == raw.shape and got.dtype == torch.float32 and got.is_contiguous()
    assert np.array_equal(got.cpu().numpy().reshape(8, 3, 224, 224), augment_batch(images, aug.draw(1, 8), (224, 224)))
    store = PhotoStore(dev, capacity_bytes=5 * slot_bytes((224, 224))).register(p)      # one slot short: one photo stays a miss
    for call, hits in ((2, 0), (3, 5)):
        raw = batch_loader(samples, resize_on_gpu=True, store=store.index)[6]
        assert int(raw.hits.sum()) == hits + (1 if hits else 0)                        # warm: the repeated photo hits twice
        got = aug(raw, dev, non_blocking=True)
        assert aug._calls == call
        rec = aug.draw(call, 8)
        assert not np.array_equal(rec, aug.draw(call - 1, 8))
        assert np.array_equal(got.cpu().numpy().reshape(8, 3, 224, 224), augment_batch(images, rec, (224, 224)))
    assert store.stats()["used"] == 5 and store.stats()["inserts"] == 5 and store.stats()["decoded_while_full"] >= 1
    plain = batch_loader(samples, resize_on_gpu=True, store=store.index)[6].to(dev)    # the store holds plain images
    assert torch.equal(plain, batch_loader(samples)[6].to(dev))


def _step_state(m, pred, loss):
    torch.cuda.synchronize()
    return (pred.detach().clone(), loss.detach().clone(), {k: v.detach().clone() for k, v in m.state_dict().items()},
            {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None})


def _same(a, b):
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    for part in (2, 3):
        assert a[part].keys() == b[part].keys() and a[part]
        for k in a[part]:
            assert torch.equal(a[part][k], b[part][k]), k


@pytest.fixture(scope="module")
def real_batch(photo_set):
    V, Pc = 1, 1
    samples = samples_for(photo_set[:2], 2, V, Pc, seed=41)
    cfg = dict(review_net_only=False, views=["food"], photo_count=Pc)
    from umpr_amd.synthetic import make_param_state
    return samples, cfg, make_param_state(141, 50, 500, V, False, m_scale=0.05)


def test_training_step_equals_a_twin_fed_the_reference_photos(dev, real_batch):
    """views = 1, B = 2, the real 224 x 224 photos: prediction, loss, every gradient and every updated weight of a step with
    photo_flip / photo_crop are those of a model without the options fed the float photos the reference makes from draw(1, n).
    Cold (misses fill the store) and warm (hits)."""
    from umpr_amd.optim import FusedAdam
    from umpr_amd.train import train_step
    samples, cfg, P = real_batch
    store = PhotoStore(dev, capacity_bytes=4 * slot_bytes((224, 224))).register(p for s in samples for v in s[3] for p in v)
    images = _plain_u8(batch_loader(samples, resize_on_gpu=True)[6], dev)
    for warm in (False, True):
        torch.manual_seed(77)
        on = _model(_cfg(photo_flip=True, photo_crop=0.3, **cfg), P, dev, seed=77)
        batch = batch_loader(samples, resize_on_gpu=True, store=store.index)
        assert bool(batch[6].hits.all()) == warm
        rec = on.photo_augment.draw(1, 2)
        assert not np.array_equal(rec[:, :4], [[0, 0, 224, 224]] * 2)
        a = _step_state(on, *train_step(on, FusedAdam(on, 1e-3, 1e-3), batch))
        assert on.photo_augment._calls == 1
        twin = _model(_cfg(**cfg), P, dev, seed=77)
        assert twin.photo_augment is None
        fed = list(batch_loader(samples))
        fed[6] = torch.from_numpy(augment_batch(images, rec, (224, 224)).reshape(tuple(fed[6].shape))).to(fed[6].dtype)
        b = _step_state(twin, *train_step(twin, FusedAdam(twin, 1e-3, 1e-3), fed))
        _same(a, b)
    assert store.stats()["inserts"] == 2 and store.stats()["hits"] == 2


def test_eval_and_no_grad_fetch_plain_photos_and_float_photos_are_refused(dev, real_batch):
    samples, cfg, P = real_batch
    on = _model(_cfg(photo_flip=True, photo_crop=0.3, **cfg), P, dev)
    off = _model(_cfg(**cfg), P, dev)
    raw = lambda: batch_loader(samples, resize_on_gpu=True)
    with torch.no_grad():
        for m in (on, off):
            m.train()
        # training mode under no_grad (validation inside training()): plain photos; dropout is seeded by the VGG's own counter
        torch.manual_seed(3)
        a = on(*raw())
        torch.manual_seed(3)
        b = off(*raw())
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    on.eval(), off.eval()
    a, b = on(*raw()), off(*raw())
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert on.photo_augment._calls == 0
    on.train()
    with pytest.raises(RuntimeError, match="photo_flip / photo_crop"):
        on(*batch_loader(samples))                                 # float photos in a training forward: loud, never skipped
    assert on.photo_augment._calls == 0
    on.eval()
    assert on(*batch_loader(samples))[0].shape == (2,)             # ... and fine where nothing is augmented


def test_resume_after_the_second_of_three_steps_ends_on_the_same_bits(dev, real_batch, tmp_path):
    from umpr_amd.checkpoint import load_checkpoint, save_checkpoint
    from umpr_amd.optim import FusedAdam
    from umpr_amd.train import train_step
    samples, cfg, P = real_batch
    cfg = _cfg(photo_flip=True, photo_crop=0.3, **cfg)
    path = str(tmp_path / "ck.pt")
    torch.manual_seed(55)
    m = _model(cfg, P, dev, seed=55)
    opt = FusedAdam(m, 1e-3, 1e-3)
    for k in range(3):
        out = train_step(m, opt, batch_loader(samples, resize_on_gpu=True))
        if k == 1:
            save_checkpoint(path, m, opt)
    want = _step_state(m, *out)
    assert m.photo_augment._calls == 3
    torch.manual_seed(55)
    fresh = _model(cfg, P, dev, seed=55)
    opt = FusedAdam(fresh, 1e-3, 1e-3)
    load_checkpoint(path, fresh, opt, map_location=dev)
    assert fresh.photo_augment._calls == 2
    _same(_step_state(fresh, *train_step(fresh, opt, batch_loader(samples, resize_on_gpu=True))), want)
