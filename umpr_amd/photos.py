"""Item photos resized on the GPU (umpr_photo_resize_u8, csrc/photos.hip).

The host form of the loader (data.get_image) decodes, resizes and divides by 255 on the host and uploads a float32
[B, V, P, 3, dh, dw] tensor.  Here the host only decodes: ``decode_for_gpu`` keeps the source rows and columns the resize
taps read (at most 2*dh x 2*dw x 3 bytes, never more than the 3*dh*dw*4 bytes of the float photo) and the tap tables
data.resize_bilinear_u8 would use; ``RawPhotos`` packs a batch of them into one uint8 buffer (descriptors, tables, pixels), so
a batch is one H2D copy, and ``RawPhotos.to(device)`` runs the integer resize on the device.  The result is bit-identical to
the host form.

``PhotoStore`` (off unless asked for) keeps the resized uint8 image of every photo it has seen in device memory: a photo is
decoded once per run, every later use ships no pixels and is a table lookup on the device (umpr_photo_fetch_u8), still
bit-identical.  No eviction: once the slots are used up, further photos are decoded every time.

``PhotoAugment`` (off unless asked for) draws a random crop window and a flip per photo of a training batch and fetches the photos
augmented (umpr_photo_fetch_augment_u8): the window of the resized uint8 image - a store slot, or a scratch slot - resized back
with the same integer resize, bit-identical to doing so on the host.  A store slot always holds the plain image.

``FeatureStore`` (off unless asked for, frozen VGG only) keeps what the VGG makes of a photo instead: 1000 floats, 4 000 B against
the photo's 150 528 B.  A resident photo is then neither decoded nor resized nor run through the VGG: ``features`` resizes only the
photos the store lacks, runs the VGG once on those, and one kernel (umpr_feature_fetch_f32) builds the dense feature tensor the
head takes and fills the new slots.

``Pool5Store`` (off unless asked for, frozen conv base only: UMPR(freeze_conv=True)) keeps the conv stage's pool5 row instead:
25088 floats, 100 352 B, still less than the uint8 photo.  The classifier trains on the stored rows: ``features`` returns the
compact classifier arena with the rows fetched into its head, and an Adam step on the classifier leaves the store as it is.
"""
from __future__ import annotations

import logging
import uuid
import weakref

import numpy as np
import torch

from .data import _column_taps, _row_taps

# one per photo, at the head of the packed buffer; layout of umpr_photo_desc (include/umpr_hip.h)
DESC = np.dtype([("pixels", "<i8"), ("taps", "<i8"), ("rows", "<i4"), ("cols", "<i4")])
assert DESC.itemsize == 24


def decode_for_gpu(path, size=(224, 224)):
    """(pixels uint8 [rows][cols][3], taps int32 [4*dw + 4*dh]) of one photo, or None for a missing one (unreadable file,
    'unknown' path: get_image's except branch).  `size` = (dw, dh) as for get_image.  The taps index the compacted pixels."""
    dw, dh = size
    try:
        from PIL import Image
        with Image.open(path) as im:
            rgb = np.asarray(im.convert('RGB'), dtype=np.uint8)
        h, w, _ = rgb.shape
        x0, x1, a0, a1 = _column_taps(dw, w)
        y0, y1, b0, b1 = _row_taps(dh, h)
    except Exception:
        return None
    rows = np.unique(np.concatenate([y0, y1]))
    cols = np.unique(np.concatenate([x0, x1]))
    if len(rows) < h:
        rgb = np.take(rgb, rows, axis=0)
    if len(cols) < w:
        rgb = np.take(rgb, cols, axis=1)
    taps = np.concatenate([np.searchsorted(cols, x0), np.searchsorted(cols, x1), a0, a1,
                           np.searchsorted(rows, y0), np.searchsorted(rows, y1), b0, b1]).astype(np.int32)
    return np.ascontiguousarray(rgb), taps


class RawPhotos:
    """A batch of decoded photos in one packed uint8 buffer: [n descriptors][tap tables][pixels], n = B*V*P.

    Stands in for the float32 photo tensor of a collated batch: ``.shape`` is the logical (B, V, P, 3, dh, dw),
    ``.pin_memory()`` (DataLoader(pin_memory=True)) and pickling (DataLoader workers) keep the buffer, and
    ``.to(device)`` uploads it on the current stream and returns the float32 photos resized there."""

    def __init__(self, data, geometry, size, ids=None, hits=None, store_key=None):
        self.data = data                          # torch.uint8, 1-D, host
        self.geometry = tuple(int(g) for g in geometry)
        self.size = (int(size[0]), int(size[1]))  # (dw, dh)
        # collated against a PhotoStore's index (batch_loader(store=...)): per photo its id in the store (-1: none) and whether
        # the worker left it undecoded because the store held it; the key finds the store in this process
        self.ids = ids                            # torch.int32 [n] or None
        self.hits = hits                          # torch.uint8 [n] or None
        self.store_key = store_key

    @classmethod
    def pack(cls, decoded, geometry, size):
        """Packs decode_for_gpu results (photo order: sample, view, photo) for a batch of `geometry` = (B, V, P).  None stands
        for a missing photo, and for one a PhotoStore holds: both get a 0 x 0 descriptor."""
        n = int(np.prod(geometry))
        assert len(decoded) == n, (len(decoded), geometry)
        dw, dh = size
        tap_bytes = 16 * (dw + dh)
        desc = np.zeros(n, dtype=DESC)
        head = -(-desc.nbytes // 16) * 16          # tables and pixels start 16-byte aligned
        off = head
        present = [i for i, d in enumerate(decoded) if d is not None]
        for i in present:
            desc["taps"][i] = off
            off += tap_bytes
        for i in present:
            pix = decoded[i][0]
            desc["pixels"][i] = off
            desc["rows"][i], desc["cols"][i] = pix.shape[:2]
            off += pix.nbytes
        buf = np.empty(off, dtype=np.uint8)
        buf[:desc.nbytes] = desc.view(np.uint8)
        buf[desc.nbytes:head] = 0
        for i in present:
            pix, taps = decoded[i]
            t, p = int(desc["taps"][i]), int(desc["pixels"][i])
            buf[t:t + tap_bytes] = taps.view(np.uint8)
            buf[p:p + pix.nbytes] = pix.reshape(-1)
        return cls(torch.from_numpy(buf), geometry, size)

    @property
    def shape(self):
        dw, dh = self.size
        return torch.Size(self.geometry + (3, dh, dw))

    def descriptors(self):
        """The n umpr_photo_desc records as a numpy structured array (a view of the buffer)."""
        n = int(np.prod(self.geometry))
        return self.data.numpy()[:n * DESC.itemsize].view(DESC)

    def pin_memory(self, device=None):
        return RawPhotos(self.data.pin_memory(), self.geometry, self.size, self.ids, self.hits, self.store_key)

    def is_pinned(self):
        return self.data.is_pinned()

    def to(self, device, non_blocking=False):
        """Uploads the buffer (one copy) and resizes on `device`'s current stream: float32 [B, V, P, 3, dh, dw]."""
        from ._lib import UmprHipError, lib
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("RawPhotos resize on an MI355X only (no CPU path): use batch_loader(resize_on_gpu=False)")
        dw, dh = self.size
        n = int(np.prod(self.geometry))
        if self.store_key is not None and n:
            store = PhotoStore.find(self.store_key)
            if store is not None:
                return store.fetch(self, device, non_blocking)
            if bool(self.hits.any()):
                raise UmprHipError(f"RawPhotos: {int(self.hits.sum())} photos were left to photo store {self.store_key}, which "
                                   f"is not registered in this process")
        out = torch.empty(self.shape, dtype=torch.float32, device=device)
        if n == 0:
            return out
        if self.data.dtype != torch.uint8 or self.data.dim() != 1 or self.data.numel() < n * DESC.itemsize:
            raise UmprHipError(f"RawPhotos: buffer of {self.data.numel()} bytes cannot hold the {n} photo descriptors")
        with torch.cuda.device(device):
            packed = self.data.to(device, non_blocking=non_blocking)
            # the descriptors are read (and checked against the buffer size) on the host, from the head of the host buffer
            lib().call("umpr_photo_resize_u8", packed, packed.numel(), self.data, n, dh, dw, out,
                       torch.cuda.current_stream(device).cuda_stream)
        return out

    def __repr__(self):
        kept = "" if self.hits is None else f", {int(self.hits.sum())} left to the store"
        return f"RawPhotos(shape={tuple(self.shape)}, bytes={self.data.numel()}{kept})"


class PhotoIndex:
    """What the loader workers know of a PhotoStore: path -> dense id, and one byte per id in shared memory that the store
    sets once the photo is resident.  Picklable; the bytes stay shared across fork and torch.multiprocessing pickling."""

    def __init__(self, key, size, max_photos):
        self.key = key
        self.size = (int(size[0]), int(size[1]))
        self.ids = {}
        self.resident = torch.zeros(int(max_photos), dtype=torch.uint8).share_memory_()

    def lookup(self, paths):
        """(ids int32 [n], hits uint8 [n]) of `paths`; a hit is a photo the worker need not open."""
        ids = np.fromiter((self.ids.get(p, -1) for p in paths), dtype=np.int32, count=len(paths))
        hits = np.zeros(len(paths), dtype=np.uint8)
        known = ids >= 0
        hits[known] = self.resident.numpy()[ids[known]]
        return ids, hits


class PhotoTable:
    """The host half of a PhotoStore: ids, the id -> slot table, which photo of a batch reads or fills which slot, and the
    counters.  Touches no device, so the planning is testable without one."""

    def __init__(self, size=(224, 224), slots=0, max_photos=1 << 22):
        self.key = uuid.uuid4().hex
        self.index = PhotoIndex(self.key, size, max_photos)
        self.slots = int(slots)
        self.max_photos = int(max_photos)
        self._slot = np.full(self.max_photos, -1, dtype=np.int32)      # id -> slot; with index.ids the path -> slot table
        self.used = self.hits = self.inserts = self.decoded_while_full = self.unregistered = 0
        self._logged_overflow = False

    @property
    def size(self):
        return self.index.size

    def register(self, paths):
        """Ids for the new paths among `paths` (any iterable; 'unknown' and paths past max_photos get none).  Call it before
        the DataLoader that serves these paths is built: its workers copy the table when they start."""
        ids = self.index.ids
        for p in paths:
            if p == 'unknown' or p in ids:
                continue
            if len(ids) >= self.max_photos:
                self.unregistered += 1
                continue
            ids[p] = len(ids)
        if self.unregistered and not self._logged_overflow:
            self._logged_overflow = True
            logging.getLogger(__name__).warning("photo store: more than max_photos = %d distinct photos; the rest are decoded "
                                                "every time", self.max_photos)
        return self

    def id_of(self, path):
        return self.index.ids.get(path, -1)

    def slot_of(self, path):
        """Slot that holds `path`'s resized image, or -1."""
        i = self.id_of(path)
        return int(self._slot[i]) if i >= 0 else -1

    def plan(self, raw):
        """(src_slot, dst_slot) int32 [n] for a RawPhotos collated against this table's index: hits read their slot; the first
        decoded occurrence of an id that is not resident yet gets a free slot while there is one; everything else - later
        occurrences, photos decoded by a worker whose view lagged, photos beyond the capacity - is only resized."""
        from ._lib import UmprHipError
        if raw.size != self.size:
            raise UmprHipError(f"photo store holds {self.size} photos, the batch is {raw.size}")
        n = int(np.prod(raw.geometry))
        ids, hits = raw.ids.numpy(), raw.hits.numpy()
        if len(ids) != n or len(hits) != n:
            raise UmprHipError(f"RawPhotos: {len(ids)} ids and {len(hits)} hit flags for {n} photos")
        src = np.full(n, -1, dtype=np.int32)
        dst = np.full(n, -1, dtype=np.int32)
        hit = np.flatnonzero(hits)
        if len(hit):
            if ids[hit].min() < 0 or ids[hit].max() >= self.max_photos or self._slot[ids[hit]].min() < 0:
                raise UmprHipError("photo store: a photo was left to the store, which does not hold it")
            src[hit] = self._slot[ids[hit]]
        free, full = self.used, 0
        taken = set()
        for i in np.flatnonzero((hits == 0) & (ids >= 0) & (ids < self.max_photos) & (raw.descriptors()["rows"] > 0)):
            k = int(ids[i])
            if self._slot[k] >= 0 or k in taken:
                continue
            if free >= self.slots:
                full += 1
                continue
            dst[i] = free
            free += 1
            taken.add(k)
        return src, dst, full

    def commit(self, raw, src, dst, full=0):
        """Books a fetch that has been enqueued: the filled slots become resident, for the workers too.  Returns the number of
        slots filled."""
        ids = raw.ids.numpy()
        new = np.flatnonzero(dst >= 0)
        self.decoded_while_full += full
        self._slot[ids[new]] = dst[new]
        self.used += len(new)
        self.inserts += len(new)
        self.hits += int((src >= 0).sum())
        self.index.resident.numpy()[ids[new]] = 1
        return len(new)

    def stats(self):
        return dict(slots=self.slots, used=self.used, hits=self.hits, inserts=self.inserts,
                    decoded_while_full=self.decoded_while_full, unregistered=self.unregistered)


class PhotoStore(PhotoTable):
    """Resized photos kept in device memory: `capacity_bytes // slot_bytes` slots of 3*dh*dw uint8 (rounded up to 16), allocated
    once.  `register(paths)` gives paths ids, `index` goes to batch_loader(store=...), and RawPhotos.to(device) finds the store
    again by its key: the first decoded use of a photo also fills a slot, later uses read it.  No eviction: when the slots run
    out, further photos are decoded every time."""

    _registry = weakref.WeakValueDictionary()

    def __init__(self, device, size=(224, 224), capacity_bytes=1 << 30, max_photos=1 << 22):
        from ._lib import UmprHipError, lib
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("PhotoStore lives on an MI355X (no CPU path)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)
        dw, dh = size
        self.slot_bytes = lib().size("umpr_photo_store_slot_bytes", int(dh), int(dw))
        if self.slot_bytes == 0:
            raise UmprHipError(f"PhotoStore: bad photo size {size}")
        super().__init__(size, int(capacity_bytes) // self.slot_bytes, max_photos)
        self.buffer = torch.empty(max(self.slots, 1) * self.slot_bytes, dtype=torch.uint8, device=self.device)
        self._insert_stream = self._insert_event = None
        PhotoStore._registry[self.key] = self

    @classmethod
    def find(cls, key):
        return cls._registry.get(key)

    def fetch(self, raw, device, non_blocking=False):
        """RawPhotos.to(device) with this store, on the current stream: float32 [B, V, P, 3, dh, dw]."""
        from ._lib import UmprHipError, lib
        device = torch.device(device)
        if device.index is not None and device != self.device:
            raise UmprHipError(f"PhotoStore on {self.device} asked for photos on {device}")
        dw, dh = raw.size
        n = int(np.prod(raw.geometry))
        if raw.data.dtype != torch.uint8 or raw.data.dim() != 1 or raw.data.numel() < n * DESC.itemsize:
            raise UmprHipError(f"RawPhotos: buffer of {raw.data.numel()} bytes cannot hold the {n} photo descriptors")
        src, dst, full = self.plan(raw)
        with torch.cuda.device(self.device):
            out = torch.empty(raw.shape, dtype=torch.float32, device=self.device)
            stream = torch.cuda.current_stream(self.device)
            if self._insert_event is not None and stream != self._insert_stream:
                stream.wait_event(self._insert_event)     # slots filled on another stream
            packed = raw.data.to(self.device, non_blocking=non_blocking)
            lib().call("umpr_photo_fetch_u8", packed, packed.numel(), raw.data, src.ctypes.data, dst.ctypes.data, len(src), dh,
                       dw, self.buffer, self.slots, out, stream.cuda_stream)
            if self.commit(raw, src, dst, full):               # the workers stop decoding these only now that the fill is enqueued
                self._insert_event = torch.cuda.Event()
                self._insert_event.record(stream)
                self._insert_stream = stream
        return out

    def stats(self):
        return dict(super().stats(), bytes=self.slots * self.slot_bytes)

    def __repr__(self):
        return (f"PhotoStore({self.size[0]}x{self.size[1]}, {self.used}/{self.slots} slots of {self.slot_bytes} B on "
                f"{self.device}, {len(self.index.ids)} photos registered)")


def tap_tables(size):
    """(xt int32 [dw][4*dw], yt int32 [dh][4*dh]) for umpr_photo_fetch_augment_u8: row s-1 holds the concatenated
    data._column_taps(dw, s) / data._row_taps(dh, s), the taps resize_bilinear_u8 uses for a source of extent s."""
    dw, dh = size
    xt = np.stack([np.concatenate(_column_taps(dw, s)) for s in range(1, dw + 1)]).astype(np.int32)
    yt = np.stack([np.concatenate(_row_taps(dh, s)) for s in range(1, dh + 1)]).astype(np.int32)
    return xt, yt


def _mix64(x):
    """splitmix64's output function on a uint64 array (wrapping arithmetic)."""
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        x = (x ^ (x >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        x = (x ^ (x >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return x ^ (x >> np.uint64(31))


class PhotoAugment(torch.nn.Module):
    """Random resized crop and horizontal flip of a batch's photos at the fetch (umpr_photo_fetch_augment_u8): the photo's resized
    uint8 image - its PhotoStore slot, or a scratch slot - is cropped to a window, resized back with the integer resize the loader
    uses and mirrored, on the device.  `draw` is torchvision's RandomResizedCrop on the dh x dw image, scale (min_area, 1), ratio
    (3/4, 4/3); `min_area` = 1 keeps the whole image, `flip` adds a fair coin.  Counter-based randomness: every number is a hash of
    (seed, call, photo index in the batch, draw number), seed = torch.initial_seed() and the data-parallel rank, so no global
    generator is touched and the draws do not depend on the store, the hits or the loader workers.  `_calls` counts the augmented
    fetches and travels in a checkpoint's rng_calls.  No parameters, no buffers: the scratch slots and the tap tables are plain
    attributes, made on first use and kept."""

    TRIES = 10
    RATIO = (3.0 / 4.0, 4.0 / 3.0)

    def __init__(self, flip=False, min_area=1.0, size=(224, 224)):
        super().__init__()
        if not 0.0 < float(min_area) <= 1.0:
            raise ValueError(f"PhotoAugment: min_area must lie in (0, 1], got {min_area!r}")
        self.flip, self.min_area = bool(flip), float(min_area)
        self.size = (int(size[0]), int(size[1]))       # (dw, dh)
        self._calls = 0
        self._tables = self._scratch = None

    def extra_repr(self):
        return f"flip={self.flip}, min_area={self.min_area}, size={self.size}"

    @staticmethod
    def seed():
        from . import parallel
        rank = torch.distributed.get_rank() if parallel.active() else 0
        return (torch.initial_seed() * 1000003 + rank) & 0xFFFFFFFFFFFFFFFF

    def _uniform(self, key, k):
        """Draw number k of every photo: float64 in [0, 1) from the top 53 bits of the hash."""
        return (_mix64(key + np.uint64(k)) >> np.uint64(11)).astype(np.float64) * 2.0 ** -53

    def draw(self, call, n):
        """int32 [n][5] = (x0, y0, cw, ch, flip) of augmented fetch number `call` for photos 0 .. n-1."""
        dw, dh = self.size
        index = np.arange(n, dtype=np.uint64)
        key = _mix64(_mix64(_mix64(np.full(n, self.seed(), dtype=np.uint64)) + np.uint64(int(call) & 0xFFFFFFFFFFFFFFFF)) + index)
        out = np.zeros((n, 5), dtype=np.int32)
        out[:, 2], out[:, 3] = dw, dh
        if self.min_area < 1.0:
            # the fall-back after TRIES failures: the largest centred window whose ratio lies in RATIO
            if dw / dh < self.RATIO[0]:
                cw, ch = dw, min(dh, int(np.rint(dw / self.RATIO[0])))
            elif dw / dh > self.RATIO[1]:
                cw, ch = min(dw, int(np.rint(dh * self.RATIO[1]))), dh
            else:
                cw, ch = dw, dh
            cw, ch = np.full(n, cw, dtype=np.int64), np.full(n, ch, dtype=np.int64)
            x0, y0 = (dw - cw) // 2, (dh - ch) // 2
            found = np.zeros(n, dtype=bool)
            lo, hi = np.log(self.RATIO[0]), np.log(self.RATIO[1])
            for t in range(self.TRIES):
                area = dh * dw * (self.min_area + (1.0 - self.min_area) * self._uniform(key, 2 * t))
                ratio = np.exp(lo + (hi - lo) * self._uniform(key, 2 * t + 1))
                w = np.rint(np.sqrt(area * ratio)).astype(np.int64)
                h = np.rint(np.sqrt(area / ratio)).astype(np.int64)
                take = ~found & (w >= 1) & (w <= dw) & (h >= 1) & (h <= dh)
                cw, ch = np.where(take, w, cw), np.where(take, h, ch)
                found |= take
            # the offset: uniform over the positions at which the window fits
            px = np.minimum((self._uniform(key, 2 * self.TRIES) * (dw - cw + 1)).astype(np.int64), dw - cw)
            py = np.minimum((self._uniform(key, 2 * self.TRIES + 1) * (dh - ch + 1)).astype(np.int64), dh - ch)
            out[:, 0], out[:, 1] = np.where(found, px, x0), np.where(found, py, y0)
            out[:, 2], out[:, 3] = cw, ch
        if self.flip:
            out[:, 4] = _mix64(key + np.uint64(2 * self.TRIES + 2)) >> np.uint64(63)
        return out

    def _device_state(self, device, need, slot_bytes):
        """The tap tables on `device` and `need` scratch slots (grown to the largest count seen, at most a batch's photos)."""
        if self._tables is None or self._tables[0].device != device:
            self._tables = tuple(torch.from_numpy(t).to(device) for t in tap_tables(self.size))
            self._scratch = None
        if need and (self._scratch is None or self._scratch.numel() < need * slot_bytes):
            self._scratch = torch.empty(need * slot_bytes, dtype=torch.uint8, device=device)
        return self._tables[0], self._tables[1], self._scratch

    def forward(self, raw, device, non_blocking=False):
        """RawPhotos.to(device) with a fresh draw per photo, on the current stream: float32 [B, V, P, 3, dh, dw].  With a
        PhotoStore the plan, the fills and the bookkeeping are PhotoStore.fetch's: a slot receives the plain image."""
        from ._lib import UmprHipError, lib
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("PhotoAugment runs on an MI355X only (no CPU path)")
        if raw.size != self.size:
            raise UmprHipError(f"PhotoAugment was built for {self.size} photos, the batch is {raw.size}")
        dw, dh = raw.size
        n = int(np.prod(raw.geometry))
        if raw.data.dtype != torch.uint8 or raw.data.dim() != 1 or raw.data.numel() < n * DESC.itemsize:
            raise UmprHipError(f"RawPhotos: buffer of {raw.data.numel()} bytes cannot hold the {n} photo descriptors")
        store = PhotoStore.find(raw.store_key) if raw.store_key is not None else None
        if store is None and raw.store_key is not None and bool(raw.hits.any()):
            raise UmprHipError(f"RawPhotos: {int(raw.hits.sum())} photos were left to photo store {raw.store_key}, which is not "
                               f"registered in this process")
        if store is not None:
            if device.index is not None and device != store.device:
                raise UmprHipError(f"PhotoStore on {store.device} asked for photos on {device}")
            device = store.device
            src, dst, full = store.plan(raw)
        else:
            device = torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)
            src = dst = np.full(n, -1, dtype=np.int32)
        self._calls += 1
        crop = np.ascontiguousarray(self.draw(self._calls, n))
        with torch.cuda.device(device):
            out = torch.empty(raw.shape, dtype=torch.float32, device=device)
            if n == 0:
                return out
            slot_bytes = lib().size("umpr_photo_store_slot_bytes", dh, dw)
            need = int(((src < 0) & (dst < 0) & (raw.descriptors()["rows"] > 0)).sum())
            xt, yt, scratch = self._device_state(device, need, slot_bytes)
            stream = torch.cuda.current_stream(device)
            if store is not None and store._insert_event is not None and stream != store._insert_stream:
                stream.wait_event(store._insert_event)     # slots filled on another stream
            packed = raw.data.to(device, non_blocking=non_blocking)
            lib().call("umpr_photo_fetch_augment_u8", packed, packed.numel(), raw.data, src.ctypes.data, dst.ctypes.data,
                       crop.ctypes.data, n, dh, dw, store.buffer if store is not None else None, store.slots if store is not None else 0,
                       scratch, need, xt, yt, out, stream.cuda_stream)
            if store is not None and store.commit(raw, src, dst, full):   # as PhotoStore.fetch: resident once the fill is enqueued
                store._insert_event = torch.cuda.Event()
                store._insert_event.record(stream)
                store._insert_stream = stream
        return out


def vgg_fingerprint(vgg):
    """What a FeatureStore remembers of the VGG parameters its rows were computed from: storage address, version counter, dtype
    and device of every parameter, and the module's compute dtype.  ``load_state_dict`` / ``load_checkpoint`` (in-place copies:
    the version counters advance), ``.to()`` and a dtype change (new storage) all change it."""
    return (str(getattr(vgg, "compute_dtype", "")),) + tuple(
        (p.data_ptr(), p._version, str(p.dtype), str(p.device)) for p in vgg.parameters())


def conv_fingerprint(vgg):
    """vgg_fingerprint over the conv stage (``features.*``) only - what a Pool5Store's rows were computed from.  A step on the
    classifier leaves it as it is; any write to a conv parameter changes it."""
    return (str(getattr(vgg, "compute_dtype", "")),) + tuple(
        (p.data_ptr(), p._version, str(p.dtype), str(p.device)) for p in vgg.features.parameters())


class FeatureTable(PhotoTable):
    """The host half of a FeatureStore: PhotoTable's ids, id -> slot table and resident bytes, and the plan of which photo of a
    batch reads a slot, which is computed, and which computed row fills a slot.  Slot `slots` (one past the last) is the reserved
    row of the all-zero image.  Touches no device."""

    def __init__(self, size=(224, 224), slots=0, max_photos=1 << 22):
        super().__init__(size, slots, max_photos)
        self.zero_slot = self.slots
        self.zero_ready = False
        self.fingerprint = None
        self.computed = self.shared = self.missing = self.flushes = self.vgg_calls = 0

    def guard(self, fingerprint):
        """Empties the table when `fingerprint` is not the one its rows were filled under; returns whether it did."""
        if fingerprint == self.fingerprint:
            return False
        stale = self.fingerprint is not None and (self.used > 0 or self.zero_ready)
        self.fingerprint = fingerprint
        if stale:
            self.invalidate()
        return stale

    def invalidate(self):
        """Nothing is resident any more, for the workers too.  A batch collated before this still names its hits: plan() refuses it."""
        self.index.resident.zero_()
        self._slot[:] = -1
        self.used = 0
        self.zero_ready = False
        self.flushes += 1

    def plan(self, raw):
        """(src_slot, dst_slot, fresh_row int32 [n], miss, full) for a RawPhotos collated against this table's index.  Hits read
        their slot, and so does a photo that became resident after its worker looked.  A 0 x 0 descriptor without a hit is a
        missing photo and reads the zero-image row.  Every other photo is computed: `miss` lists the photos to run through the
        VGG, in batch order, and fresh_row[i] is the position in `miss` of the photo whose row photo i takes - its own, or that of
        the first photo of the call with the same id.  The first computed occurrence of an id gets a free slot while there is
        one; `full` counts those that found none.  Photos without an id are computed every time."""
        from ._lib import UmprHipError
        if raw.size != self.size:
            raise UmprHipError(f"feature store holds {self.size} photos, the batch is {raw.size}")
        n = int(np.prod(raw.geometry))
        if raw.ids is None or raw.hits is None:
            raise UmprHipError("RawPhotos: not collated against a store's index (no ids)")
        ids, hits = raw.ids.numpy(), raw.hits.numpy()
        if len(ids) != n or len(hits) != n:
            raise UmprHipError(f"RawPhotos: {len(ids)} ids and {len(hits)} hit flags for {n} photos")
        src = np.full(n, -1, dtype=np.int32)
        dst = np.full(n, -1, dtype=np.int32)
        row = np.full(n, -1, dtype=np.int32)
        hit = np.flatnonzero(hits)
        if len(hit):
            if ids[hit].min() < 0 or ids[hit].max() >= self.max_photos or self._slot[ids[hit]].min() < 0:
                raise UmprHipError("feature store: a photo was left to the store, which does not hold it")
            src[hit] = self._slot[ids[hit]]
        rows = raw.descriptors()["rows"]
        free, full, miss, first = self.used, 0, [], {}
        for i in np.flatnonzero(hits == 0):
            k = int(ids[i]) if 0 <= ids[i] < self.max_photos else -1
            if rows[i] <= 0:
                src[i] = self.zero_slot
            elif k >= 0 and self._slot[k] >= 0:
                src[i] = self._slot[k]
            elif k >= 0 and k in first:
                row[i] = first[k]
            else:
                row[i] = len(miss)
                miss.append(int(i))
                if k >= 0:
                    first[k] = row[i]
                    if free < self.slots:
                        dst[i] = free
                        free += 1
                    else:
                        full += 1
        return src, dst, row, np.asarray(miss, dtype=np.int64), full

    def commit(self, raw, src, dst, row, full=0):
        """Books a `features` call that has been enqueued: the filled slots become resident, for the workers too.  Returns the
        number of slots filled."""
        ids = raw.ids.numpy()
        new = np.flatnonzero(dst >= 0)
        zero = int((src == self.zero_slot).sum())
        n_miss = int(row.max()) + 1 if len(row) and row.max() >= 0 else 0
        self.decoded_while_full += full
        self._slot[ids[new]] = dst[new]
        self.used += len(new)
        self.inserts += len(new)
        self.hits += int((src >= 0).sum()) - zero
        self.missing += zero
        self.computed += n_miss
        self.shared += int((row >= 0).sum()) - n_miss
        self.index.resident.numpy()[ids[new]] = 1
        return len(new)

    def stats(self):
        return dict(super().stats(), computed=self.computed, shared=self.shared, missing=self.missing, flushes=self.flushes,
                    vgg_calls=self.vgg_calls)


class FeatureStore(FeatureTable):
    """VGG features of photos kept in device memory: `capacity_bytes // 4000` slots of 1000 fp32 plus the reserved row of the
    all-zero image, allocated once, private to this process and gone with it.  For a FROZEN VGG only (UMPR(freeze_vgg=True)): its
    output for a photo is then a constant of the run.  `register(paths)` and `index` are PhotoStore's; UMPR.forward hands a
    RawPhotos collated against the index to `features(raw, vgg)`.  The store remembers which parameters filled it
    (vgg_fingerprint) and empties itself when they change.  No eviction: when the slots run out, further photos are computed
    every time."""

    F = 1000
    _registry = weakref.WeakValueDictionary()

    def __init__(self, device, size=(224, 224), capacity_bytes=1 << 30, max_photos=1 << 22):
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError(f"{type(self).__name__} lives on an MI355X (no CPU path)")
        self.device = torch.device("cuda", torch.cuda.current_device() if device.index is None else device.index)
        self.slot_bytes = 4 * self.F
        super().__init__(size, int(capacity_bytes) // self.slot_bytes, max_photos)
        self.buffer = torch.empty((self.slots + 1) * self.F, dtype=torch.float32, device=self.device)
        self._insert_stream = self._insert_event = None
        type(self)._registry[self.key] = self      # each store class has a key space of its own

    @classmethod
    def find(cls, key):
        return cls._registry.get(key)

    def _vgg(self, vgg, images):
        self.vgg_calls += 1
        with torch.no_grad():
            out = vgg(images)
        if out.requires_grad or out.dtype != torch.float32 or tuple(out.shape) != (images.shape[0], self.F):
            raise RuntimeError(f"FeatureStore: the VGG returned {tuple(out.shape)} {out.dtype}, not fp32 [n, {self.F}] without grad")
        return out if out.is_contiguous() else out.contiguous()

    def _refuse_trainable(self, vgg):
        from ._lib import UmprHipError
        if any(p.requires_grad for p in vgg.parameters()):
            raise UmprHipError("FeatureStore: the VGG has trainable parameters, so its output for a photo is no constant of the "
                               "run: build the model with freeze_vgg=True")

    _fingerprint = staticmethod(vgg_fingerprint)
    _emptied = "feature store: the VGG parameters changed; emptied"

    def _out(self, n):
        """What `features` returns; the fetch writes the n rows at its base."""
        return torch.empty(n, self.F, dtype=torch.float32, device=self.device)

    def features(self, raw, vgg, non_blocking=False):
        """float32 [B*V*P, 1000] on the current stream: what `vgg(raw.to(device).flatten(0, 2))` returns for a frozen `vgg`, with
        the VGG run only on the photos the store lacks."""
        from ._lib import UmprHipError, lib
        self._refuse_trainable(vgg)
        dw, dh = raw.size
        n = int(np.prod(raw.geometry))
        if raw.data.dtype != torch.uint8 or raw.data.dim() != 1 or raw.data.numel() < n * DESC.itemsize:
            raise UmprHipError(f"RawPhotos: buffer of {raw.data.numel()} bytes cannot hold the {n} photo descriptors")
        if self.guard(self._fingerprint(vgg)):
            logging.getLogger(__name__).info(self._emptied)
        src, dst, row, miss, full = self.plan(raw)
        call = lambda *a: lib().call("umpr_feature_fetch_f32", *a)
        with torch.cuda.device(self.device):
            stream = torch.cuda.current_stream(self.device)
            if self._insert_event is not None and stream != self._insert_stream:
                stream.wait_event(self._insert_event)     # slots filled on another stream
            filled = False
            if not self.zero_ready and bool((src == self.zero_slot).any()):
                # the missing photo: the VGG on ONE all-zero image, once per store (and again after it was emptied)
                fresh = self._vgg(vgg, torch.zeros(1, 3, dh, dw, dtype=torch.float32, device=self.device))
                one = lambda v: np.asarray([v], dtype=np.int32)
                r0, s0, d0 = one(0), one(-1), one(self.zero_slot)
                call(fresh, 1, r0.ctypes.data, s0.ctypes.data, d0.ctypes.data, 1, self.F, self.buffer, self.slots + 1,
                     torch.empty(self.F, dtype=torch.float32, device=self.device), stream.cuda_stream)
                self.zero_ready = filled = True
            fresh = None
            if len(miss):
                packed = raw.data.to(self.device, non_blocking=non_blocking)
                desc = np.ascontiguousarray(raw.descriptors()[miss])      # the misses' records; offsets into the same buffer
                images = torch.empty(len(miss), 3, dh, dw, dtype=torch.float32, device=self.device)
                lib().call("umpr_photo_resize_u8", packed, packed.numel(), desc.ctypes.data, len(miss), dh, dw, images,
                           stream.cuda_stream)
                fresh = self._vgg(vgg, images)
            out = self._out(n)
            call(fresh, len(miss), row.ctypes.data, src.ctypes.data, dst.ctypes.data, n, self.F, self.buffer, self.slots + 1, out,
                 stream.cuda_stream)
            if self.commit(raw, src, dst, row, full) or filled:      # the workers skip these only now that the fill is enqueued
                self._insert_event = torch.cuda.Event()
                self._insert_event.record(stream)
                self._insert_stream = stream
        return out

    def stats(self):
        return dict(super().stats(), bytes=(self.slots + 1) * self.slot_bytes)

    def __repr__(self):
        return (f"FeatureStore({self.used}/{self.slots} slots of {self.slot_bytes} B on {self.device}, "
                f"{len(self.index.ids)} photos registered)")


class Pool5Store(FeatureStore):
    """pool5 rows of photos kept in device memory: `capacity_bytes // 100352` slots of 25088 fp32 plus the reserved row of the
    all-zero image.  For a FROZEN CONV BASE only (UMPR(freeze_conv=True)): the conv stage's output for a photo is then a constant
    of the run while the classifier trains on it.  Plan, zero row, ids and `find` are FeatureStore's, in a key space of its own.
    The store remembers the conv parameters that filled it (conv_fingerprint): an optimiser step on the classifier leaves it as it
    is, a write to any conv parameter empties it.  Rows stay fp32 in both precisions; no eviction; gone with the process."""

    F = 25088
    _registry = weakref.WeakValueDictionary()

    def _vgg(self, vgg, images):
        self.vgg_calls += 1
        out = vgg.conv_base(images)
        if out.requires_grad or out.dtype != torch.float32 or tuple(out.shape) != (images.shape[0], self.F):
            raise RuntimeError(f"Pool5Store: the conv base returned {tuple(out.shape)} {out.dtype}, not fp32 [n, {self.F}] without grad")
        return out if out.is_contiguous() else out.contiguous()

    def _refuse_trainable(self, vgg):
        from ._lib import UmprHipError
        if any(p.requires_grad for p in vgg.features.parameters()):
            raise UmprHipError("Pool5Store: the conv base has trainable parameters, so its pool5 for a photo is no constant of the "
                               "run: build the model with freeze_conv=True")

    _fingerprint = staticmethod(conv_fingerprint)
    _emptied = "pool5 store: the conv parameters changed; emptied"

    def _out(self, n):
        from ._lib import lib
        return torch.empty(lib().size("umpr_vgg16_cls_arena_bytes", n) // 4, dtype=torch.float32, device=self.device)

    def features(self, raw, vgg, non_blocking=False):
        """The compact classifier arena of the batch (umpr_vgg16_cls_arena_bytes(B*V*P) as flat fp32) on the current stream, its
        first B*V*P x 25088 floats filled with the photos' pool5 rows by the one fetch: ready for `vgg.classify(arena, B*V*P)`.
        The conv base runs only on the photos the store lacks."""
        return super().features(raw, vgg, non_blocking)

    def __repr__(self):
        return (f"Pool5Store({self.used}/{self.slots} slots of {self.slot_bytes} B on {self.device}, "
                f"{len(self.index.ids)} photos registered)")
