"""Tokenised reviews kept in device memory: a batch's padded id tensors are written by one kernel from B sample indices.

The text half of ``data.batch_loader`` pads three ragged Python lists of token lists into ``[B,S,L]`` LongTensors on the host and
uploads them - 5 to 10 ms per batch, more than a whole step of the fast regimes (UMPR-R, the frozen models with a warm store).
But a sentence is tokenised once, in ``Dataset.__init__``, and the same sentence sits in the pool of every sample of its user and
of its item.  So:

* ``ReviewStore`` - every DISTINCT sentence of a dataset once in an int32 token arena on the device (de-duplicated by content,
  first seen first), per role (user, item, ui) a CSR table sample -> sentence ids, and the ratings.  On the host it keeps, per
  role, each sample's sentence count, longest sentence and row of sentence lengths: all the per-batch host work needs.
  ``collate(indices)`` returns ``batch_loader``'s tuple with the same shapes, dtypes and values; the ids and the labels are
  device tensors written by ``umpr_review_collate`` (csrc/reviews.hip), user and item ids the two halves of ONE [2,B,S,L]
  allocation, which ``UMPR._forward`` takes as its ids_pair without a copy; the lengths are host LongTensors, as the model's host
  sort wants them.  The indices travel in the kernel's arguments: no upload, no pinned staging, no synchronisation.
* ``IndexView`` / ``PhotoCollate`` / ``StoreLoader`` - the loader side (main.py --review_store True): the DataLoader runs over
  (index, photo paths) items with the batch size, shuffle, generator and workers it would have, its workers do the photo half
  only, and the training process turns the indices into the batch.

The store holds a dataset whole or is not used (no partial residency), and lives in the process that built it.  Like the photo
stores it is built and tested for data-parallel sharding (``collate(shard=...)`` against ``batch_loader(shard=...)``) but not run
on more than one rank.
"""
from __future__ import annotations

import numpy as np
import torch

from ._lib import lib

ROLES = ("user", "item", "ui")


class ReviewTable:
    """The host half of a ReviewStore: the de-duplicated arena, the three CSR tables and the per-sample shape arrays, as numpy.
    Touches no device, so the construction and the shape arithmetic are testable without one."""

    def __init__(self, users, items, uis, ratings):
        n = len(ratings)
        if not (len(users) == len(items) == len(uis) == n):
            raise ValueError(f"ReviewTable: {len(users)} user, {len(items)} item, {len(uis)} ui pools and {n} ratings")
        seen, tokens, offs = {}, [], [0]
        self.row_ptr, self.sent_id, self.count, self.longest = {}, {}, {}, {}
        lens = {}
        for role, pools in zip(ROLES, (users, items, uis)):
            ptr, sid, ln = np.zeros(n + 1, dtype=np.int64), [], []
            for k, sents in enumerate(pools):
                for s in sents:
                    key = tuple(s)
                    j = seen.get(key)
                    if j is None:
                        j = seen[key] = len(seen)
                        tokens.extend(key)
                        offs.append(len(tokens))
                    sid.append(j)
                    ln.append(len(key))
                ptr[k + 1] = len(sid)
            self.row_ptr[role], self.sent_id[role] = ptr, np.asarray(sid, dtype=np.int32)
            self.count[role] = np.diff(ptr)
            lens[role] = np.asarray(ln, dtype=np.int64)
        self.tokens = np.asarray(tokens, dtype=np.int64)
        if self.tokens.size and (self.tokens.min() < 0 or self.tokens.max() > 0x7fffffff):
            raise ValueError("ReviewTable: a token id does not fit the int32 arena")
        self.tokens = self.tokens.astype(np.int32)
        self.sent_off = np.asarray(offs, dtype=np.int64)
        self.ratings = torch.Tensor(list(ratings))          # as batch_loader builds its labels: the same bits
        self.n_samples, self.n_sent = n, len(seen)
        self.per_sample_tokens = int(sum(l.sum() for l in lens.values()))   # what one copy per sample would hold
        # lengths[role][k] = pad_reviews' lengths row of sample k: max(1, len) per sentence, 1 for the sentences padding adds.
        # User and item share their padded count in a batch, so their matrices share a width.
        cap = {"ui": int(self.count["ui"].max(initial=0))}
        cap["user"] = cap["item"] = int(max(self.count["user"].max(initial=0), self.count["item"].max(initial=0)))
        self.lengths = {}
        for role in ROLES:
            m = np.ones((n, max(cap[role], 1)), dtype=np.int64)
            cnt = self.count[role]
            rows = np.repeat(np.arange(n), cnt)
            cols = np.arange(len(rows)) - np.repeat(self.row_ptr[role][:-1], cnt)
            m[rows, cols] = np.maximum(lens[role], 1)
            self.lengths[role] = m
            # batch_loader takes the raw longest sentence for user and item, pad_reviews' max(1, len) for ui
            longest = np.zeros(n, dtype=np.int64)
            np.maximum.at(longest, rows, lens[role])
            self.longest[role] = np.maximum(longest, 1) if role == "ui" else longest

    def shape(self, idx):
        """(S, L, S_ui, L_ui) of the batch of samples `idx`: the maxima batch_loader computes, user and item sharing S and L."""
        S = int(max(self.count["user"][idx].max(), self.count["item"][idx].max()))
        L = int(max(self.longest["user"][idx].max(), self.longest["item"][idx].max()))
        return S, L, int(self.count["ui"][idx].max()), int(self.longest["ui"][idx].max())

    def checked(self, indices):
        """`indices` as an int64 array, refused unless every one names a sample."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if idx.size == 0:
            raise ValueError("ReviewStore.collate: an empty batch")
        if idx.min() < 0 or idx.max() >= self.n_samples:
            bad = idx[(idx < 0) | (idx >= self.n_samples)][0]
            raise IndexError(f"ReviewStore.collate: sample index {int(bad)} outside the {self.n_samples} samples of the store")
        return idx

    def host_lengths(self, idx, S, S_ui):
        """The three CPU LongTensors of lengths for samples `idx`, [len(idx), S] twice and [len(idx), S_ui]."""
        return tuple(torch.from_numpy(self.lengths[role][idx, :w]) for role, w in zip(ROLES, (S, S, S_ui)))


class ReviewStore(ReviewTable):
    """A dataset's tokenised reviews in device memory, allocated once: `tokens` int32 [T], `sent_off` int64 [n_sent + 1], per role
    `row_ptr` int64 [n_samples + 1] and `sent_id` int32 [nnz], `ratings` float32 [n_samples].  `collate(indices)` is
    data.batch_loader(samples, ignore_photos=True) for the samples of those indices, written on the device.  With
    `device="cpu"` the arrays are built (for inspection and tests) but collate has no CPU path."""

    def __init__(self, dataset, device):
        users, items, uis, _, ratings = dataset.data
        self._build(users, items, uis, ratings, device)

    @classmethod
    def from_lists(cls, users, items, uis, ratings, device):
        """From raw lists: each of users / items / uis holds, per sample, a list of token lists."""
        self = cls.__new__(cls)
        self._build(users, items, uis, ratings, device)
        return self

    def _build(self, users, items, uis, ratings, device):
        ReviewTable.__init__(self, users, items, uis, ratings)
        device = torch.device(device)
        if device.type == "cuda" and device.index is None:
            device = torch.device("cuda", torch.cuda.current_device())
        self.device = device
        dev = lambda a: torch.from_numpy(a).to(device)
        self.d_tokens, self.d_sent_off = dev(self.tokens), dev(self.sent_off)
        self.d_row_ptr = {r: dev(self.row_ptr[r]) for r in ROLES}
        self.d_sent_id = {r: dev(self.sent_id[r]) for r in ROLES}
        self.d_ratings = self.ratings.to(device)
        self.nbytes = sum(t.numel() * t.element_size() for t in
                          (self.d_tokens, self.d_sent_off, self.d_ratings, *self.d_row_ptr.values(), *self.d_sent_id.values()))
        self.batches = 0

    def collate(self, indices, pad=0, shard=None, photos=None):
        """batch_loader's eight-tuple (nine with `shard=(rank, world)`: the number of non-empty chunks comes last) for the samples
        `indices`, repeats allowed.  Ids and labels are device tensors, user and item ids the halves of one [2,B,S,L] allocation;
        the lengths are CPU LongTensors.  (S, L, S_ui, L_ui) are taken over the whole (global) batch, only this rank's contiguous
        chunk is produced; an empty chunk gives zero-row tensors without a launch.  `photos` fills the photo element (a
        photos.RawPhotos of this chunk, a tensor), the empty tensor of batch_loader(ignore_photos=True) by default.
        Allocates from torch's caching allocator and launches on the current stream: no upload, no synchronisation."""
        if self.device.type != "cuda":
            raise RuntimeError("ReviewStore collates on an MI355X only (no CPU path): use data.batch_loader")
        idx = self.checked(indices)
        S, L, S_ui, L_ui = self.shape(idx)
        lo, hi = 0, len(idx)
        if shard is not None:
            from .parallel import active_shards, shard_bounds
            lo, hi = shard_bounds(len(idx), *shard)
        mine = idx[lo:hi]
        B = len(mine)
        ids_pair = torch.empty((2, B, S, L), dtype=torch.int64, device=self.device)
        ids_ui = torch.empty((B, S_ui, L_ui), dtype=torch.int64, device=self.device)
        labels = torch.empty(B, dtype=torch.float32, device=self.device)
        if B:
            host_idx = np.ascontiguousarray(mine, dtype=np.int32)       # read during the call: it rides in the kernel arguments
            p, s = self.d_row_ptr, self.d_sent_id
            lib().call("umpr_review_collate", self.d_tokens, self.d_sent_off, self.n_sent, p["user"], s["user"], p["item"], s["item"],
                       p["ui"], s["ui"], self.d_ratings, self.n_samples, host_idx.ctypes.data, B, S, L, S_ui, L_ui, int(pad),
                       ids_pair, ids_ui, labels, torch.cuda.current_stream(self.device).cuda_stream)
            self.batches += 1
        out = (ids_pair[0], ids_pair[1], ids_ui, *self.host_lengths(mine, S, S_ui),
               torch.Tensor([]) if photos is None else photos, labels)
        if shard is not None:
            out = out + (torch.tensor(active_shards(len(idx), shard[1])),)
        return out

    def stats(self):
        return dict(samples=self.n_samples, sentences=self.n_sent, tokens=int(self.tokens.size),
                    per_sample_tokens=self.per_sample_tokens, bytes=self.nbytes, batches=self.batches)

    def __repr__(self):
        return (f"ReviewStore({self.n_samples} samples, {self.n_sent} distinct sentences, {self.tokens.size} tokens "
                f"({self.per_sample_tokens} stored per sample), {self.nbytes} B on {self.device})")


class IndexView(torch.utils.data.Dataset):
    """A Dataset seen as (index, photo paths): what a DataLoader runs over when the reviews come from a ReviewStore.  Same length,
    so the same sampler draws the same indices in the same order."""

    def __init__(self, dataset):
        self.photos = dataset.data[3]

    def __len__(self):
        return len(self.photos)

    def __getitem__(self, i):
        return i, self.photos[i]


class PhotoCollate:
    """Picklable worker-side collate over IndexView items: (indices as an int64 array, the photo half of batch_loader - a
    photos.RawPhotos of this rank's chunk, store ids included - or None with `ignore_photos`)."""

    def __init__(self, ignore_photos, rank=0, world=1, store=None):
        self.ignore_photos = ignore_photos
        self.shard = (rank, world) if world > 1 else None
        self.store = store

    def __call__(self, items):
        idx = np.fromiter((i for i, _ in items), dtype=np.int64, count=len(items))
        if self.ignore_photos:
            return idx, None
        from .data import raw_photos
        from .parallel import shard_bounds
        lo, hi = shard_bounds(len(items), *self.shard) if self.shard is not None else (0, len(items))
        first = items[0][1]
        return idx, raw_photos([p for _, p in items[lo:hi]], (len(first), len(first[0])), store=self.store)


class StoreLoader:
    """Wraps the index DataLoader in the training process: every (indices, photos) batch becomes store.collate(...)'s tuple.
    `.loader` is the DataLoader (train._shuffle_generator finds its generator through it)."""

    def __init__(self, loader, store, rank=0, world=1):
        self.loader, self.store = loader, store
        self.shard = (rank, world) if world > 1 else None

    def __iter__(self):
        for idx, photos in self.loader:
            yield self.store.collate(idx, shard=self.shard, photos=photos)

    def __len__(self):
        return len(self.loader)
