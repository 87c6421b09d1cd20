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
* ``ReviewDraw`` - a training batch drawn anew every epoch (main.py --review_pool / --word_dropout): a store built with ``keep``
  holds user and item POOLS of up to 1024 sentences; ``collate(indices, draw=)`` shows each sample ``keep`` of them, chosen and
  ordered by counter-based hashes of (seed, epoch, sample, role, position), and replaces tokens by ``<UNK>``, all inside
  ``umpr_review_collate_sampled``.  ``ReviewTable.draw`` is the definition: the host runs it for the batch's samples to get the
  shapes and lengths, the kernel agrees with it bit for bit.  A plain ``collate`` on such a store shows the first ``keep``.
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
from .photos import _mix64

ROLES = ("user", "item", "ui")
MAX_POOL = 1024                           # sentences of one pool the sampled collate ranks (its LDS key table)
DROP_KEY = 0xD6E8FEB86659FD93             # separates the word-dropout stream from the sentence keys of the same role


def role_keys(key, idx, role):
    """uint64 [len(idx)]: mix64(mix64(key + n) + role) for the samples n of `idx`; role 0 / 1 / 2 = user / item / ui."""
    with np.errstate(over="ignore"):
        return _mix64(_mix64(np.uint64(key) + np.asarray(idx).astype(np.uint64)) + np.uint64(role))


class ReviewDraw:
    """The randomness of a sampled collate, counter-based like photos.PhotoAugment's: every number is a hash of (seed, epoch, the
    sample's index in the store, role, position), so a sample's draw does not depend on its batch-mates, its place in the batch,
    the shard, the rank, the loader workers or the collates made before it, and no counter has to travel in a checkpoint.
    `seed` defaults to torch.initial_seed().  `word_dropout` = p in [0, 1): a token inside a sentence becomes `unk` with
    probability p - at output position (s, l) of a role iff
        (mix64(mix64(role_key ^ DROP_KEY) + ((s << 8) | l)) >> 32) < threshold = min(floor(p * 2**32), 2**32 - 1)."""

    def __init__(self, seed=None, epoch=0, word_dropout=0.0, unk=None):
        p = float(word_dropout)
        if not 0.0 <= p < 1.0:
            raise ValueError(f"ReviewDraw: word_dropout must lie in [0, 1), got {word_dropout!r}")
        self.seed = (torch.initial_seed() if seed is None else int(seed)) & 0xFFFFFFFFFFFFFFFF
        self.word_dropout = p
        self.threshold = min(int(np.floor(p * 2.0 ** 32)), 2 ** 32 - 1)
        if self.threshold and unk is None:
            raise ValueError("ReviewDraw: word_dropout > 0 needs the id of <UNK> (unk=)")
        self.unk = None if unk is None else int(unk)
        self.set_epoch(epoch)

    def set_epoch(self, epoch):
        """`key` = mix64(mix64(seed) + epoch), the part of every key the samples share."""
        self.epoch = int(epoch)
        with np.errstate(over="ignore"):
            self.key = int(_mix64(_mix64(np.uint64(self.seed)) + np.uint64(self.epoch & 0xFFFFFFFFFFFFFFFF)))

    def drop_mask(self, idx, role, S, L):
        """bool [len(idx), S, L]: the output positions of `role` (0 / 1 / 2) word dropout hits, were they all inside a sentence."""
        if not self.threshold:
            return np.zeros((len(idx), S, L), dtype=bool)
        at = (np.arange(S, dtype=np.uint64)[:, None] << np.uint64(8)) | np.arange(L, dtype=np.uint64)[None, :]
        with np.errstate(over="ignore"):
            h = _mix64(_mix64(role_keys(self.key, idx, role) ^ np.uint64(DROP_KEY))[:, None, None] + at[None])
        return (h >> np.uint64(32)) < np.uint64(self.threshold)

    def __repr__(self):
        return f"ReviewDraw(seed={self.seed}, epoch={self.epoch}, word_dropout={self.word_dropout}, unk={self.unk})"


class ReviewTable:
    """The host half of a ReviewStore: the de-duplicated arena, the three CSR tables and the per-sample shape arrays, as numpy.
    Touches no device, so the construction and the shape arithmetic are testable without one."""

    def __init__(self, users, items, uis, ratings, keep=None):
        n = len(ratings)
        if not (len(users) == len(items) == len(uis) == n):
            raise ValueError(f"ReviewTable: {len(users)} user, {len(items)} item, {len(uis)} ui pools and {n} ratings")
        # keep = k: the user and item lists are POOLS of which a sample shows k sentences - the first k in a plain collate (all
        # the shape arithmetic below runs on the counts clipped to k), a fresh draw of k in a sampled one (`draw`)
        self.keep = None if keep is None else int(keep)
        if self.keep is not None:
            if self.keep < 1:
                raise ValueError(f"ReviewTable: keep = {keep!r}: a sample must show at least one sentence of its pools")
            for role, pools in zip(ROLES[:2], (users, items)):
                for k, sents in enumerate(pools):
                    if len(sents) > MAX_POOL:
                        raise ValueError(f"ReviewTable: the {role} pool of sample {k} holds {len(sents)} sentences, above the "
                                         f"{MAX_POOL} a draw can rank")
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
        self.pool_count = {role: self.count[role] for role in ROLES[:2]}      # the whole pools; `count` below is what shows
        if self.keep is not None:
            for role in ROLES[:2]:
                self.count[role] = np.minimum(self.count[role], self.keep)
        self.tokens = np.asarray(tokens, dtype=np.int64)
        if self.tokens.size and (self.tokens.min() < 0 or self.tokens.max() > 0x7fffffff):
            raise ValueError("ReviewTable: a token id does not fit the int32 arena")
        self.tokens = self.tokens.astype(np.int32)
        self.sent_off = np.asarray(offs, dtype=np.int64)
        self._sent_len = None                               # per distinct sentence, made by the first draw
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
            cnt = np.diff(self.row_ptr[role])
            rows = np.repeat(np.arange(n), cnt)
            cols = np.arange(len(rows)) - np.repeat(self.row_ptr[role][:-1], cnt)
            ln = lens[role]
            if self.keep is not None and role != "ui":                    # the sentences a plain collate shows
                shown = cols < self.keep
                rows, cols, ln = rows[shown], cols[shown], ln[shown]
            m[rows, cols] = np.maximum(ln, 1)
            self.lengths[role] = m
            # batch_loader takes the raw longest sentence for user and item, pad_reviews' max(1, len) for ui
            longest = np.zeros(n, dtype=np.int64)
            np.maximum.at(longest, rows, ln)
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

    def draw_keep(self):
        """How many sentences of a pool a sampled collate shows: `keep`, or without one the largest user or item count."""
        if self.keep is not None:
            return self.keep
        return max(1, int(max(self.count["user"].max(initial=0), self.count["item"].max(initial=0))))

    def draw(self, idx, draw):
        """THE DEFINITION of a sampled batch's sentence draw (the kernel agrees with it bit for bit): for the samples `idx` and
        the ReviewDraw `draw`, per role user / item (pos [B, keep] int64 - pool positions by slot, -1 beyond the sample's count -
        and len [B, keep] - the raw lengths of those sentences, 0 beyond).  With n a sample's index in the store,
            role_key = mix64(mix64(draw.key + n) + role),   key_j = mix64(role_key + j) for j in 0 .. n_pool - 1,
        and slot s holds the position whose key has rank s (ties to the smaller j), s < min(keep, n_pool).  A function of
        (seed, epoch, n) only: B x 2 x n_pool hashes and one stable row-wise sort."""
        keep, B = self.draw_keep(), len(idx)
        if self._sent_len is None:
            self._sent_len = np.diff(self.sent_off)
        # both roles in one pass: rows 0 .. B-1 the user pools, rows B .. 2B-1 the item pools
        c = np.minimum(np.concatenate([self.pool_count[role][idx] for role in ROLES[:2]]), MAX_POOL)
        j = np.arange(max(int(c.max(initial=0)), 1), dtype=np.uint64)
        with np.errstate(over="ignore"):
            base = _mix64(np.uint64(draw.key) + np.asarray(idx).astype(np.uint64))
            role_key = _mix64(np.concatenate([base, base + np.uint64(1)]))
            keys = _mix64(role_key[:, None] + j[None, :])
        # the columns beyond a pool sort behind every position of it: the largest key, and the sort is stable
        keys[j[None, :] >= c[:, None].astype(np.uint64)] = np.uint64(0xFFFFFFFFFFFFFFFF)
        order = np.argsort(keys, axis=1, kind="stable")[:, :keep]
        k = order.shape[1]
        shown = np.arange(k)[None, :] < c[:, None]
        pos = np.full((2 * B, keep), -1, dtype=np.int64)
        ln = np.zeros((2 * B, keep), dtype=np.int64)
        pos[:, :k] = np.where(shown, order, -1)
        at = np.where(shown, order, 0)
        for r, role in enumerate(ROLES[:2]):
            rows = slice(r * B, (r + 1) * B)
            if self.sent_id[role].size:
                sid = self.sent_id[role][np.minimum(self.row_ptr[role][idx][:, None] + at[rows], self.sent_id[role].size - 1)]
                ln[rows, :k] = np.where(shown[rows], self._sent_len[sid], 0)
        return {role: (pos[r * B:(r + 1) * B], ln[r * B:(r + 1) * B]) for r, role in enumerate(ROLES[:2])}

    def drawn_shape(self, idx, draw):
        """(S, L, S_ui, L_ui) and the three host length tensors of the sampled batch of samples `idx`: what batch_loader computes
        on the drawn lists.  Word dropout changes no length."""
        drawn = self.draw(idx, draw)
        S = int(max(self.count["user"][idx].max(), self.count["item"][idx].max()))   # a draw shows min(keep, n_pool) sentences
        L = int(max(drawn["user"][1].max(initial=0), drawn["item"][1].max(initial=0)))
        S_ui, L_ui = int(self.count["ui"][idx].max()), int(self.longest["ui"][idx].max())
        lengths = tuple(np.maximum(drawn[role][1][:, :S], 1) for role in ROLES[:2])
        return (S, L, S_ui, L_ui), lengths + (self.lengths["ui"][idx, :S_ui],)


class ReviewStore(ReviewTable):
    """A dataset's tokenised reviews in device memory, allocated once: `tokens` int32 [T], `sent_off` int64 [n_sent + 1], per role
    `row_ptr` int64 [n_samples + 1] and `sent_id` int32 [nnz], `ratings` float32 [n_samples].  `collate(indices)` is
    data.batch_loader(samples, ignore_photos=True) for the samples of those indices, written on the device.  With
    `device="cpu"` the arrays are built (for inspection and tests) but collate has no CPU path."""

    def __init__(self, dataset, device):
        users, items, uis, _, ratings = dataset.data
        pools, keep = getattr(dataset, "pools", None), None
        if pools is not None:                           # Dataset(review_pool=N): the tables hold the whole pools
            (users, items), keep = pools, dataset.max_s_count
        self._build(users, items, uis, ratings, device, keep)

    @classmethod
    def from_lists(cls, users, items, uis, ratings, device, keep=None):
        """From raw lists: each of users / items / uis holds, per sample, a list of token lists.  With `keep` = k the user and
        item lists are pools of up to 1024 sentences, of which a batch shows k per sample."""
        self = cls.__new__(cls)
        self._build(users, items, uis, ratings, device, keep)
        return self

    def _build(self, users, items, uis, ratings, device, keep=None):
        ReviewTable.__init__(self, users, items, uis, ratings, keep)
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
        self.batches = self.sampled = 0

    def collate(self, indices, pad=0, shard=None, photos=None, draw=None):
        """batch_loader's eight-tuple (nine with `shard=(rank, world)`: the number of non-empty chunks comes last) for the samples
        `indices`, repeats allowed.  Ids and labels are device tensors, user and item ids the halves of one [2,B,S,L] allocation;
        the lengths are CPU LongTensors.  (S, L, S_ui, L_ui) are taken over the whole (global) batch, only this rank's contiguous
        chunk is produced; an empty chunk gives zero-row tensors without a launch.  `photos` fills the photo element (a
        photos.RawPhotos of this chunk, a tensor), the empty tensor of batch_loader(ignore_photos=True) by default.
        Allocates from torch's caching allocator and launches on the current stream: no upload, no synchronisation.
        On a store with `keep` a sample shows the first `keep` sentences of its pools: the un-pooled store's batch, bit for bit.
        `draw=` a ReviewDraw: the sampled collate (umpr_review_collate_sampled) - batch_loader's tuple for the samples whose user
        and item lists were replaced by their draw (ReviewTable.draw) and whose tokens were then dropped (ReviewDraw.drop_mask);
        the host forms the same draw for the batch's samples to get the shapes and the lengths."""
        if self.device.type != "cuda":
            raise RuntimeError("ReviewStore collates on an MI355X only (no CPU path): use data.batch_loader")
        idx = self.checked(indices)
        if draw is None:
            S, L, S_ui, L_ui = self.shape(idx)
        else:
            (S, L, S_ui, L_ui), drawn_lengths = self.drawn_shape(idx, draw)
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
            tables = (self.d_tokens, self.d_sent_off, self.n_sent, p["user"], s["user"], p["item"], s["item"], p["ui"], s["ui"],
                      self.d_ratings, self.n_samples, host_idx.ctypes.data, B, S, L, S_ui, L_ui, int(pad))
            outputs = (ids_pair, ids_ui, labels, torch.cuda.current_stream(self.device).cuda_stream)
            if draw is None:
                lib().call("umpr_review_collate", *tables, *outputs)
            else:
                lib().call("umpr_review_collate_sampled", *tables, self.draw_keep(), draw.key, draw.threshold,
                           -1 if draw.unk is None else draw.unk, *outputs)
                self.sampled += 1
            self.batches += 1
        lengths = self.host_lengths(mine, S, S_ui) if draw is None else \
            tuple(torch.from_numpy(np.ascontiguousarray(m[lo:hi])) for m in drawn_lengths)
        out = (ids_pair[0], ids_pair[1], ids_ui, *lengths, torch.Tensor([]) if photos is None else photos, labels)
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

    def __init__(self, loader, store, rank=0, world=1, draw=None):
        self.loader, self.store = loader, store
        self.shard = (rank, world) if world > 1 else None
        self.draw = draw            # a ReviewDraw: every batch is a sampled collate of the draw's epoch (training only)

    def set_epoch(self, epoch):
        """train.training calls this at the head of every epoch: the draws of epoch e are those of (seed, e, sample)."""
        if self.draw is not None:
            self.draw.set_epoch(epoch)

    def __iter__(self):
        for idx, photos in self.loader:
            yield self.store.collate(idx, shard=self.shard, photos=photos, draw=self.draw)

    def __len__(self):
        return len(self.loader)
