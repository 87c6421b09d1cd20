"""The host definition of a sampled review batch (umpr_amd/reviews.py::ReviewDraw, csrc/reviews.hip::umpr_review_collate_sampled),
restated in plain Python integers, one sample at a time: the draw is applied to Python lists of token lists, the tokens are
dropped, and data.batch_loader collates the result.  Shares no code with reviews.py but the constants written out here, so the
vectorised numpy definition there and the kernel are both checked against it."""
M64 = (1 << 64) - 1
DROP_KEY = 0xD6E8FEB86659FD93
ROLE = {"user": 0, "item": 1, "ui": 2}


def mix64(x):
    """splitmix64's output function"""
    x = (x + 0x9E3779B97F4A7C15) & M64
    x = ((x ^ (x >> 30)) * 0xBF58476D1CE4E5B9) & M64
    x = ((x ^ (x >> 27)) * 0x94D049BB133111EB) & M64
    return x ^ (x >> 31)


def role_key(seed, epoch, n, role):
    base = mix64((mix64((mix64(seed & M64) + epoch) & M64) + n) & M64)
    return mix64((base + ROLE[role]) & M64)


def threshold(p):
    return min(int(p * 2 ** 32), 2 ** 32 - 1)          # floor: p >= 0


def positions(seed, epoch, n, role, n_pool, keep):
    """pool positions by slot: the min(keep, n_pool) smallest keys, ties to the smaller position"""
    rk = role_key(seed, epoch, n, role)
    return sorted(range(n_pool), key=lambda j: (mix64((rk + j) & M64), j))[:keep]


def dropped(seed, epoch, n, role, sents, p, unk):
    """`sents` (the role's sentences by slot) with word dropout at rate p"""
    T = threshold(p)
    if T == 0:
        return [list(s) for s in sents]
    dk = mix64(role_key(seed, epoch, n, role) ^ DROP_KEY)
    return [[unk if (mix64((dk + ((s << 8) | l)) & M64) >> 32) < T else tok for l, tok in enumerate(sent)]
            for s, sent in enumerate(sents)]


def sampled_sample(sample, n, seed, epoch, keep, p=0.0, unk=None):
    """(user sentences, item sentences, ui sentences, photos, rating) of sample n of the store after its draw: `sample` holds the
    user and item POOLS."""
    out = []
    for role, sents in zip(("user", "item"), sample[:2]):
        out.append(dropped(seed, epoch, n, role, [sents[j] for j in positions(seed, epoch, n, role, len(sents), keep)], p, unk))
    out.append(dropped(seed, epoch, n, "ui", sample[2], p, unk))          # never sampled
    return tuple(out) + tuple(sample[3:])


def sampled_batch(samples, idx, seed, epoch, keep, p=0.0, unk=None, pad=0, shard=None):
    """data.batch_loader(..., ignore_photos=True) on the drawn samples `idx` of `samples` (pools).  batch_loader takes the maximum
    over an empty sequence for a sample without user or item sentences and raises; such a pool stands in as ONE empty sentence,
    which pad_reviews pads to the rows it gives the empty list (all `pad`, lengths 1) whenever the batch has a row at all."""
    from umpr_amd.data import batch_loader
    drawn = []
    for k in idx:
        u, i, ui, ph, r = sampled_sample(samples[int(k)], int(k), seed, epoch, keep, p, unk)
        drawn.append((u or [[]], i or [[]], ui, ph, r))
    return batch_loader(drawn, ignore_photos=True, pad=pad, shard=shard)
