"""Float64 NumPy reference of the embedding-table gradient (test helper, not a test module; CPU only).

A trainable table (nn.Embedding.from_pretrained(..., freeze=False)) receives
    dx [T][E]       = dgx[:, 0:3H] W_ih_f + dgx[:, 3H:6H] W_ih_r          (dgx: gradient of the GRU's input projections)
    d_emb [vocab][E]: row v = the sum of dx over the positions whose id is v, rows no token names zero
over every use of the table.  The functions here state both in NumPy - in float64 for the reference, in float32 for the yardstick
of the gate (coattn_decisions.gate: a HIP tensor may be K = 4 x as far from float64 as the float32 CPU evaluation is, floor 2^-22;
the float32 scatter adds position by position in ascending order, np.add.at) - and build the id patterns and the `sorted_pos`
argument of umpr_embed_grad for the GPU tests.  tests/test_embed_grad_reference.py checks them against torch autograd.
"""
import numpy as np
import torch

from coattn_decisions import K_START, gate   # noqa: F401  (shared, not copied)

K = K_START
PATTERNS = ("equal", "distinct", "zipf", "ends")


def dx_reference(dgx, w_ih_f, w_ih_r, dtype=np.float64):
    """dgx [T][6H] (forward direction's 3H gate columns first), w_ih_* [3H][E] -> dx [T][E] in `dtype`"""
    dgx, wf, wr = (np.asarray(a, dtype=dtype) for a in (dgx, w_ih_f, w_ih_r))
    g3 = wf.shape[0]
    assert dgx.shape[1] == 2 * g3 and wr.shape == wf.shape, (dgx.shape, wf.shape, wr.shape)
    return dgx[:, :g3] @ wf + dgx[:, g3:] @ wr


def scatter_reference(sources, vocab, E, dtype=np.float64):
    """sources: [(ids [T_k] integers, dx [T_k][E])] -> d_emb [vocab][E] in `dtype`: positions are added one by one in source
    order, ascending position (np.add.at is unbuffered and sequential); ids outside [0, vocab) are dropped."""
    out = np.zeros((vocab, E), dtype=dtype)
    for ids, dx in sources:
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        dx = np.asarray(dx, dtype=dtype).reshape(ids.size, E)
        ok = (ids >= 0) & (ids < vocab)
        np.add.at(out, ids[ok], dx[ok])
    return out


def sorted_positions(ids_list):
    """int32 [T]: positions of the concatenated sources, stable-sorted by id (the `sorted_pos` argument of umpr_embed_grad)"""
    flat = np.concatenate([np.asarray(i, dtype=np.int64).reshape(-1) for i in ids_list]) if ids_list else np.zeros(0, np.int64)
    return np.argsort(flat, kind="stable").astype(np.int32)


def make_ids(pattern, T, vocab, rng):
    """int64 [T].  equal: one id (7 % vocab) at every position - one run of T.  distinct: T different ids (T <= vocab), shuffled.
    zipf: rank r with probability ~ 1 / (r + 1): long runs of the first ids, singletons in the tail.  ends: uniform, with id 0 at
    the first and vocab - 1 at the last position (and both again in the middle when T >= 4)."""
    assert pattern in PATTERNS, pattern
    if pattern == "equal":
        return np.full(T, 7 % vocab, dtype=np.int64)
    if pattern == "distinct":
        assert T <= vocab, (T, vocab)
        return rng.permutation(vocab)[:T].astype(np.int64)
    if pattern == "zipf":
        p = 1.0 / np.arange(1, vocab + 1)
        return rng.choice(vocab, size=T, p=p / p.sum()).astype(np.int64)
    ids = rng.integers(0, vocab, size=T, dtype=np.int64)
    if T >= 1:
        ids[0] = 0
        ids[-1] = vocab - 1 if T >= 2 else 0
    if T >= 4:
        ids[T // 2] = 0
        ids[T // 2 + 1] = vocab - 1
    return ids


def split_sources(ids, dx, counts):
    """cut ids [T] / dx [T][E] into consecutive sources of the given lengths (sum = T)"""
    assert sum(counts) == len(ids), (counts, len(ids))
    out, lo = [], 0
    for n in counts:
        out.append((ids[lo:lo + n], dx[lo:lo + n]))
        lo += n
    return out


def touched_rows(sources, vocab):
    m = np.zeros(vocab, dtype=bool)
    for ids, _ in sources:
        ids = np.asarray(ids, dtype=np.int64).reshape(-1)
        m[ids[(ids >= 0) & (ids < vocab)]] = True
    return m


def as_tensor(a):
    return torch.from_numpy(np.ascontiguousarray(a))
