"""The sampled review collate on the GPU (reviews.ReviewStore.collate(draw=), csrc/reviews.hip::umpr_review_collate_sampled)
against the host definition of tests/review_sample_reference.py - the draw applied to Python lists, then data.batch_loader -
torch.equal on all eight outputs, the ids and labels written between sentinel-filled guard bands into sentinel-filled buffers;
then the model, training() with a resume inside an epoch, and validation fed from a pooled store."""
import os

import numpy as np
import pytest
import torch

import review_sample_reference as ref
from conftest import GOLDEN
from test_gpu_review_store import GUARD, SENTINEL, _cfg, _one_step

pytestmark = pytest.mark.gpu

CORPUS = os.path.join(GOLDEN, "tiny_corpus")
SEED = 0x5eed5eed5eed5eed5eed       # above 2^64: the draw takes its low 64 bits
KEEP = 4                            # max_sent_count on the tiny corpus


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


class Pools:
    """samples holding user and item POOLS + the store built from the same lists with `keep`"""

    def __init__(self, users, items, uis, ratings, keep, dev):
        from umpr_amd.reviews import ReviewStore
        self.samples = [(u, i, ui, None, r) for u, i, ui, r in zip(users, items, uis, ratings)]
        self.keep = keep
        self.store = ReviewStore.from_lists(users, items, uis, ratings, dev, keep=keep)


def _sentences(rng, n, lo=1, hi=12):
    return [[int(t) for t in rng.integers(3, 400003, size=int(k))] for k in rng.integers(lo, hi + 1, size=n)]


def _pools(sizes_u, sizes_i, keep, dev, seed, lo=1, hi=12):
    rng = np.random.default_rng(seed)
    users = [_sentences(rng, k, lo, hi) for k in sizes_u]
    items = [_sentences(rng, k, lo, hi) for k in sizes_i]
    uis = [_sentences(rng, 1 + n % 4, lo, hi) for n in range(len(users))]
    return Pools(users, items, uis, [float(1 + n % 5) for n in range(len(users))], keep, dev)


def check(c, idx, epoch=0, p=0.0, unk=1, pad=0, shard=None, seed=SEED):
    """both ways to the kernel against the host definition: the C entry point writing between guard bands into sentinel-filled
    buffers, and ReviewStore.collate(draw=)"""
    from umpr_amd._lib import lib
    from umpr_amd.parallel import shard_bounds
    from umpr_amd.reviews import ReviewDraw
    st = c.store
    idx = np.asarray(idx, dtype=np.int64)
    want = ref.sampled_batch(c.samples, idx, seed & ref.M64, epoch, c.keep, p, unk, pad, shard)
    draw = ReviewDraw(seed, epoch, p, unk)
    lo, hi = shard_bounds(len(idx), *shard) if shard else (0, len(idx))
    B = hi - lo
    S, L, S_ui, L_ui = want[0].shape[1], want[0].shape[2], want[2].shape[1], want[2].shape[2]
    assert S <= c.keep
    if B:
        n_pair, n_ui = 2 * B * S * L, B * S_ui * L_ui
        buf = torch.full((GUARD + n_pair + GUARD + n_ui + GUARD,), SENTINEL, dtype=torch.int64, device=st.device)
        lab = torch.full((GUARD + B + GUARD,), float("nan"), dtype=torch.float32, device=st.device)
        host_idx = np.ascontiguousarray(idx[lo:hi], dtype=np.int32)
        t, s = st.d_row_ptr, st.d_sent_id
        lib().call("umpr_review_collate_sampled", st.d_tokens, st.d_sent_off, st.n_sent, t["user"], s["user"], t["item"], s["item"],
                   t["ui"], s["ui"], st.d_ratings, st.n_samples, host_idx.ctypes.data, B, S, L, S_ui, L_ui, pad, c.keep, draw.key,
                   draw.threshold, unk, buf.data_ptr() + 8 * GUARD, buf.data_ptr() + 8 * (2 * GUARD + n_pair),
                   lab.data_ptr() + 4 * GUARD, torch.cuda.current_stream().cuda_stream)
        got, labels = buf.cpu(), lab.cpu()
        for a, b in ((0, GUARD), (GUARD + n_pair, 2 * GUARD + n_pair), (2 * GUARD + n_pair + n_ui, len(got))):
            assert bool((got[a:b] == SENTINEL).all()), "a guard band was written"
        assert bool(labels[:GUARD].isnan().all()) and bool(labels[GUARD + B:].isnan().all())
        pair = got[GUARD:GUARD + n_pair].view(2, B, S, L)
        assert torch.equal(pair[0], want[0]) and torch.equal(pair[1], want[1])
        assert torch.equal(got[2 * GUARD + n_pair:2 * GUARD + n_pair + n_ui].view(B, S_ui, L_ui), want[2])
        assert torch.equal(labels[GUARD:GUARD + B], want[7])
    served = st.stats()["batches"]
    out = st.collate(idx, pad=pad, shard=shard, draw=draw)
    assert st.stats()["batches"] == served + (1 if B else 0)
    assert len(out) == len(want) == (9 if shard else 8)
    for k in (0, 1, 2, 7):
        assert out[k].device == st.device and out[k].dtype == want[k].dtype and out[k].is_contiguous()
    for k in (3, 4, 5, 6):
        assert out[k].device.type == "cpu" and out[k].dtype == want[k].dtype
    for k, (g, w) in enumerate(zip(out, want)):
        assert g.shape == w.shape and torch.equal(g.cpu(), w), k
    assert out[1].untyped_storage().data_ptr() == out[0].untyped_storage().data_ptr()
    if B:
        assert out[1].data_ptr() == out[0].data_ptr() + B * S * L * 8
    return out


# ---- pool sizes x keep ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", (1, 5, 20, 64))
def test_pool_sizes_around_keep_the_wave_the_block_and_the_cap(dev, keep):
    sizes = sorted({0, 1, keep - 1, keep, keep + 1, 63, 64, 65, 255, 256, 257, 1024})
    c = _pools(sizes, sizes[::-1], keep, dev, seed=keep)
    n = len(sizes)
    assert int(c.store.pool_count["user"].max()) == 1024 and int(c.store.count["user"].max()) == keep
    out = check(c, np.arange(n))
    assert out[0].shape[1] == keep
    check(c, np.arange(n), epoch=1, p=0.25, pad=7)
    check(c, [0, n - 1])                                            # no sentence at all on one side, the cap on the other
    for k in range(n):
        check(c, [k], epoch=2)                                      # alone: S and L are the sample's own
    again = check(c, np.arange(n), epoch=1)
    assert not torch.equal(again[0][-1], out[0][-1])                # another epoch: other sentences of the pool of 1024


def test_sentence_lengths_around_the_wave_and_the_longest(dev):
    """pools whose sentences have 0, 1, 63, 64, 65 and 256 tokens: L follows the draw, a sentence without tokens is a row of pad
    with length 1"""
    rng = np.random.default_rng(5)
    lens = (0, 1, 63, 64, 65, 256)
    sent = lambda k: [int(t) for t in rng.integers(3, 400003, size=k)]
    pool = lambda m: [sent(lens[int(j)]) for j in rng.integers(0, 6, size=m)]
    users = [pool(30) for _ in range(6)] + [[sent(k)] for k in lens[1:]] + [[sent(0), sent(1)]]
    items = [pool(7) for _ in range(6)] + [[sent(k)] for k in lens[:0:-1]] + [[sent(64), sent(0)]]
    uis = [[sent(lens[(n + k) % 6 or 1]) for k in range(1 + n % 3)] for n in range(len(users))]
    from umpr_amd.reviews import ReviewStore
    c = Pools.__new__(Pools)
    c.samples = [(u, i, ui, None, 2.5) for u, i, ui in zip(users, items, uis)]
    c.keep, c.store = 5, ReviewStore.from_lists(users, items, uis, [2.5] * len(users), dev, keep=5)
    seen = set()
    for epoch in range(4):
        out = check(c, np.arange(6), epoch=epoch, p=0.5 if epoch % 2 else 0.0, pad=400003)
        seen.add(out[0].shape[2])
    assert 256 in seen
    for k in range(6, 12):
        check(c, [k])                                               # one sentence of 1 .. 256 tokens on each side
    check(c, [11, 6], p=0.9)                                        # rows without tokens next to a short one
    check(c, np.arange(12), epoch=9, p=0.1)


@pytest.fixture(scope="module")
def mixed(dev):
    """40 samples, pools of 1 .. 60 short sentences, keep 20"""
    rng = np.random.default_rng(21)
    return _pools(rng.integers(1, 61, size=40), rng.integers(1, 61, size=40), 20, dev, seed=22)


@pytest.mark.parametrize("B", (1, 64, 257))
def test_batch_sizes_across_the_chunk_seam(dev, mixed, B):
    idx = np.random.default_rng(B).integers(0, 40, size=B)          # with repeats
    out = check(mixed, idx, epoch=B, p=0.2)
    assert out[0].shape[0] == B


def test_a_repeated_index_gives_equal_rows(dev, mixed):
    from umpr_amd.reviews import ReviewDraw
    out = mixed.store.collate([6, 13, 6, 6], draw=ReviewDraw(SEED, 3, 0.3, 1))
    for k in (0, 1, 2, 3, 4, 5, 7):
        assert torch.equal(out[k][0], out[k][2]) and torch.equal(out[k][0], out[k][3])
    alone = mixed.store.collate([13, 6], draw=ReviewDraw(SEED, 3, 0.3, 1))      # other batch-mates, another place: the same draw
    S, L = min(out[0].shape[1], alone[0].shape[1]), min(out[0].shape[2], alone[0].shape[2])
    assert torch.equal(out[0][0, :S, :L], alone[0][1, :S, :L]) and torch.equal(out[1][1, :S, :L], alone[1][0, :S, :L])


def test_shards_against_the_hosts(dev, mixed):
    rng = np.random.default_rng(8)
    for shard in ((0, 2), (1, 2), (2, 3)):
        check(mixed, rng.integers(0, 40, size=7), epoch=1, p=0.2, shard=shard)
    for rank in range(4):                                            # 5 samples over 4 ranks: chunks of 2, 2, 1 and none
        out = check(mixed, [3, 1, 8, 8, 22], epoch=2, shard=(rank, 4))
        assert out[0].shape[0] == (2, 2, 1, 0)[rank] and int(out[8]) == 3


# ---- word dropout -------------------------------------------------------------------------------------------------------------------
def test_word_dropout(dev, mixed):
    from umpr_amd.reviews import ReviewDraw
    st, idx = mixed.store, np.arange(40)
    base = check(mixed, idx, epoch=4)                                # p = 0
    for same in (ReviewDraw(SEED, 4), ReviewDraw(SEED, 4, 0.0, unk=1), ReviewDraw(SEED, 4, 1e-12, unk=1)):
        assert same.threshold == 0
        out = st.collate(idx, draw=same)
        for k in (0, 1, 2, 3, 4, 5, 7):
            assert torch.equal(out[k].cpu(), base[k].cpu())
    real = [(base[k] != 0).cpu() for k in range(3)]
    for p, pad in ((0.5, 0), (1 - 2.0 ** -33, 0), (0.5, 7)):
        out = check(mixed, idx, epoch=4, p=p, unk=1, pad=pad)
        for k in range(3):
            got, plain = out[k].cpu(), base[k].cpu()
            assert bool((got[~real[k]] == pad).all())                # padding stays padding
            hit = real[k] & (got == 1)
            assert bool((got[real[k] & ~hit] == plain[real[k] & ~hit]).all())      # a token is itself or <UNK>, where it was
            n, q = int(real[k].sum()), ref.threshold(p) / 2 ** 32
            assert abs(int(hit.sum()) - n * q) <= 5 * np.sqrt(n * q * (1 - q)) + 1, (k, p, int(hit.sum()), n)
            assert torch.equal(out[3 + k], base[3 + k])              # lengths never change
    # the ui rows are dropped (above, k = 2) but never sampled: without dropout they are the plain collate's
    assert torch.equal(base[2].cpu(), st.collate(idx)[2].cpu())
    assert not torch.equal(base[0].cpu(), st.collate(idx)[0].cpu())


# ---- refusals -------------------------------------------------------------------------------------------------------------------------
def test_refused_calls_leave_the_outputs_untouched(dev, mixed):
    from umpr_amd._lib import UmprHipError, lib
    from umpr_amd.reviews import ReviewDraw
    st = mixed.store
    buf = torch.full((8192,), SENTINEL, dtype=torch.int64, device=dev)
    lab = torch.full((16,), float("nan"), dtype=torch.float32, device=dev)
    t, s = st.d_row_ptr, st.d_sent_id
    cases = (([0, 40], 2, 4, 20, 0, -1, "outside the 40 samples"), ([0, -1], 2, 4, 20, 0, -1, "outside the 40 samples"),
             ([0, 3], 0, 4, 20, 0, -1, "bad shape"), ([0, 3], 2, 257, 20, 0, -1, "bad shape"),
             ([0, 3], 2, 4, 0, 0, -1, "keep = 0"), ([0, 3], 2, 4, 1025, 0, -1, "keep = 1025"), ([0, 3], 2, 4, -5, 0, -1, "keep = -5"),
             ([0, 3], 3, 4, 2, 0, -1, "S = 3 rows above keep = 2"), ([0, 3], 2, 4, 20, 1, -1, "without an unk id"),
             ([0, 3], 2, 4, 20, 2 ** 32 - 1, -1, "without an unk id"))
    for idx, S, L, keep, thr, unk, match in cases:
        host_idx = np.asarray(idx, dtype=np.int32)
        with pytest.raises(UmprHipError, match=match):
            lib().call("umpr_review_collate_sampled", st.d_tokens, st.d_sent_off, st.n_sent, t["user"], s["user"], t["item"], s["item"],
                       t["ui"], s["ui"], st.d_ratings, st.n_samples, host_idx.ctypes.data, 2, S, L, 1, 1, 0, keep, 12345, thr, unk,
                       buf, buf[4096:], lab, torch.cuda.current_stream().cuda_stream)
    with pytest.raises(IndexError, match="outside the 40 samples"):
        st.collate([0, 40], draw=ReviewDraw(1, 0))
    with pytest.raises(ValueError, match="an empty batch"):
        st.collate([], draw=ReviewDraw(1, 0))
    torch.cuda.synchronize()
    assert bool((buf.cpu() == SENTINEL).all()) and bool(lab.cpu().isnan().all())


# ---- the plain collate on a pooled store ----------------------------------------------------------------------------------------------
_TINY = {}


def tiny(level, dev):
    """the tiny corpus at max_sent_count 4: (Dataset, plain store, pooled Dataset, pooled store, Word2vec)"""
    if level not in _TINY:
        from umpr_amd.data import Dataset, Word2vec
        from umpr_amd.reviews import ReviewStore
        w2v = Word2vec(os.path.join(CORPUS, "glove.txt"))
        sets = []
        for review_pool in (0, 64):
            cfg = _cfg(max_sent_count=KEEP, min_sent_count=2, max_ui_sent_count=3, max_sent_length=10, photo_count=1, views=["food"],
                       review_level=level, review_pool=review_pool)
            ds = Dataset(os.path.join(CORPUS, "train.csv"), os.path.join(CORPUS, "photos.json"), os.path.join(CORPUS, "photos"), w2v,
                         cfg)
            sets += [ds, ReviewStore(ds, dev)]
        _TINY[level] = (*sets, w2v)
    return _TINY[level]


def _tiny_pools(level, dev):
    _, _, ds, store, w2v = tiny(level, dev)
    c = Pools.__new__(Pools)
    c.samples = [(u, i, ui, None, r) for u, i, ui, r in zip(*ds.pools, ds.data[2], ds.data[4])]
    c.keep, c.store, c.ds, c.w2v = KEEP, store, ds, w2v
    return c


@pytest.mark.parametrize("level", ("sentence", "review"))
def test_plain_collate_on_a_pooled_store_is_the_unpooled_stores(dev, level):
    from umpr_amd.data import batch_loader
    ds, plain, pooled_ds, pooled, _ = tiny(level, dev)
    assert pooled.keep == KEEP and plain.keep is None and pooled.nbytes > plain.nbytes
    n = len(ds)
    rng = np.random.default_rng(2)
    for idx, kw in (([5], {}), (np.arange(n), {}), (rng.permutation(n), dict(pad=7)), ([4, 11, 4, 4, 20], {}),
                    (rng.integers(0, n, size=7), dict(shard=(1, 2)))):
        a, b = plain.collate(idx, **kw), pooled.collate(idx, **kw)
        host = batch_loader([ds[int(k)] for k in idx], ignore_photos=True, **kw)
        assert len(a) == len(b) == len(host)
        for k, (x, y, h) in enumerate(zip(a, b, host)):
            assert x.dtype == y.dtype and x.shape == y.shape and torch.equal(x.cpu(), y.cpu()) and torch.equal(y.cpu(), h), k
    assert pooled.sampled == 0
    # and the sampled collate on the corpus, both review levels
    c = _tiny_pools(level, dev)
    check(c, np.arange(n), epoch=1, p=0.2, unk=c.w2v.word2index["<UNK>"])
    check(c, rng.integers(0, n, size=9), epoch=2)


# ---- the model ------------------------------------------------------------------------------------------------------------------------
def _model(dev, w2v, **kw):
    from umpr_amd.model import UMPR
    from umpr_amd.synthetic import make_param_state
    cfg = _cfg(**{**dict(max_sent_count=KEEP, min_sent_count=2, max_ui_sent_count=3, max_sent_length=10, photo_count=1,
                         views=["food"], review_net_only=True, batch_size=8, train_epochs=1, learning_rate=1e-3), **kw})
    P = make_param_state(91, w2v.embedding.shape[1], len(w2v), 1, True, m_scale=0.05)
    P["embedding.weight"] = torch.tensor(w2v.embedding, dtype=torch.float32)
    model = UMPR(cfg, w2v.embedding)
    model.load_state_dict(P)
    return model.to(dev), cfg


@pytest.mark.parametrize("mask_padding", (False, True))
def test_a_step_on_the_sampled_batch_is_the_step_on_the_host_definitions(dev, mask_padding):
    from umpr_amd.reviews import ReviewDraw
    c = _tiny_pools("sentence", dev)
    model, _ = _model(dev, c.w2v, mask_padding=mask_padding)
    assert model.mask_padding is mask_padding
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    idx = [3, 12, 7, 25, 7]
    host = ref.sampled_batch(c.samples, idx, SEED & ref.M64, 5, KEEP, 0.2, 1)
    plain = c.store.collate(idx)
    assert not torch.equal(host[0], plain[0].cpu())                   # the step is not the plain batch's
    a = _one_step(model, start, host)
    b = _one_step(model, start, c.store.collate(idx, draw=ReviewDraw(SEED, 5, 0.2, 1)))
    for what, xs, ys in zip(("prediction / loss", "gradients", "parameters and moments"), a, b):
        assert len(xs) == len(ys) > 0
        for x, y in zip(xs, ys):
            assert torch.equal(x, y), what
    assert any(bool(g.any()) for g in a[1]) and bool(torch.isfinite(a[0][1]))


def _loaders(c, plain_store, draw):
    from torch.utils.data import DataLoader
    from umpr_amd.reviews import IndexView, PhotoCollate, StoreLoader
    g = torch.Generator().manual_seed(0)
    train = StoreLoader(DataLoader(IndexView(c.ds), collate_fn=PhotoCollate(True), batch_size=8, shuffle=True, generator=g), c.store,
                        draw=draw)
    valid = StoreLoader(DataLoader(IndexView(c.ds), collate_fn=PhotoCollate(True), batch_size=8), plain_store)
    return train, valid


def test_training_resumed_inside_an_epoch_ends_on_the_uninterrupted_runs_bits(dev, tmp_path):
    """two shuffled epochs of UMPR-R at batch 8 (4 batches each) from a sampled loader; the only checkpoint is written behind step
    6 - epoch 1, two batches in; a fresh model, loader and draw resumed from it skip those two and draw what the first run drew"""
    from umpr_amd.reviews import ReviewDraw
    from umpr_amd.train import training
    c = _tiny_pools("sentence", dev)

    def run(resume, path):
        model, cfg = _model(dev, c.w2v, train_epochs=2, valid_every=6, resume=resume)
        torch.manual_seed(7)
        draw = ReviewDraw(None, 0, 0.1, 1)                            # torch.initial_seed()
        train, valid = _loaders(c, c.store, draw)
        lines = []
        before = c.store.sampled
        opt, saved = training(train, valid, model, cfg, path, logger=type("L", (), {"info": staticmethod(lines.append)}))
        torch.cuda.synchronize()
        assert draw.epoch == 1 and draw.seed == 7
        return [t.clone() for g_ in opt.groups for t in (g_.p, g_.m, g_.v)], saved, lines, c.store.sampled - before

    full, saved, _, sampled = run("", str(tmp_path / "full.pt"))
    assert saved and sampled == 8
    res, _, lines, sampled = run(str(tmp_path / "full.pt"), str(tmp_path / "res.pt"))
    assert any(ln.startswith("Resumed from") and "2 batches into the epoch" in ln for ln in lines), lines
    assert sampled == 4                                               # the whole epoch is collated, two batches are skipped
    for x, y in zip(full, res):
        assert torch.equal(x, y)


def test_validation_sees_what_it_sees_without_the_options(dev):
    from umpr_amd.train import evaluate_mse
    _, plain, _, pooled, _ = tiny("sentence", dev)
    c = _tiny_pools("sentence", dev)
    model, _ = _model(dev, c.w2v)
    before = pooled.sampled
    a = evaluate_mse(model, _loaders(c, plain, None)[1])
    b = evaluate_mse(model, _loaders(c, pooled, None)[1])
    assert a == b and pooled.sampled == before


def test_main_with_the_options(dev, tmp_path, monkeypatch, capsys):
    """main.py --review_pool / --word_dropout on a reference-layout directory: the setting and the share of samples with a large
    pool are logged, only the training set is pooled, and the initial validation is the run's without the options"""
    import importlib
    import shutil
    import sys
    d = tmp_path / "music"
    d.mkdir()
    for split in ("train", "valid", "test"):
        shutil.copy(os.path.join(CORPUS, "train.csv"), d / f"{split}.csv")
    shutil.copy(os.path.join(CORPUS, "photos.json"), d / "photos.json")
    (d / "photos").mkdir()
    argv = ["main.py", "--data_dir", str(d), "--word2vec_file", os.path.join(CORPUS, "glove.txt"), "--review_net_only", "True",
            "--train_epochs", "2", "--batch_size", "8", "--max_sent_count", "4", "--min_sent_count", "2", "--max_ui_sent_count", "3",
            "--max_sent_length", "10", "--views", "food", "--learning_rate", "1e-3", "--valid_every", "2", "--review_store", "True"]
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main")
    outs = []
    for extra in ([], ["--review_pool", "64", "--word_dropout", "0.25"]):
        monkeypatch.setattr(sys, "argv", argv + extra + ["--model_path", str(tmp_path / f"m{len(extra)}.pt")])
        torch.manual_seed(3)
        main.main()
        outs.append(capsys.readouterr().out)
    assert "Sampled collate" not in outs[0]
    assert "Sampled collate (train): a fresh draw of 4 sentences per user and item pool every epoch out of up to 64, word dropout " \
           "0.25" in outs[1], outs[1][-3000:]
    assert "100.0% of the 28 samples have a pool above 4 sentences" in outs[1]
    assert outs[1].count("Sampled collate") == 1
    first = [[ln.split(" ", 2)[2] for ln in o.splitlines() if "Initial validation mse" in ln] for o in outs]
    assert len(first[0]) == 1 and first[0] == first[1]
    stores = [[ln.split(" ", 2)[2] for ln in o.splitlines() if "Review store (" in ln] for o in outs]
    assert stores[0][1:] == stores[1][1:] and stores[0][0] != stores[1][0]      # valid and test: the stores they were
    later = [[ln.split(" ", 2)[2] for ln in o.splitlines() if "train loss" in ln and "valid mse" in ln] for o in outs]
    assert later[0] and later[0] != later[1]                                    # the training run is another one
