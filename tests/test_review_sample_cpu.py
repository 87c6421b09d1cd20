"""Per-epoch sampling of the review pools and word dropout (data.Dataset(review_pool=), reviews.ReviewTable(keep=) / .draw,
reviews.ReviewDraw, main.py --review_pool / --word_dropout), host half: the full pools beside the truncated ones, the pooled
table's plain shape arithmetic, the numpy definition of the draw against the plain-Python restatement of
tests/review_sample_reference.py, its statistics, and the refusals.  No GPU needed."""
import os

import numpy as np
import pytest
import torch

import review_sample_reference as ref
from conftest import GOLDEN
from test_feature_store import main_config  # noqa: F401  (fixture)

CORPUS = os.path.join(GOLDEN, "tiny_corpus")
KEEP = 4          # max_sent_count on the tiny corpus: most of its pools are larger


def _dataset(level, review_pool=0, **kw):
    from umpr_amd.config import Config
    from umpr_amd.data import Dataset, Word2vec
    cfg = Config(argv=[])
    for k, v in dict(max_sent_count=KEEP, min_sent_count=2, max_ui_sent_count=3, max_sent_length=10, photo_count=1, views=["food"],
                     review_level=level, **kw).items():
        setattr(cfg, k, v)
    if review_pool is not None:
        cfg.review_pool = review_pool
    w2v = Word2vec(os.path.join(CORPUS, "glove.txt"))
    return Dataset(os.path.join(CORPUS, "train.csv"), os.path.join(CORPUS, "photos.json"), os.path.join(CORPUS, "photos"), w2v, cfg)


# ---- Dataset --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ("sentence", "review"))
def test_the_truncated_pool_is_a_prefix_of_the_full_one(level):
    ds = _dataset(level, 64)
    users, items = ds.pools
    assert len(users) == len(items) == len(ds) > 0
    large = 0
    for k in (0, 1):
        for shown, pool in zip(ds.data[k], ds.pools[k]):
            assert shown == pool[:KEEP] and KEEP < 64 and len(pool) <= 64
            if len(pool) > KEEP:                      # sorted longest first, stably
                assert [len(s) for s in pool] == sorted((len(s) for s in pool), reverse=True)
    for u, i in zip(users, items):
        large += len(u) > KEEP or len(i) > KEEP
    assert 2 * large >= len(ds), (large, len(ds))     # at least half of the samples have something to draw from
    cut = _dataset(level, 6).pools                    # the cap itself
    assert max(len(p) for k in (0, 1) for p in cut[k]) == 6
    assert all(c == p[:6] for k in (0, 1) for c, p in zip(cut[k], ds.pools[k]))


@pytest.mark.parametrize("level", ("sentence", "review"))
def test_data_is_what_it_is_without_the_option(level):
    plain, absent, pooled = _dataset(level, 0), _dataset(level, None), _dataset(level, 64)
    assert plain.data == pooled.data == absent.data and plain.retain_idx == pooled.retain_idx
    assert not hasattr(plain, "pools") and not hasattr(absent, "pools")
    for bad in (KEEP, 1, -3, 1025):
        with pytest.raises(ValueError, match="review_pool"):
            _dataset(level, bad)
    _dataset(level, 1024), _dataset(level, KEEP + 1)


# ---- the table ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ("sentence", "review"))
def test_pooled_table_has_the_unpooled_tables_shapes_and_lengths(level):
    from umpr_amd.reviews import ROLES, ReviewStore
    plain, pooled = ReviewStore(_dataset(level, 0), "cpu"), ReviewStore(_dataset(level, 64), "cpu")
    assert plain.keep is None and pooled.keep == KEEP and pooled.n_samples == plain.n_samples
    assert pooled.sent_id["user"].size > plain.sent_id["user"].size
    rng = np.random.default_rng(0)
    for role in ROLES:
        for what in ("count", "longest", "lengths"):
            assert np.array_equal(getattr(plain, what)[role], getattr(pooled, what)[role]), (role, what)
    for idx in ([3], np.arange(plain.n_samples), rng.integers(0, plain.n_samples, size=9)):
        idx = np.asarray(idx)
        assert plain.shape(idx) == pooled.shape(idx)
        S, _, S_ui, _ = plain.shape(idx)
        for a, b in zip(plain.host_lengths(idx, S, S_ui), pooled.host_lengths(idx, S, S_ui)):
            assert torch.equal(a, b)
    # the first KEEP sentences of a pool are the truncated pool's
    for role in ROLES[:2]:
        for n in range(plain.n_samples):
            a = plain.sent_id[role][plain.row_ptr[role][n]:plain.row_ptr[role][n + 1]]
            b = pooled.sent_id[role][pooled.row_ptr[role][n]:][:len(a)]
            assert [tuple(plain.tokens[plain.sent_off[j]:plain.sent_off[j + 1]]) for j in a] == \
                   [tuple(pooled.tokens[pooled.sent_off[j]:pooled.sent_off[j + 1]]) for j in b]


def test_table_refusals_name_the_sample():
    from umpr_amd.reviews import ReviewTable
    s = [1, 2, 3]
    ok = [[s] * 1024, [s]]
    ReviewTable(ok, ok, [[s], [s]], [1.0, 2.0], keep=20)
    with pytest.raises(ValueError, match="the item pool of sample 1 holds 1025 sentences"):
        ReviewTable(ok, [[s], [s] * 1025], [[s], [s]], [1.0, 2.0], keep=20)
    ReviewTable(ok, [[s], [s] * 1025], [[s], [s]], [1.0, 2.0])             # no keep: as before, no bound
    for keep in (0, -1):
        with pytest.raises(ValueError, match="keep = "):
            ReviewTable(ok, ok, [[s], [s]], [1.0, 2.0], keep=keep)


# ---- the draw -------------------------------------------------------------------------------------------------------------------
def _table(sizes_u, sizes_i, keep, seed=1):
    from umpr_amd.reviews import ReviewTable
    rng = np.random.default_rng(seed)
    sent = lambda: [int(t) for t in rng.integers(3, 9000, size=int(rng.integers(0, 12)))]
    users = [[sent() for _ in range(k)] for k in sizes_u]
    items = [[sent() for _ in range(k)] for k in sizes_i]
    uis = [[sent() for _ in range(1 + n % 3)] for n in range(len(users))]
    ratings = [float(1 + n % 5) for n in range(len(users))]
    return ReviewTable(users, items, uis, ratings, keep=keep), list(zip(users, items, uis, [None] * len(users), ratings))


def test_numpy_draw_is_the_plain_python_definition():
    from umpr_amd.reviews import ReviewDraw
    sizes = [0, 1, 4, 5, 6, 63, 64, 65, 300, 1024]
    table, samples = _table(sizes, sizes[::-1], keep=5)
    for seed, epoch in ((0, 0), (0x123456789abcdef0fedcba, 3), (2 ** 64 - 1, 2 ** 40)):
        draw = ReviewDraw(seed, epoch)
        assert draw.key == ref.mix64((ref.mix64(seed & ref.M64) + epoch) & ref.M64)
        idx = np.asarray([9, 0, 3, 3, 8, 1, 2, 4, 5, 6, 7])
        got = table.draw(idx, draw)
        for r, role in enumerate(("user", "item")):
            pos, ln = got[role]
            for b, n in enumerate(idx):
                want = ref.positions(seed & ref.M64, epoch, int(n), role, len(samples[n][r]), 5)
                assert list(pos[b][:len(want)]) == want and (pos[b][len(want):] == -1).all()
                assert list(ln[b][:len(want)]) == [len(samples[n][r][j]) for j in want] and (ln[b][len(want):] == 0).all()
                assert len(set(want)) == len(want) == min(5, len(samples[n][r])) and all(0 <= j < len(samples[n][r]) for j in want)


def test_draw_depends_on_seed_epoch_and_sample_only():
    from umpr_amd.reviews import ReviewDraw
    table, _ = _table([50] * 12, [30] * 12, keep=20)
    a = table.draw(np.arange(12), ReviewDraw(7, 2))
    again = table.draw(np.arange(12), ReviewDraw(7, 2))
    other = np.asarray([5, 11, 5, 0])                                # other batch-mates, another place, a repeat
    b = table.draw(other, ReviewDraw(7, 2))
    stepped = ReviewDraw(7, 0)
    stepped.set_epoch(2)
    c = table.draw(np.arange(12), stepped)
    for role in ("user", "item"):
        for x, y in zip(a[role], again[role]):
            assert np.array_equal(x, y)
        for x, y in zip(a[role], c[role]):
            assert np.array_equal(x, y)
        assert np.array_equal(b[role][0], a[role][0][other])
        for n in range(12):
            assert len(set(a[role][0][n])) == 20 and a[role][0][n].min() >= 0
        for moved in (ReviewDraw(7, 3), ReviewDraw(8, 2)):           # another epoch, another seed: another draw
            d = table.draw(np.arange(12), moved)[role][0]
            assert all(not np.array_equal(d[n], a[role][0][n]) for n in range(12))
    assert not np.array_equal(a["user"][0][:, :20], a["item"][0][:, :20])      # the roles draw apart
    assert not np.array_equal(a["user"][0][0], a["user"][0][1])                # and so do the samples


def test_pools_that_fit_are_shuffled():
    from umpr_amd.data import batch_loader
    from umpr_amd.reviews import ReviewDraw
    sizes = [1, 2, 3, 4, 5, 5, 4, 3]
    table, samples = _table(sizes, sizes[::-1], keep=5)
    idx = list(range(len(sizes)))
    plain = batch_loader([samples[k] for k in idx], ignore_photos=True)
    moved = False
    for epoch in range(3):
        got = ref.sampled_batch(samples, idx, 3, epoch, 5)
        shape, lengths = table.drawn_shape(np.asarray(idx), ReviewDraw(3, epoch))
        assert shape == table.shape(np.asarray(idx)) and tuple(got[0].shape[1:]) == shape[:2]
        for k in (0, 1):
            assert torch.equal(torch.from_numpy(lengths[k]), got[3 + k])
            for b in idx:        # the rows of a sample are a permutation of its plain rows, the lengths travelling with them
                rows = sorted(map(tuple, torch.cat([got[k][b], got[3 + k][b][:, None]], 1).tolist()))
                assert rows == sorted(map(tuple, torch.cat([plain[k][b], plain[3 + k][b][:, None]], 1).tolist()))
            moved |= not torch.equal(got[k], plain[k])
        assert torch.equal(got[2], plain[2]) and torch.equal(got[5], plain[5]) and torch.equal(got[7], plain[7])
        assert torch.equal(torch.from_numpy(lengths[2]), got[5])
    assert moved


def test_host_shapes_and_lengths_of_a_sampled_batch():
    from umpr_amd.reviews import ReviewDraw
    sizes = [0, 1, 4, 5, 6, 63, 64, 65, 300, 1024]
    table, samples = _table(sizes, sizes[::-1], keep=5)
    rng = np.random.default_rng(4)
    for epoch, idx in enumerate(([0, 9], [1], [4, 4, 8], np.arange(10), rng.integers(0, 10, size=7))):
        idx = np.asarray(idx)
        want = ref.sampled_batch(samples, idx, 11, epoch, 5, p=0.3, unk=1)          # dropout changes no length
        shape, lengths = table.drawn_shape(idx, ReviewDraw(11, epoch, 0.3, 1))
        assert shape == (want[0].shape[1], want[0].shape[2], want[2].shape[1], want[2].shape[2])
        for k in range(3):
            assert torch.equal(torch.from_numpy(np.ascontiguousarray(lengths[k])), want[3 + k])


def test_every_sentence_of_a_pool_is_drawn_equally_often():
    """one pool of 50, keep 20, 4000 epochs: a sentence is picked Binomial(4000, 0.4) times - within 5 standard deviations of 1600
    - and lands in each of the 20 slots"""
    from umpr_amd.reviews import ReviewDraw
    table, _ = _table([50], [50], keep=20)
    picks, slots = np.zeros(50, dtype=np.int64), np.zeros((50, 20), dtype=np.int64)
    draw = ReviewDraw(12345, 0)
    for epoch in range(4000):
        draw.set_epoch(epoch)
        pos = table.draw(np.asarray([0]), draw)["user"][0][0]
        assert len(set(pos)) == 20
        picks[pos] += 1
        slots[pos, np.arange(20)] += 1
    sd = np.sqrt(4000 * 0.4 * 0.6)
    assert picks.sum() == 80000 and np.abs(picks - 1600).max() <= 5 * sd, picks
    assert np.abs(slots - 80).max() <= 5 * np.sqrt(4000 * 0.02 * 0.98), slots      # Binomial(4000, 1/50) per (sentence, slot)


@pytest.mark.parametrize("p", (0.1, 0.5, 0.999))
def test_dropout_rate(p):
    """10^6 positions: 16 samples x 3 roles x 82 rows x 256 tokens; the rate lies within 5 binomial sigma of p"""
    from umpr_amd.reviews import ReviewDraw
    draw = ReviewDraw(99, 4, p, unk=1)
    assert draw.threshold == ref.threshold(p) == int(p * 2 ** 32)
    idx = np.arange(100, 116)
    masks = [draw.drop_mask(idx, role, 82, 256) for role in range(3)]
    n = sum(m.size for m in masks)
    hits = sum(int(m.sum()) for m in masks)
    assert n > 10 ** 6
    assert abs(hits - n * p) <= 5 * np.sqrt(n * p * (1 - p)), (hits, n)
    assert not np.array_equal(masks[0], masks[1]) and not np.array_equal(masks[0][0], masks[0][1])
    # against the plain-Python definition, on real sentences
    sents = [[7] * 256, [8] * 3, [], [9] * 65]
    for role in ("user", "ui"):
        got = ref.dropped(99, 4, 103, role, sents, p, 1)
        m = masks[ref.ROLE[role]][3]
        assert got == [[1 if m[s, l] else t for l, t in enumerate(sent)] for s, sent in enumerate(sents)]


def test_dropout_edges():
    from umpr_amd.reviews import ReviewDraw
    assert ReviewDraw(1, 0, 0.0).threshold == 0 and not ReviewDraw(1, 0, 0.0).drop_mask(np.arange(3), 0, 4, 5).any()
    assert ReviewDraw(1, 0, 1e-12, unk=1).threshold == 0                  # below 2^-32: the no-dropout call
    assert ReviewDraw(1, 0, 1 - 2.0 ** -40, unk=1).threshold == 2 ** 32 - 1
    assert ReviewDraw(None).seed == torch.initial_seed() & ref.M64
    for bad in (1.0, -0.1, 2):
        with pytest.raises(ValueError, match="word_dropout must lie in"):
            ReviewDraw(1, 0, bad, unk=1)
    with pytest.raises(ValueError, match="needs the id of <UNK>"):
        ReviewDraw(1, 0, 0.5)


# ---- loader and main.py -----------------------------------------------------------------------------------------------------------
def test_loaders_pass_the_epoch_on():
    import main
    from umpr_amd.reviews import ReviewDraw, StoreLoader
    from umpr_amd.train import _set_epoch
    draw = ReviewDraw(5, 0)
    key0 = draw.key
    sl = StoreLoader([], None, draw=draw)
    _set_epoch(main.ShardedLoader(sl, 0, 1), 3)
    assert draw.epoch == 3 and draw.key != key0 and draw.key == ReviewDraw(5, 3).key
    _set_epoch(sl, 0)
    assert draw.key == key0
    off = StoreLoader([], None)
    _set_epoch(main.ShardedLoader(off, 0, 1), 3)                          # nothing to tell
    assert off.draw is None
    _set_epoch(main.ShardedLoader([], 0, 1), 3), _set_epoch([], 3)        # loaders without the method


def test_main_flags(main_config):
    import main
    cfg = main_config()
    assert cfg.review_pool == 0 and cfg.word_dropout == 0.0
    main.check_flags(cfg)
    real = ("--data_dir", "data/music", "--review_store", "True")
    for ok in (real + ("--review_pool", "200"), real + ("--word_dropout", "0.1"), real + ("--review_pool", "21", "--word_dropout", "0.5"),
               real + ("--review_pool", "1024"), real + ("--review_pool", "0", "--word_dropout", "0")):
        main.check_flags(main_config(*ok))
    refused = {real + ("--review_pool", "20"): "--review_pool takes 0",                      # max_sent_count itself
               real + ("--review_pool", "1025"): "--review_pool takes 0",
               real + ("--review_pool", "-1"): "--review_pool takes 0",
               real + ("--review_pool", "True"): "--review_pool takes 0",
               real + ("--review_pool", "30.5"): "--review_pool takes 0",
               real + ("--word_dropout", "1"): "--word_dropout takes the share",
               real + ("--word_dropout", "-0.1"): "--word_dropout takes the share",
               real + ("--word_dropout", "True"): "--word_dropout takes the share",
               ("--data_dir", "data/music", "--review_pool", "200"): "--review_pool needs --review_store True",
               ("--data_dir", "data/music", "--word_dropout", "0.1"): "--word_dropout needs --review_store True",
               ("--data_dir", "synthetic", "--review_store", "True", "--review_pool", "200"): "--review_pool needs tokenised reviews",
               ("--data_dir", "synthetic", "--review_store", "True", "--word_dropout", "0.1"):
                   "--word_dropout needs tokenised reviews"}
    for argv, text in refused.items():
        with pytest.raises(SystemExit, match=text):
            main.check_flags(main_config(*argv))
    cfg = main_config(*real, "--review_pool", "200")
    plain = main._unpooled(cfg)                                            # what the validation and test Datasets read
    assert plain.review_pool == 0 and plain.max_sent_count == 20 and cfg.review_pool == 200
