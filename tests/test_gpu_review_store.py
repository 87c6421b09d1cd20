"""The review store on the GPU (umpr_amd/reviews.py::ReviewStore, csrc/reviews.hip::umpr_review_collate): the ids, lengths and
labels of a batch collated on the device from its sample indices against data.batch_loader(..., ignore_photos=True) on the same
samples - torch.equal everywhere - with the outputs pre-filled with a sentinel between guard bands; then the model, evaluate_mse
and training() fed from the store against the same fed from batch_loader, bit for bit."""
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN

pytestmark = pytest.mark.gpu

CORPUS = os.path.join(GOLDEN, "tiny_corpus")
GUARD = 512                      # int64 / float32 elements in front of, between and behind the outputs
SENTINEL = -0x5a5a5a5a5a5a5a5a   # no token id, no pad


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _cfg(**kw):
    from umpr_amd.config import Config
    cfg = Config(argv=[])
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


class Corpus:
    """samples as batch_loader takes them + the store built from the same lists"""

    def __init__(self, users, items, uis, ratings, store):
        self.samples = [(u, i, ui, None, r) for u, i, ui, r in zip(users, items, uis, ratings)]
        self.store = store

    def reference(self, idx, pad=0, shard=None):
        from umpr_amd.data import batch_loader
        return batch_loader([self.samples[int(k)] for k in idx], ignore_photos=True, pad=pad, shard=shard)


_TINY = {}


def tiny(level, dev):
    if level not in _TINY:
        from umpr_amd.data import Dataset, Word2vec
        from umpr_amd.reviews import ReviewStore
        cfg = _cfg(max_sent_count=6, min_sent_count=2, max_ui_sent_count=3, max_sent_length=10, photo_count=1, views=["food"],
                   review_level=level)
        w2v = Word2vec(os.path.join(CORPUS, "glove.txt"))
        ds = Dataset(os.path.join(CORPUS, "train.csv"), os.path.join(CORPUS, "photos.json"), os.path.join(CORPUS, "photos"), w2v, cfg)
        c = Corpus(*ds.data[:3], ds.data[4], ReviewStore(ds, dev))
        c.ds, c.w2v = ds, w2v
        _TINY[level] = c
    return _TINY[level]


@pytest.fixture(scope="module")
def edge(dev):
    """48 samples over a pool of sentences of lengths 1, 2, 63, 64, 65, 255, 256 (two each) and 30 of 3..40 tokens, ids up to
    400 002.  Samples 0..7 are hand-made edges; samples 8.. draw sentences of at most 65 tokens (the large batches use them)."""
    from umpr_amd.reviews import ReviewStore
    rng = np.random.default_rng(11)
    sent = lambda n: [int(t) for t in rng.integers(0, 400003, size=n)]
    by_len = {n: [sent(n), sent(n)] for n in (1, 2, 63, 64, 65, 255, 256)}
    by_len[256][0][255] = 400002
    by_len[1][0][0] = 400002
    short = [sent(int(n)) for n in rng.integers(3, 41, size=30)] + [s for n in (1, 2, 63, 64, 65) for s in by_len[n]]
    every = short + by_len[255] + by_len[256]
    draw = lambda pool, n: [pool[int(j)] for j in rng.integers(0, len(pool), size=n)]
    users = [[by_len[1][0]], draw(short, 20), draw(short, 2), [by_len[2][0]], draw(short, 5) + [by_len[255][0]], [by_len[256][1]],
             draw(every, 20), [by_len[64][0], by_len[63][0], by_len[65][0]]]
    items = [[by_len[1][1]], draw(short, 3), draw(short, 19) + [by_len[256][0]], [by_len[1][0]], draw(short, 4), [by_len[255][1]],
             draw(every, 20), [by_len[65][1], by_len[64][1]]]
    uis = [[by_len[1][0]], draw(short, 5), [by_len[256][0], by_len[2][1]], [by_len[1][1]], draw(every, 3), [by_len[255][0]],
           draw(short, 1), [by_len[63][1], by_len[1][0]]]
    for _ in range(40):
        users.append(draw(short, int(rng.integers(1, 21))))
        items.append(draw(short, int(rng.integers(1, 21))))
        uis.append(draw(short, int(rng.integers(1, 6))))
    ratings = [float(r) for r in rng.integers(1, 6, size=len(users))]
    ratings[5] = 3.7
    return Corpus(users, items, uis, ratings, ReviewStore.from_lists(users, items, uis, ratings, dev))


def check(corpus, idx, pad=0, shard=None):
    """both ways to the kernel against batch_loader on the same samples: the C entry point writing between guard bands into
    sentinel-filled buffers, and ReviewStore.collate"""
    from umpr_amd._lib import lib
    from umpr_amd.parallel import active_shards, shard_bounds
    st = corpus.store
    idx = np.asarray(idx, dtype=np.int64)
    ref = corpus.reference(idx, pad, shard)
    lo, hi = shard_bounds(len(idx), *shard) if shard else (0, len(idx))
    B, (S, L, S_ui, L_ui) = hi - lo, st.shape(idx)
    assert tuple(ref[0].shape) == tuple(ref[1].shape) == (B, S, L) and tuple(ref[2].shape) == (B, S_ui, L_ui)
    served = st.stats()["batches"]
    if B:
        n_pair, n_ui = 2 * B * S * L, B * S_ui * L_ui
        buf = torch.full((GUARD + n_pair + GUARD + n_ui + GUARD,), SENTINEL, dtype=torch.int64, device=st.device)
        lab = torch.full((GUARD + B + GUARD,), float("nan"), dtype=torch.float32, device=st.device)
        host_idx = np.ascontiguousarray(idx[lo:hi], dtype=np.int32)
        p, s = st.d_row_ptr, st.d_sent_id
        lib().call("umpr_review_collate", st.d_tokens, st.d_sent_off, st.n_sent, p["user"], s["user"], p["item"], s["item"], p["ui"],
                   s["ui"], st.d_ratings, st.n_samples, host_idx.ctypes.data, B, S, L, S_ui, L_ui, pad,
                   buf.data_ptr() + 8 * GUARD, buf.data_ptr() + 8 * (2 * GUARD + n_pair), lab.data_ptr() + 4 * GUARD,
                   torch.cuda.current_stream().cuda_stream)
        got, labels = buf.cpu(), lab.cpu()
        for a, b in ((0, GUARD), (GUARD + n_pair, 2 * GUARD + n_pair), (2 * GUARD + n_pair + n_ui, len(got))):
            assert bool((got[a:b] == SENTINEL).all()), "a guard band was written"
        assert bool(labels[:GUARD].isnan().all()) and bool(labels[GUARD + B:].isnan().all())
        pair = got[GUARD:GUARD + n_pair].view(2, B, S, L)
        assert torch.equal(pair[0], ref[0]) and torch.equal(pair[1], ref[1])
        assert torch.equal(got[2 * GUARD + n_pair:2 * GUARD + n_pair + n_ui].view(B, S_ui, L_ui), ref[2])
        assert torch.equal(labels[GUARD:GUARD + B], ref[7])
    out = st.collate(idx, pad=pad, shard=shard)
    assert st.stats()["batches"] == served + (1 if B else 0)          # an empty chunk launches nothing
    assert len(out) == len(ref) == (9 if shard else 8)
    for k in (0, 1, 2, 7):
        assert out[k].device == st.device and out[k].dtype == ref[k].dtype and out[k].is_contiguous()
    for k in (3, 4, 5, 6):
        assert out[k].device.type == "cpu" and out[k].dtype == ref[k].dtype
    for k, (g, r) in enumerate(zip(out, ref)):
        assert g.shape == r.shape and torch.equal(g.cpu(), r), k
    assert out[7].dtype == torch.float32 and out[3].dtype == torch.int64
    # the halves of one allocation, item ids right behind the user ids: UMPR._forward takes them as its ids_pair
    assert out[1].untyped_storage().data_ptr() == out[0].untyped_storage().data_ptr()
    if B:
        assert out[1].data_ptr() == out[0].data_ptr() + B * S * L * 8
    if shard:
        assert int(out[8]) == active_shards(len(idx), shard[1])
    return out


# ---- the tiny corpus ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", ("sentence", "review"))
def test_tiny_corpus_batches_equal_batch_loaders(dev, level):
    c = tiny(level, dev)
    n = len(c.samples)
    rng = np.random.default_rng(3)
    check(c, [5])
    check(c, [n - 1])
    check(c, [2, 17, 9])
    check(c, np.arange(n))
    check(c, rng.permutation(n))
    check(c, [4, 11, 4, 4, 20])                                    # one sample three times: identical rows
    check(c, [2, 17, 9], pad=7)
    check(c, np.arange(n), pad=7)
    for shard in ((0, 2), (1, 2), (2, 3)):
        check(c, rng.integers(0, n, size=7), shard=shard)
        check(c, np.arange(n), shard=shard, pad=7)
    for rank in range(4):                                          # 5 samples over 4 ranks: chunks of 2, 2, 1 and none
        out = check(c, [3, 1, 8, 8, 22], shard=(rank, 4))
        assert out[0].shape[0] == (2, 2, 1, 0)[rank] and int(out[8]) == 3


def test_repeated_sample_rows_are_identical(dev):
    c = tiny("sentence", dev)
    out = c.store.collate([6, 13, 6, 6])
    for k in (0, 1, 2, 3, 4, 5, 7):
        assert torch.equal(out[k][0], out[k][2]) and torch.equal(out[k][0], out[k][3])


# ---- the edge corpus ------------------------------------------------------------------------------------------------------------
def test_edge_lengths_counts_and_shared_shapes(dev, edge):
    assert int(edge.store.d_tokens.max()) == 400002
    out = check(edge, [0, 3])                                      # one sentence of one token everywhere
    assert tuple(out[0].shape) == (2, 1, 2) and tuple(out[2].shape) == (2, 1, 1)
    out = check(edge, [0, 1])                                      # one sentence next to twenty
    assert out[0].shape[0] == 2 and out[0].shape[1] == 20
    assert check(edge, [1])[0].shape[1] == 20                      # the user pool sets S ...
    out = check(edge, [2])                                         # ... or the item pool does, and L = 256 comes from it too
    assert tuple(out[0].shape) == (1, 20, 256) and tuple(out[2].shape) == (1, 2, 256)
    assert tuple(check(edge, [4])[0].shape) == (1, 6, 255)         # L from the user side
    assert tuple(check(edge, [5])[2].shape) == (1, 1, 255)
    check(edge, [7])                                               # 63, 64, 65: both sides of a wave of lanes
    check(edge, [7, 0], pad=400003)
    check(edge, np.arange(8))
    check(edge, [6, 2, 6, 5], pad=7, shard=(1, 2))


@pytest.mark.parametrize("B", (64, 65, 256, 257))
def test_edge_batch_sizes_around_the_one_launch_bound(dev, edge, B):
    rng = np.random.default_rng(B)
    idx = rng.integers(8, len(edge.samples), size=B)               # with repeats; sentences of at most 65 tokens
    out = check(edge, idx)
    assert out[0].shape[0] == B and out[0].shape[2] <= 65


def test_refused_calls_leave_the_outputs_untouched(dev, edge):
    from umpr_amd._lib import UmprHipError, lib
    st = edge.store
    buf = torch.full((4096,), SENTINEL, dtype=torch.int64, device=dev)
    lab = torch.full((16,), float("nan"), dtype=torch.float32, device=dev)
    p, s = st.d_row_ptr, st.d_sent_id
    for idx, S, L, match in (([0, 48], 1, 2, "outside the 48 samples"), ([0, -1], 1, 2, "outside the 48 samples"),
                             ([0, 3], 0, 2, "bad shape"), ([0, 3], 1, 257, "bad shape")):
        host_idx = np.asarray(idx, dtype=np.int32)
        with pytest.raises(UmprHipError, match=match):
            lib().call("umpr_review_collate", st.d_tokens, st.d_sent_off, st.n_sent, p["user"], s["user"], p["item"], s["item"],
                       p["ui"], s["ui"], st.d_ratings, st.n_samples, host_idx.ctypes.data, 2, S, L, 1, 1, 0, buf, buf[2048:], lab,
                       torch.cuda.current_stream().cuda_stream)
    with pytest.raises(IndexError, match="outside the 48 samples"):
        st.collate([0, 48])
    assert bool((buf.cpu() == SENTINEL).all()) and bool(lab.cpu().isnan().all())


def test_truncation_instead_of_an_out_of_bounds_write(dev, edge):
    """a count above S and a sentence longer than L cannot come from collate(); the kernel clips both"""
    from umpr_amd._lib import lib
    st = edge.store
    B, S, L, S_ui, L_ui = 2, 3, 7, 1, 2                              # samples 1 and 2 hold 20 sentences of up to 256 tokens
    n_pair, n_ui = 2 * B * S * L, B * S_ui * L_ui
    buf = torch.full((GUARD + n_pair + GUARD + n_ui + GUARD,), SENTINEL, dtype=torch.int64, device=dev)
    lab = torch.empty(B, dtype=torch.float32, device=dev)
    host_idx = np.asarray([1, 2], dtype=np.int32)
    p, s = st.d_row_ptr, st.d_sent_id
    lib().call("umpr_review_collate", st.d_tokens, st.d_sent_off, st.n_sent, p["user"], s["user"], p["item"], s["item"], p["ui"],
               s["ui"], st.d_ratings, st.n_samples, host_idx.ctypes.data, B, S, L, S_ui, L_ui, 0, buf.data_ptr() + 8 * GUARD,
               buf.data_ptr() + 8 * (2 * GUARD + n_pair), lab, torch.cuda.current_stream().cuda_stream)
    got = buf.cpu()
    for a, b in ((0, GUARD), (GUARD + n_pair, 2 * GUARD + n_pair), (2 * GUARD + n_pair + n_ui, len(got))):
        assert bool((got[a:b] == SENTINEL).all())
    ref = edge.reference([1, 2])
    pair = got[GUARD:GUARD + n_pair].view(2, B, S, L)
    assert torch.equal(pair[0], ref[0][:, :S, :L]) and torch.equal(pair[1], ref[1][:, :S, :L])
    assert torch.equal(got[2 * GUARD + n_pair:2 * GUARD + n_pair + n_ui].view(B, S_ui, L_ui), ref[2][:, :S_ui, :L_ui])


# ---- the model fed from the store ---------------------------------------------------------------------------------------------------
def _model(dev, c, review_net_only):
    from umpr_amd.model import UMPR
    from umpr_amd.synthetic import make_param_state
    cfg = _cfg(max_sent_count=6, min_sent_count=2, max_ui_sent_count=3, max_sent_length=10, photo_count=1, views=["food"],
               review_net_only=review_net_only, batch_size=8, train_epochs=1, learning_rate=1e-3)
    E = c.w2v.embedding.shape[1]
    P = make_param_state(91, E, len(c.w2v), 1, review_net_only, m_scale=0.05)
    P["embedding.weight"] = torch.tensor(c.w2v.embedding, dtype=torch.float32)
    model = UMPR(cfg, c.w2v.embedding)
    model.load_state_dict(P)
    return model.to(dev), cfg


def _one_step(model, start, batch):
    """(prediction, loss, gradient arenas, parameters and Adam moments) of one training step on `batch` from `start`"""
    from umpr_amd.optim import FusedAdam
    from umpr_amd.train import train_step
    torch.manual_seed(5)
    model.load_state_dict(start)
    for m in model.modules():
        if hasattr(m, "_calls"):
            m._calls = 0
    opt = FusedAdam(model, 1e-3, 1e-3)
    pred, loss = train_step(model, opt, batch)
    torch.cuda.synchronize()
    return ([pred.detach().cpu(), loss.detach().cpu()], [a.detach().cpu().clone() for a in opt.grad_arenas()],
            [t.detach().cpu().clone() for g in opt.groups for t in (g.p, g.m, g.v)])


@pytest.mark.parametrize("review_net_only", (True, False))
def test_a_step_on_the_stores_batch_is_the_step_on_batch_loaders(dev, review_net_only):
    c = tiny("sentence", dev)
    model, _ = _model(dev, c, review_net_only)
    start = {k: v.detach().clone() for k, v in model.state_dict().items()}
    idx = [3, 12, 7, 25] if review_net_only else [3, 12]
    host = list(c.reference(idx))
    photos = None
    if not review_net_only:                                           # B = 2, V = 1, one photo each, as a float tensor
        photos = torch.rand(2, 1, 1, 3, 224, 224, generator=torch.Generator().manual_seed(1))
        host[6] = photos
    stored = c.store.collate(idx, photos=photos)
    a, b = _one_step(model, start, tuple(host)), _one_step(model, start, stored)
    for what, xs, ys in zip(("prediction / loss", "gradients", "parameters and moments"), a, b):
        assert len(xs) == len(ys) > 0
        for x, y in zip(xs, ys):
            assert torch.equal(x, y), what
    assert any(bool(g.any()) for g in a[1]) and bool(torch.isfinite(a[0][1]))


def test_evaluate_mse_from_the_store(dev):
    from umpr_amd.train import evaluate_mse
    c = tiny("sentence", dev)
    model, _ = _model(dev, c, True)
    picks = [[0, 5, 9, 2], [27, 1, 1], [14]]
    assert evaluate_mse(model, [c.store.collate(i) for i in picks]) == evaluate_mse(model, [c.reference(i) for i in picks])


def test_training_with_and_without_the_store_ends_on_the_same_bits(dev, tmp_path):
    """one shuffled epoch of UMPR-R at batch 8: the sample DataLoader with batch_loader against the index DataLoader with the
    review store behind it - same generator, same order, same parameters and Adam moments at the end"""
    from torch.utils.data import DataLoader
    from umpr_amd.data import batch_loader
    from umpr_amd.reviews import IndexView, PhotoCollate, StoreLoader
    from umpr_amd.train import training
    c = tiny("sentence", dev)
    ends = []
    for use_store in (False, True):
        model, cfg = _model(dev, c, True)
        torch.manual_seed(7)
        g = torch.Generator().manual_seed(0)
        kw = dict(batch_size=8, shuffle=True, generator=g)
        if use_store:
            served = c.store.stats()["batches"]
            train = StoreLoader(DataLoader(IndexView(c.ds), collate_fn=PhotoCollate(True), **kw), c.store)
            valid = [c.store.collate([0, 1, 2])]
        else:
            train = DataLoader(c.ds, collate_fn=lambda x: batch_loader(x, True), **kw)
            valid = [c.reference([0, 1, 2])]
        lines = []
        opt, _ = training(train, valid, model, cfg, str(tmp_path / f"m{use_store}.pt"),
                          logger=type("L", (), {"info": staticmethod(lines.append)}))
        torch.cuda.synchronize()
        assert opt.step_count == 4                                    # 28 samples: 8, 8, 8, 4
        ends.append(([t.clone() for g_ in opt.groups for t in (g_.p, g_.m, g_.v)], [ln for ln in lines if "Time used" not in ln
                                                                                   and "samples/s" not in ln]))
    assert c.store.stats()["batches"] == served + 5
    assert ends[0][1] == ends[1][1]                                   # the validation lines carry the same numbers
    for x, y in zip(ends[0][0], ends[1][0]):
        assert torch.equal(x, y)


def test_main_with_the_option_reports_what_it_reports_without(dev, tmp_path, monkeypatch, capsys):
    """main.py --review_store True on a reference-layout directory: a store per Dataset is logged, and the run - same seed, same
    shuffle - ends on the test MSE of the run without the option.  In-process (argv patched), like the CLI test of test_gpu_e2e."""
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
            "--train_epochs", "1", "--batch_size", "8", "--max_sent_count", "6", "--min_sent_count", "2", "--max_ui_sent_count", "3",
            "--max_sent_length", "10", "--views", "food", "--learning_rate", "1e-3", "--valid_every", "2"]
    for k in ("RANK", "WORLD_SIZE", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    monkeypatch.chdir(tmp_path)
    main = importlib.import_module("main")
    outs = []
    for flag in ("False", "True"):
        monkeypatch.setattr(sys, "argv", argv + ["--review_store", flag, "--model_path", str(tmp_path / f"m{flag}.pt")])
        torch.manual_seed(3)
        main.main()
        outs.append(capsys.readouterr().out)
    assert "Review store" not in outs[0]
    for name in ("train", "valid", "test"):
        assert f"Review store ({name}): ReviewStore(28 samples" in outs[1], outs[1][-2000:]
    numbers = [[ln.split(" ", 2)[2] for ln in o.splitlines() if "mse" in ln] for o in outs]     # without date and time
    assert len(numbers[0]) >= 3 and "Test end, test mse is" in numbers[0][-1]
    assert numbers[0] == numbers[1]
