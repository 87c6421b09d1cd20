"""The review store (umpr_amd/reviews.py, --review_store): everything that can be checked without a GPU - the de-duplicated
arena and the CSR tables against Dataset.data, the host lengths and batch shapes against batch_loader, the option, the index
DataLoader against the sample DataLoader, and every refusal of umpr_review_collate (pure host code)."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from umpr_amd.data import Dataset, Word2vec, batch_loader

CORPUS = os.path.join(GOLDEN, "tiny_corpus")
LEVELS = ("sentence", "review")


class Cfg:
    max_sent_count = 6
    min_sent_count = 2
    max_ui_sent_count = 3
    max_sent_length = 10
    photo_count = 2
    views = ["food"]
    review_level = "sentence"


_DATA = {}


def tiny(level):
    """(Dataset, CPU ReviewStore) of the tiny corpus at `level`, built once"""
    if level not in _DATA:
        from umpr_amd.reviews import ReviewStore
        cfg = Cfg()
        cfg.review_level = level
        ds = Dataset(os.path.join(CORPUS, "train.csv"), os.path.join(CORPUS, "photos.json"), os.path.join(CORPUS, "photos"),
                     Word2vec(os.path.join(CORPUS, "glove.txt")), cfg)
        _DATA[level] = ds, ReviewStore(ds, "cpu")
    return _DATA[level]


# ---- the tables -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("level", LEVELS)
def test_every_distinct_sentence_is_stored_once_and_the_tables_reproduce_the_dataset(level):
    ds, st = tiny(level)
    assert st.n_samples == len(ds) == {"sentence": 28, "review": 29}[level]
    tokens, off = st.d_tokens.numpy(), st.d_sent_off.numpy()
    assert st.d_tokens.dtype == torch.int32 and st.d_sent_off.dtype == torch.int64 and st.d_ratings.dtype == torch.float32
    assert off[0] == 0 and off[-1] == len(tokens) and len(off) == st.n_sent + 1
    stored = [tuple(tokens[off[j]:off[j + 1]].tolist()) for j in range(st.n_sent)]
    assert len(set(stored)) == len(stored)
    distinct = []                                                  # first seen first: users, then items, then uis
    for pools in ds.data[:3]:
        for sents in pools:
            for s in sents:
                if tuple(s) not in distinct:
                    distinct.append(tuple(s))
    assert stored == distinct
    for role, pools in zip(("user", "item", "ui"), ds.data[:3]):
        ptr, sid = st.d_row_ptr[role].numpy(), st.d_sent_id[role].numpy()
        assert st.d_row_ptr[role].dtype == torch.int64 and st.d_sent_id[role].dtype == torch.int32
        assert len(ptr) == len(ds) + 1 and ptr[-1] == len(sid)
        got = [[list(stored[j]) for j in sid[ptr[k]:ptr[k + 1]]] for k in range(len(ds))]
        assert got == pools
    assert torch.equal(st.d_ratings, torch.Tensor(ds.data[4]))
    per_sample = sum(len(s) for pools in ds.data[:3] for sents in pools for s in sents)
    assert st.stats()["tokens"] == len(tokens) < per_sample == st.stats()["per_sample_tokens"]
    assert st.stats()["bytes"] == st.nbytes == 4 * len(tokens) + 8 * len(off) + 3 * 8 * (len(ds) + 1) + 4 * len(ds) + \
        4 * sum(len(st.d_sent_id[r]) for r in st.d_sent_id)


@pytest.mark.parametrize("level", LEVELS)
def test_host_lengths_and_shapes_equal_batch_loaders(level):
    ds, st = tiny(level)
    rng = np.random.default_rng(5)
    batches = [rng.integers(0, len(ds), size=int(rng.integers(1, 13))) for _ in range(200)]      # with repeats
    batches += [np.array([k]) for k in range(len(ds))] + [np.arange(len(ds))]
    for idx in batches:
        ref = batch_loader([ds[int(i)] for i in idx], ignore_photos=True)
        S, L, S_ui, L_ui = st.shape(st.checked(idx))
        assert (len(idx), S, L) == tuple(ref[0].shape) == tuple(ref[1].shape) and (len(idx), S_ui, L_ui) == tuple(ref[2].shape)
        got = st.host_lengths(idx, S, S_ui)
        for g, r in zip(got, ref[3:6]):
            assert g.dtype == torch.int64 and g.device.type == "cpu" and torch.equal(g, r)


def test_indices_are_checked_on_the_host():
    _, st = tiny("sentence")
    for bad in ([0, 28], [-1], [3, 1 << 40]):
        with pytest.raises(IndexError, match="outside the 28 samples"):
            st.checked(bad)
    with pytest.raises(ValueError, match="empty batch"):
        st.checked([])


def test_collate_has_no_cpu_path():
    _, st = tiny("sentence")
    with pytest.raises(RuntimeError, match="no CPU path"):
        st.collate([0, 1])
    assert st.stats()["batches"] == 0


def test_from_lists_checks_its_lists():
    from umpr_amd.reviews import ReviewStore
    st = ReviewStore.from_lists([[[5, 6]]], [[[5, 6], [7]]], [[[7]]], [4.0], "cpu")
    assert st.n_sent == 2 and st.d_tokens.tolist() == [5, 6, 7] and st.shape(np.array([0])) == (2, 2, 1, 1)
    with pytest.raises(ValueError, match="pools and 2 ratings"):
        ReviewStore.from_lists([[[1]]], [[[1]]], [[[1]]], [1.0, 2.0], "cpu")
    with pytest.raises(ValueError, match="int32"):
        ReviewStore.from_lists([[[1 << 31]]], [[[1]]], [[[1]]], [1.0], "cpu")


# ---- the option -----------------------------------------------------------------------------------------------------------------
@pytest.fixture
def main_config():
    import main
    from umpr_amd.config import Config
    saved = Config._extra
    Config.extend(main.EXTRA_OPTIONS)
    yield lambda *argv: Config(argv=list(argv))
    Config._extra = saved


def test_review_store_flag(main_config):
    import main
    cfg = main_config()
    assert cfg.review_store is False
    main.check_flags(cfg)
    assert main_config("--review_store", "True").review_store is True
    assert main_config("--review_store", "False").review_store is False
    main.check_flags(main_config("--review_store", "True", "--review_net_only", "True"))
    main.check_flags(main_config("--review_store", "True", "--freeze_conv", "True", "--pool5_store_gb", "1", "--train_embedding", "True",
                                 "--sparse_embedding", "True", "--grad_clip", "5.0", "--loader_workers", "4", "--dtype", "bf16"))
    main.check_flags(main_config("--review_store", "True", "--freeze_vgg", "True", "--feature_store_gb", "1", "--accum_steps", "4"))
    for bad in ("1", "0", "'yes'", "0.5"):
        with pytest.raises(SystemExit, match="--review_store takes True or False"):
            main.check_flags(main_config("--review_store", bad))


# ---- the index DataLoader -------------------------------------------------------------------------------------------------------
def _samples(batch):
    return batch


def _epoch(ds, workers, state, index):
    """one shuffled epoch's batches from `state` of the generator: the samples themselves, or (indices, photo paths)"""
    from torch.utils.data import DataLoader
    from umpr_amd.reviews import IndexView, PhotoCollate
    g = torch.Generator().manual_seed(0)
    if state is not None:
        g.set_state(state)
    kw = dict(batch_size=5, shuffle=True, generator=g, num_workers=workers)
    if index:
        return [b[0] for b in DataLoader(IndexView(ds), collate_fn=PhotoCollate(True), **kw)], g
    return list(DataLoader(ds, collate_fn=_samples, **kw)), g


@pytest.mark.parametrize("workers", (0, 2))
def test_index_loader_draws_the_batches_of_the_sample_loader(workers):
    ds, _ = tiny("sentence")
    g0 = torch.Generator().manual_seed(0)
    torch.randperm(7, generator=g0)                                 # a state from the middle of a run
    for state in (None, g0.get_state()):
        ref, g_ref = _epoch(ds, workers, state, index=False)
        got, g_got = _epoch(ds, workers, state, index=True)
        assert len(ref) == len(got) == 6
        for samples, idx in zip(ref, got):
            assert isinstance(idx, np.ndarray) and idx.dtype == np.int64
            assert [ds[int(i)] for i in idx] == samples
        assert torch.equal(g_ref.get_state(), g_got.get_state())     # the next epoch starts from the same state too
    assert sorted(int(i) for idx in got for i in idx) == list(range(len(ds)))


def test_index_view_items_and_the_wrappers_generator():
    from torch.utils.data import DataLoader
    from umpr_amd.reviews import IndexView, PhotoCollate, StoreLoader
    from umpr_amd.train import _shuffle_generator
    import main
    ds, st = tiny("sentence")
    view = IndexView(ds)
    assert len(view) == len(ds) and view[3] == (3, ds.data[3][3])
    g = torch.Generator().manual_seed(0)
    dl = DataLoader(view, batch_size=4, shuffle=True, generator=g, collate_fn=PhotoCollate(True))
    wrapped = main.ShardedLoader(StoreLoader(dl, st), 0, 1)
    assert _shuffle_generator(wrapped) is g and len(wrapped) == 7
    idx, photos = PhotoCollate(True)([view[2], view[0]])
    assert idx.tolist() == [2, 0] and photos is None


def test_photo_half_is_batch_loaders():
    """the worker-side collate packs the photos batch_loader(resize_on_gpu=True) packs, whole and per shard"""
    from umpr_amd.reviews import IndexView, PhotoCollate
    ds, _ = tiny("sentence")
    view = IndexView(ds)
    picks = [4, 0, 9]
    for shard in (None, (0, 2), (1, 2)):
        ref = batch_loader([ds[i] for i in picks], shard=shard, resize_on_gpu=True)[6]
        rank, world = shard if shard else (0, 1)
        idx, raw = PhotoCollate(False, rank, world)([view[i] for i in picks])
        assert idx.tolist() == picks                                  # the GLOBAL batch's indices: its shapes need them all
        assert tuple(raw.shape) == tuple(ref.shape) and torch.equal(raw.data, ref.data)


# ---- the entry point --------------------------------------------------------------------------------------------------------------
def test_review_collate_is_declared_and_exported():
    from conftest import ROOT
    from umpr_amd._lib import SIGNATURES, lib
    assert SIGNATURES["umpr_review_collate"] == ("pplppppppplpiiiiilpppp", "i")
    header = open(os.path.join(ROOT, "include", "umpr_hip.h")).read()
    assert "int umpr_review_collate(const int32_t* tokens, const int64_t* sent_off, long n_sent," in header
    assert hasattr(lib().cdll, "umpr_review_collate")
    assert "reviews.hip" in open(os.path.join(ROOT, "umpr_amd", "csrc", "Makefile")).read()


def test_review_collate_refusals_need_no_gpu():
    """everything refused is refused before any launch, with the cause in the message: pure host work on made-up addresses"""
    from umpr_amd._lib import UmprHipError, lib
    L = lib()
    host_idx = (ctypes.c_int32 * 3)(0, 4, 2)
    base = dict(tokens=64, sent_off=128, n_sent=9, ptr_u=192, sid_u=256, ptr_i=320, sid_i=384, ptr_ui=448, sid_ui=512, ratings=576,
                n_samples=5, idx=ctypes.addressof(host_idx), B=3, S=2, L=8, S_ui=1, L_ui=4, pad=0, ids_pair=640, ids_ui=704,
                labels=768, stream=None)

    def refused(match, **change):
        args = dict(base, **change)
        with pytest.raises(UmprHipError, match=match):
            L.call("umpr_review_collate", *args.values())

    for name in ("tokens", "sent_off", "idx", "ids_pair", "labels", "ratings"):
        refused(f"null {name}", **{name: None})
    for role, names in (("user", ("ptr_u", "sid_u")), ("item", ("ptr_i", "sid_i")), ("ui", ("ptr_ui", "sid_ui"))):
        for name in names:
            refused(f"null table of the {role} role", **{name: None})
    # the ui tables may be null when the role is not in use: the call gets past them to the index check
    refused("outside the 4 samples", ptr_ui=None, sid_ui=None, ids_ui=None, S_ui=0, L_ui=0, n_samples=4)
    for B in (0, -3):
        refused(f"B = {B}", B=B)
    refused("bad shape S = 0", S=0)
    refused("bad shape S = 2, L = 0", L=0)
    refused("bad shape S = 2, L = 257", L=257)
    refused("L_ui = 257", L_ui=257)
    refused("null ids_ui with S_ui = 1, L_ui = 4", ids_ui=None)
    refused("null ids_ui with S_ui = 0, L_ui = 4", ids_ui=None, S_ui=0)
    refused("ids_ui given with S_ui = 0, L_ui = 0", S_ui=0, L_ui=0)
    refused("ids_ui given with S_ui = 1, L_ui = 0", L_ui=0)
    refused("index 1 of the batch is 4, outside the 4 samples", n_samples=4)
    host_idx[2] = -1
    refused("index 2 of the batch is -1, outside the 5 samples")
    refused("not 8-byte aligned", ids_pair=644)
