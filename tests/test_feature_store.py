"""Frozen VGG and the device-resident feature store (umpr_amd/photos.py::FeatureStore, csrc/photos.hip::umpr_feature_fetch_f32),
host half: the plan of which photo reads a slot, which is computed and which computed row fills a slot; the fingerprint that
empties the store; a frozen UMPR and its optimiser built on the CPU; main.py's flag checks; the argument checks of the C entry
point, which refuse before any launch.  No GPU needed."""
import ctypes

import numpy as np
import pytest
import torch

from test_photo_pack import photo_set, samples_for  # noqa: F401  (module fixture)
from umpr_amd.data import batch_loader
from umpr_amd.photos import FeatureTable, PhotoTable, vgg_fingerprint

SIZE = (37, 23)


def gather_in_numpy(fresh, row, src, dst, store):
    """What umpr_feature_fetch_f32 computes and leaves in `store` ([n_slots][F], updated in place)."""
    out = np.where((src >= 0)[:, None], store[np.maximum(src, 0)], fresh[np.maximum(row, 0)] if len(fresh) else 0)
    store[dst[dst >= 0]] = out[dst >= 0]
    return out


def _raw(t, order, V=None):
    V = V or len(order)
    return batch_loader(samples_for(order, 1, V, len(order) // V), photo_size=SIZE, resize_on_gpu=True, store=t.index)[6]


def test_cold_then_warm(photo_set):
    p = photo_set[:4]
    t = FeatureTable(SIZE, 8).register(p)
    assert t.zero_slot == 8 and not t.zero_ready
    raw = _raw(t, p)
    src, dst, row, miss, full = t.plan(raw)
    assert list(src) == [-1] * 4 and list(dst) == [0, 1, 2, 3] and list(row) == [0, 1, 2, 3] and list(miss) == [0, 1, 2, 3]
    assert full == 0 and not t.index.resident.any()                     # nothing is resident before the commit
    assert t.commit(raw, src, dst, row, full) == 4
    assert t.index.resident[:4].tolist() == [1] * 4 and [t.slot_of(q) for q in p] == [0, 1, 2, 3]
    warm = _raw(t, p[::-1])
    assert warm.hits.all() and not (warm.descriptors()["rows"] > 0).any()
    src, dst, row, miss, full = t.plan(warm)
    assert list(src) == [3, 2, 1, 0] and (dst < 0).all() and (row < 0).all() and len(miss) == 0 and full == 0
    t.commit(warm, src, dst, row, full)
    assert t.stats() == dict(slots=8, used=4, hits=4, inserts=4, decoded_while_full=0, unregistered=0, computed=4, shared=0,
                             missing=0, flushes=0, vgg_calls=0)


def test_mixed_batch_and_fresh_row_numbering(photo_set):
    """One batch with a hit, first misses, the same id twice, a photo without an id, and missing photos."""
    p = photo_set
    t = FeatureTable(SIZE, 8).register(p[:4] + [p[11]])                    # p[5] has no id; p[11] does not exist
    first = _raw(t, p[:1])
    t.commit(first, *t.plan(first)[:3])
    order = [p[2], p[0], p[5], p[2], "unknown", p[1], p[5], p[11], p[1]]
    raw = _raw(t, order, V=3)
    assert raw.hits.tolist() == [0, 1, 0, 0, 0, 0, 0, 0, 0] and raw.ids.tolist() == [2, 0, -1, 2, -1, 1, -1, 4, 1]
    src, dst, row, miss, full = t.plan(raw)
    Z = t.zero_slot
    assert list(src) == [-1, 0, -1, -1, Z, -1, -1, Z, -1]
    assert list(row) == [0, -1, 1, 0, -1, 2, 3, -1, 2]                     # p[2] and p[1] share a row; p[5] (no id) never does
    assert list(miss) == [0, 2, 5, 6]                                      # the photos the VGG sees, in batch order
    assert list(dst) == [1, -1, -1, -1, -1, 2, -1, -1, -1] and full == 0   # one slot per new id, at its first occurrence
    assert ((src >= 0) != (row >= 0)).all()
    # what the kernel makes of it
    F = 8
    store = np.full((9, F), np.nan, dtype=np.float32)
    store[0], store[Z] = 100.0, 0.5
    fresh = np.arange(4 * F, dtype=np.float32).reshape(4, F)
    out = gather_in_numpy(fresh, row, src, dst, store)
    assert np.array_equal(out[[0, 3]], fresh[[0, 0]]) and np.array_equal(out[[5, 8]], fresh[[2, 2]])
    assert (out[1] == 100.0).all() and (out[[4, 7]] == 0.5).all() and np.array_equal(out[[2, 6]], fresh[[1, 3]])
    assert np.array_equal(store[1], fresh[0]) and np.array_equal(store[2], fresh[2]) and np.isnan(store[3:8]).all()
    t.commit(raw, src, dst, row, full)
    s = t.stats()
    assert (s["used"], s["inserts"], s["hits"], s["computed"], s["shared"], s["missing"]) == (3, 3, 1, 1 + 4, 2, 2)
    assert t.index.resident[:5].tolist() == [1, 1, 1, 0, 0]
    # a batch decoded by a worker whose view lagged arrives with pixels: it reads the slot all the same
    src, dst, row, miss, full = t.plan(raw)
    assert list(src) == [1, 0, -1, 1, Z, 2, -1, Z, 2] and list(miss) == [2, 6] and list(row) == [-1, -1, 0, -1, -1, -1, 1, -1, -1]
    assert (dst < 0).all()


def test_capacity_exhausted(photo_set):
    p = photo_set[:3]
    t = FeatureTable(SIZE, 1).register(p)
    for k in range(3):
        raw = _raw(t, p + [p[2]])
        src, dst, row, miss, full = t.plan(raw)
        if k == 0:
            assert list(dst) == [0, -1, -1, -1] and list(row) == [0, 1, 2, 2] and list(miss) == [0, 1, 2] and full == 2
        else:
            assert raw.hits.tolist() == [1, 0, 0, 0] and list(src) == [0, -1, -1, -1] and (dst < 0).all()
            assert list(row) == [-1, 0, 1, 1] and list(miss) == [1, 2] and full == 2
        t.commit(raw, src, dst, row, full)
    s = t.stats()
    assert (s["slots"], s["used"], s["inserts"], s["hits"], s["decoded_while_full"], s["computed"], s["shared"]) == (1, 1, 1, 2, 6, 7, 3)


def test_table_empties_when_the_fingerprint_changes(photo_set):
    from umpr_amd._lib import UmprHipError
    p = photo_set[:3]
    t = FeatureTable(SIZE, 4).register(p)
    assert not t.guard(("a",))                                             # the first fingerprint: nothing to empty
    raw = _raw(t, p)
    t.commit(raw, *t.plan(raw)[:3])
    t.zero_ready = True
    assert not t.guard(("a",)) and t.used == 3
    warm = _raw(t, p)
    assert warm.hits.all()
    assert t.guard(("b",))
    assert t.used == 0 and not t.zero_ready and not t.index.resident.any() and [t.slot_of(q) for q in p] == [-1] * 3
    assert t.stats()["flushes"] == 1 and t.stats()["inserts"] == 3
    with pytest.raises(UmprHipError, match="left to the store, which does not hold it"):
        t.plan(warm)                                                       # collated before the store was emptied
    again = _raw(t, p)
    assert not again.hits.any() and list(t.plan(again)[1]) == [0, 1, 2]
    assert not t.guard(("b",))


def test_plan_refuses_other_sizes_and_batches_without_ids(photo_set):
    from umpr_amd._lib import UmprHipError
    t = FeatureTable(SIZE, 4).register(photo_set[:2])
    other = PhotoTable((224, 224)).register(photo_set[:2])
    with pytest.raises(UmprHipError, match="feature store holds"):
        t.plan(batch_loader(samples_for(photo_set[:2], 1, 1, 2), resize_on_gpu=True, store=other.index)[6])
    with pytest.raises(UmprHipError, match="no ids"):
        t.plan(batch_loader(samples_for(photo_set[:2], 1, 1, 2), photo_size=SIZE, resize_on_gpu=True)[6])


def test_fingerprint_follows_the_parameters():
    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.a, self.b = torch.nn.Linear(4, 3), torch.nn.Linear(3, 2)
            self.compute_dtype = "fp32"

    m = Tiny().requires_grad_(False)
    f0 = vgg_fingerprint(m)
    assert vgg_fingerprint(m) == f0
    m.load_state_dict({k: v + 1 for k, v in m.state_dict().items()})
    f1 = vgg_fingerprint(m)
    assert f1 != f0
    m.load_state_dict(m.state_dict())                                      # the same values again: still a reload
    f2 = vgg_fingerprint(m)
    assert f2 != f1
    m.to(torch.float64)
    f3 = vgg_fingerprint(m)
    assert f3 != f2
    m.compute_dtype = "bf16"
    assert vgg_fingerprint(m) != f3


# ---- a frozen UMPR on the CPU --------------------------------------------------------------------------------------------------
def _cfg(**kw):
    from umpr_amd.config import Config
    cfg = Config(argv=[])
    cfg.device = torch.device("cpu")
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


@pytest.fixture(scope="module")
def frozen():
    from umpr_amd.model import UMPR
    torch.manual_seed(3)
    return UMPR(_cfg(review_net_only=False, views=["food", "inside"], freeze_vgg=True), np.zeros((40, 50), dtype=np.float32))


def test_frozen_model_parameters(frozen):
    from umpr_amd.synthetic import make_param_state
    assert frozen.freeze_vgg and frozen.visual_net.vgg16[0].frozen
    named = dict(frozen.named_parameters())
    vgg = [k for k in named if k.startswith("visual_net.vgg16.")]
    assert len(vgg) == 32 and not any(named[k].requires_grad for k in vgg)
    rest = [k for k in named if k not in vgg and k != "embedding.weight"]      # (the GloVe table never trains)
    assert all(named[k].requires_grad for k in rest)
    assert {"visual_net.pos_v_emb", "visual_net.neg_v_emb", "visual_net.linear.weight", "visual_net.linear.bias"} <= set(rest)
    # the reference's keys and shapes, as the unfrozen model has them (tests/test_gpu_parity.py pins those to make_param_state)
    want = make_param_state(1, 50, 40, 2, False, with_vgg=False)
    have = {k: tuple(v.shape) for k, v in frozen.state_dict().items()}
    assert {k: have[k] for k in have if ".vgg16." not in k} == {k: tuple(v.shape) for k, v in want.items() if ".vgg16." not in k}
    from umpr_amd.model import VGG16
    meta = {}
    with torch.device("meta"):
        meta = {"visual_net.vgg16.0." + k: tuple(v.shape) for k, v in VGG16().state_dict().items()}
    assert {k: have[k] for k in have if ".vgg16." in k} == meta


def test_flag_is_off_by_default_and_ignored_without_a_visual_net():
    from umpr_amd.model import UMPR
    emb = np.zeros((40, 50), dtype=np.float32)
    r = UMPR(_cfg(review_net_only=True, freeze_vgg=True), emb)
    assert r.freeze_vgg is False and all(p.requires_grad for n, p in r.named_parameters() if n != "embedding.weight")
    assert UMPR(_cfg(review_net_only=True), emb).freeze_vgg is False


def test_fused_adam_on_a_frozen_model(frozen):
    from umpr_amd.optim import FusedAdam
    from umpr_amd.parallel import GradReducer
    vgg = frozen.visual_net.vgg16[0]
    before = [p.data_ptr() for p in vgg.parameters()]
    opt = FusedAdam(frozen, 1e-3, 1e-3, max_grad_norm=0.0)
    names = [n for g in opt.groups for n in g.names]
    assert names and not any(".vgg16." in n for n in names)
    assert set(names) == {n for n, p in frozen.named_parameters() if p.requires_grad}
    assert sum(g.numel for g in opt.groups) < 1 << 20                       # the text path and the head: no 138 M floats of VGG
    assert [p.data_ptr() for p in vgg.parameters()] == before and all(p.grad is None for p in vgg.parameters())
    # the pieces built around the classifier slice are inert
    assert opt.early_bucket() is None and vgg.grad_callbacks == []
    opt.arm_early(1.0)
    assert opt._early is None
    opt._on_classifier_grads()
    opt.early_step(())
    assert opt._early_done is None
    red = GradReducer(opt)
    assert red.early is None and red.block_slices == {} and red._find_block_slices() == {} and red.hooks == []
    assert not hasattr(next(vgg.parameters()), "_umpr_block_hook")
    # Adam moments only for what trains; a state written with the VGG trainable is refused, and names the flag
    st = opt.state_dict()
    assert set(st["m"]) == set(names) == set(st["v"])
    opt.check_state_dict(st)
    st["m"]["visual_net.vgg16.0.features.0.weight"] = torch.zeros(64 * 27)
    with pytest.raises(ValueError, match="written with the VGG trainable, this run has it frozen"):
        opt.load_state_dict(st)
    clipped = FusedAdam(frozen, 1e-3, 1e-3, max_grad_norm=1.0)              # clipping: the arenas it will reduce over
    assert sum(a.numel() for a in clipped.grad_arenas()) == sum(g.numel for g in clipped.groups)


def test_resume_with_other_optimizer_state_changes_nothing(tmp_path):
    from umpr_amd.checkpoint import load_checkpoint, save_checkpoint
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    emb = np.zeros((40, 50), dtype=np.float32)
    a, b = UMPR(_cfg(review_net_only=True), emb), UMPR(_cfg(review_net_only=True), emb)
    oa, ob = FusedAdam(a, 1e-3, 1e-3), FusedAdam(b, 1e-3, 1e-3)
    save_checkpoint(str(tmp_path / "ok.pt"), a, oa)
    ck = torch.load(str(tmp_path / "ok.pt"), weights_only=True)
    del ck["optimizer"]["m"]["linear_fusion.0.bias"]                         # as if that parameter had been frozen
    torch.save(ck, str(tmp_path / "bad.pt"))
    kept = {k: v.clone() for k, v in b.state_dict().items()}
    with pytest.raises(ValueError, match="optimizer state does not match the trainable parameters"):
        load_checkpoint(str(tmp_path / "bad.pt"), b, ob)
    assert all(torch.equal(v, kept[k]) for k, v in b.state_dict().items()) and ob.step_count == 0
    seen = vgg_fingerprint(b.review_net)                                    # (any module: the fingerprint reads parameters)
    load_checkpoint(str(tmp_path / "ok.pt"), b, ob)
    assert vgg_fingerprint(b.review_net) != seen                            # a store filled before the load would empty itself
    assert all(torch.equal(v, a.state_dict()[k]) for k, v in b.state_dict().items())


# ---- main.py --------------------------------------------------------------------------------------------------------------------
@pytest.fixture
def main_config():
    import main
    from umpr_amd.config import Config
    saved = Config._extra
    Config.extend(main.EXTRA_OPTIONS)
    yield lambda *argv: Config(argv=list(argv))
    Config._extra = saved


def test_main_flags(main_config):
    import main
    cfg = main_config()
    assert cfg.freeze_vgg is False and cfg.feature_store_gb == 0.0
    main.check_flags(cfg)
    cfg = main_config("--freeze_vgg", "True", "--feature_store_gb", "0.5")
    assert cfg.freeze_vgg is True and cfg.feature_store_gb == 0.5
    main.check_flags(cfg)
    main.check_flags(main_config("--freeze_vgg", "True"))
    main.check_flags(main_config("--freeze_vgg", "True", "--review_net_only", "True"))
    with pytest.raises(SystemExit, match="--feature_store_gb needs --freeze_vgg True"):
        main.check_flags(main_config("--feature_store_gb", "1"))
    with pytest.raises(SystemExit, match="--feature_store_gb needs --freeze_vgg True"):
        main.check_flags(main_config("--feature_store_gb", "1", "--photo_store_gb", "1"))
    with pytest.raises(SystemExit, match="must be >= 0"):
        main.check_flags(main_config("--freeze_vgg", "True", "--feature_store_gb", "-1"))
    with pytest.raises(SystemExit, match="takes True or False"):
        main.check_flags(main_config("--freeze_vgg", "1"))


# ---- the C entry point's argument checks (they run on the host, before any launch) ------------------------------------------
def test_feature_fetch_refuses_bad_arguments_without_a_gpu():
    from umpr_amd._lib import lib
    L = lib()
    fn = L.fn["umpr_feature_fetch_f32"]
    FRESH, STORE, OUT = 0x10000, 0x20000, 0x30000                          # never dereferenced: every call below is refused

    def rc(row, src, dst, n_fresh=2, F=1000, n_slots=4, fresh=FRESH, store=STORE, out=OUT, n=None):
        a = [np.asarray(x, dtype=np.int32) for x in (row, src, dst)]
        return fn(fresh, n_fresh, a[0].ctypes.data, a[1].ctypes.data, a[2].ctypes.data, len(a[0]) if n is None else n, F, store,
                  n_slots, out, None), L.last_error()

    cases = {"src_slot 4 outside": rc([-1], [4], [-1]),
             "dst_slot 4 outside": rc([0], [-1], [4]),
             "both a src_slot and a fresh_row": rc([0], [1], [-1]),
             "neither a src_slot and a fresh_row": rc([-1], [-1], [-1]),
             "fresh_row 2 outside": rc([2], [-1], [-1]),
             "dst_slot of two photos": rc([0, 1], [-1, -1], [3, 3]),
             "which this call writes": rc([0, -1], [-1, 3], [3, -1]),
             "not a positive multiple of 4": rc([0], [-1], [-1], F=1001),
             "not 16-byte aligned": rc([0], [-1], [-1], out=OUT + 4),
             "store is null": rc([-1], [1], [-1], store=None),
             "null `fresh`": rc([0], [-1], [-1], fresh=None),
             "n = -1": rc([0], [-1], [-1], n=-1)}
    for text, (code, err) in cases.items():
        assert code == -1 and text in err, (text, code, err)
    assert rc([-1], [-1], [-1], F=2)[1].count("multiple of 4") == 1
    assert rc([0], [-1], [-1], fresh=FRESH + 8)[0] == -1 and rc([-1], [0], [-1], store=STORE + 8)[0] == -1
    assert rc([], [], [], n=0)[0] == 0                                      # nothing to do is no error
    assert ctypes.sizeof(ctypes.c_int32) == 4
