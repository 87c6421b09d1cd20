"""Photo augmentation at the fetch (photos.PhotoAugment, main.py --photo_flip / --photo_crop), host half: the definition, the tap
tables the kernel reads, the counter-based draws, the options and their refusals, and the module in the model and its checkpoint.
No GPU needed."""
import numpy as np
import pytest
import torch

from photo_augment_reference import augment_u8
from umpr_amd.data import _column_taps, _row_taps
from umpr_amd.photos import PhotoAugment, tap_tables

EMB = np.random.default_rng(0).standard_normal((30, 6)).astype(np.float32)


@pytest.fixture
def main_config():
    import main
    from umpr_amd.config import Config
    saved = Config._extra
    Config.extend(main.EXTRA_OPTIONS)
    yield lambda *argv: Config(argv=list(argv))
    Config._extra = saved


# ---- the definition and the tables ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dw,dh", [(224, 224), (7, 5), (32, 33)])
def test_the_whole_window_is_the_identity(dw, dh):
    U = np.random.default_rng(dw).integers(0, 256, (dh, dw, 3), dtype=np.uint8)
    assert np.array_equal(augment_u8(U, (0, 0, dw, dh, 0)), U)
    assert np.array_equal(augment_u8(U, (0, 0, dw, dh, 1)), U[:, ::-1])


@pytest.mark.parametrize("d", [224, 33, 5])
def test_tables_hold_the_host_taps_of_every_source_size(d):
    xt, yt = tap_tables((d, d + 1))
    assert xt.shape == (d, 4 * d) and yt.shape == (d + 1, 4 * (d + 1)) and xt.dtype == yt.dtype == np.int32
    for table, taps, dst in ((xt, _column_taps, d), (yt, _row_taps, d + 1)):
        for s in range(1, dst + 1):
            i0, i1, w0, w1 = taps(dst, s)
            assert np.array_equal(table[s - 1], np.concatenate([i0, i1, w0, w1])), s
            # what the kernel relies on: indices inside the source, 11-bit weights that sum to one
            assert i0.min() >= 0 and i1.min() >= 0 and i0.max() <= s - 1 and i1.max() <= s - 1
            assert w0.min() >= 0 and w1.min() >= 0 and np.array_equal(w0 + w1, np.full(dst, 2048))


# ---- the draws ------------------------------------------------------------------------------------------------------------------
def test_draw_is_a_pure_function_of_seed_call_and_index():
    aug = PhotoAugment(flip=True, min_area=0.3)
    torch.manual_seed(5)
    a = aug.draw(1, 64)
    assert a.shape == (64, 5) and a.dtype == np.int32
    assert np.array_equal(aug.draw(1, 64), a)
    assert np.array_equal(PhotoAugment(flip=True, min_area=0.3).draw(1, 64), a)        # no state in the module
    assert np.array_equal(aug.draw(1, 3), a[:3])                                       # a photo's draw is its index's, not the batch's
    assert not np.array_equal(aug.draw(2, 64), a)
    torch.manual_seed(6)
    assert not np.array_equal(aug.draw(1, 64), a)
    torch.manual_seed(5)
    assert np.array_equal(aug.draw(1, 64), a)
    assert aug._calls == 0                                                             # only an augmented fetch counts


def test_draw_leaves_the_global_generators_alone():
    torch.manual_seed(9)
    np.random.seed(9)
    t, (_, keys, pos, *_rest) = torch.get_rng_state(), np.random.get_state()
    PhotoAugment(flip=True, min_area=0.08).draw(3, 4096)
    assert torch.equal(torch.get_rng_state(), t)
    after = np.random.get_state()
    assert np.array_equal(after[1], keys) and after[2] == pos


@pytest.mark.parametrize("size", [(224, 224), (37, 23), (8, 40)])
@pytest.mark.parametrize("min_area", [0.08, 0.3, 0.9])
def test_windows_fit_and_keep_their_share_and_shape(size, min_area):
    dw, dh = size
    torch.manual_seed(1)
    x0, y0, cw, ch, flip = PhotoAugment(flip=False, min_area=min_area, size=size).draw(7, 2048).T.astype(np.int64)
    assert (cw >= 1).all() and (x0 >= 0).all() and (x0 + cw <= dw).all()
    assert (ch >= 1).all() and (y0 >= 0).all() and (y0 + ch <= dh).all()
    assert not flip.any()
    if 3 / 4 <= dw / dh <= 4 / 3:
        # each side was rounded to a whole pixel: it moved by at most a half
        assert ((cw + 0.5) * (ch + 0.5) >= min_area * dh * dw).all()
        assert ((cw - 0.5) * (ch - 0.5) <= dh * dw).all()
        assert ((cw + 0.5) / (ch - 0.5) >= 3 / 4).all() and ((cw - 0.5) / (ch + 0.5) <= 4 / 3).all()
        assert len(np.unique(x0)) > 1 and len(np.unique(cw)) > 1
    else:
        # an image outside the ratios: a try that fits has its own numbers, the rest are the largest centred window inside them
        fw, fh = (dw, int(np.rint(dw / (3 / 4)))) if dw / dh < 3 / 4 else (int(np.rint(dh * (4 / 3))), dh)
        centred = (x0 == (dw - fw) // 2) & (y0 == (dh - fh) // 2) & (cw == fw) & (ch == fh)
        fits = ((cw + 0.5) / (ch - 0.5) >= 3 / 4) & ((cw - 0.5) / (ch + 0.5) <= 4 / 3)
        assert (centred | fits).all()
        if size == (8, 40) and min_area == 0.9:
            # area >= 288 and ratio >= 3/4 give a width of at least sqrt(216) = 14.7 > 8: no try can fit
            assert centred.all()


def test_offsets_reach_both_edges():
    torch.manual_seed(2)
    x0, y0, cw, ch, _ = PhotoAugment(min_area=0.3).draw(1, 4096).T
    assert (x0 == 0).any() and (x0 + cw == 224).any() and (y0 == 0).any() and (y0 + ch == 224).any()


def test_no_crop_is_the_whole_image_and_the_coin_is_fair():
    torch.manual_seed(3)
    rec = PhotoAugment(flip=True, min_area=1.0).draw(1, 4096)
    assert (rec[:, :4] == (0, 0, 224, 224)).all()
    assert set(np.unique(rec[:, 4])) == {0, 1}
    assert 1856 <= int(rec[:, 4].sum()) <= 2240              # 2048 +- 6 sigma (sigma = 32): a fixed sequence, not a measurement
    assert not PhotoAugment(flip=False, min_area=1.0).draw(1, 64)[:, 4].any()
    for bad in (0.0, 1.5, -1):
        with pytest.raises(ValueError, match="min_area"):
            PhotoAugment(min_area=bad)


# ---- the options ----------------------------------------------------------------------------------------------------------------
def test_flags(main_config):
    import main
    cfg = main_config()
    assert cfg.photo_flip is False and cfg.photo_crop == 1.0
    assert main.EXTRA_OPTIONS["photo_flip"] is False and main.EXTRA_OPTIONS["photo_crop"] == 1.0
    main.check_flags(cfg)
    for ok in (("--photo_flip", "True"), ("--photo_crop", "0.08"), ("--photo_crop", "1"),
               ("--photo_flip", "True", "--photo_crop", "0.3", "--photo_store_gb", "1", "--dtype", "bf16", "--accum_steps", "4",
                "--review_store", "True", "--loader_workers", "2"),
               ("--photo_flip", "True", "--freeze_conv", "True"), ("--photo_crop", "0.5", "--freeze_vgg", "True"),
               # UMPR-R has no photos: accepted and ignored, like the freeze options
               ("--photo_flip", "True", "--photo_crop", "0.5", "--review_net_only", "True", "--data_dir", "synthetic"),
               ("--photo_flip", "True", "--review_net_only", "True", "--freeze_vgg", "True", "--feature_store_gb", "1")):
        main.check_flags(main_config(*ok))
    refused = {("--photo_flip", "1"): "--photo_flip takes True or False",
               ("--photo_crop", "True"): "--photo_crop takes the smallest share",
               ("--photo_crop", "0.05"): "--photo_crop takes the smallest share",
               ("--photo_crop", "1.5"): "--photo_crop takes the smallest share",
               ("--photo_crop", "'0.5'"): "--photo_crop takes the smallest share",
               ("--photo_flip", "True", "--freeze_vgg", "True", "--feature_store_gb", "1"): "--feature_store_gb > 0 exclude each other",
               ("--photo_crop", "0.5", "--freeze_conv", "True", "--pool5_store_gb", "1"): "--pool5_store_gb > 0 exclude each other",
               ("--photo_flip", "True", "--data_dir", "synthetic"): "need decoded photos",
               ("--photo_crop", "0.5", "--data_dir", "synthetic"): "need decoded photos"}
    for argv, text in refused.items():
        with pytest.raises(SystemExit, match=text):
            main.check_flags(main_config(*argv))


# ---- the model ------------------------------------------------------------------------------------------------------------------
class _SmallVGG(torch.nn.Module):
    """Stands in for the 138 M parameter stack: these tests read module names, counters and state_dict keys only."""

    def __init__(self, num_classes=1000, dtype="fp32"):
        super().__init__()
        self.fc = torch.nn.Linear(2, 2)
        self._calls = 0
        self.frozen = self.frozen_conv = False


def _umpr(monkeypatch, main_config, *argv):
    from umpr_amd import model
    monkeypatch.setattr(model, "VGG16", _SmallVGG)
    return model.UMPR(main_config("--views", "food,inside", *argv), EMB)


def test_module_is_registered_only_when_an_option_is_on(monkeypatch, main_config):
    off = _umpr(monkeypatch, main_config)
    assert off.photo_augment is None and "photo_augment" not in dict(off.named_modules())
    for argv, flip, area in ((("--photo_flip", "True"), True, 1.0), (("--photo_crop", "0.3"), False, 0.3),
                             (("--photo_flip", "True", "--photo_crop", "0.5"), True, 0.5)):
        on = _umpr(monkeypatch, main_config, *argv)
        aug = on.photo_augment
        assert isinstance(aug, PhotoAugment) and dict(on.named_modules())["photo_augment"] is aug
        assert (aug.flip, aug.min_area, aug.size, aug._calls) == (flip, area, (224, 224), 0)
        assert not list(aug.parameters()) and not list(aug.buffers())
        assert list(on.state_dict()) == list(off.state_dict())
    r = _umpr(monkeypatch, main_config, "--photo_flip", "True", "--photo_crop", "0.3", "--review_net_only", "True")
    assert r.photo_augment is None


def test_counter_travels_in_a_checkpoint(monkeypatch, main_config, tmp_path):
    from umpr_amd.checkpoint import load_checkpoint, save_checkpoint
    m = _umpr(monkeypatch, main_config, "--photo_flip", "True", "--photo_crop", "0.3")
    m.photo_augment._calls = 41
    m.visual_net.vgg16[0]._calls = 7
    path = str(tmp_path / "ck.pt")
    save_checkpoint(path, m)
    ck = torch.load(path, weights_only=True)
    assert ck["rng_calls"] == {"photo_augment": 41, "visual_net.vgg16.0": 7}
    fresh = _umpr(monkeypatch, main_config, "--photo_flip", "True", "--photo_crop", "0.3")
    assert fresh.photo_augment._calls == 0
    load_checkpoint(path, fresh)
    assert fresh.photo_augment._calls == 41 and fresh.visual_net.vgg16[0]._calls == 7
    plain = _umpr(monkeypatch, main_config)                     # the checkpoint of an augmented run loads into a plain model
    load_checkpoint(path, plain)
    assert plain.photo_augment is None

