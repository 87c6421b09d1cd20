"""Photos resized on the GPU (umpr_amd/photos.py, csrc/photos.hip), host half: the packed uint8 buffer a RawPhotos carries holds
everything the kernel needs to reproduce the host form of batch_loader bit for bit.  `kernel_in_numpy` restates
photo_resize_u8_kernel reading nothing but that buffer; no GPU needed."""
import pickle

import numpy as np
import pytest
import torch

from umpr_amd.data import batch_loader, get_image
from umpr_amd.photos import DESC, RawPhotos, decode_for_gpu

LUT = (np.arange(256, dtype=np.float64) / 255.0).astype(np.float32)


def kernel_in_numpy(raw):
    """What umpr_photo_resize_u8 computes from RawPhotos.data alone: float32 [B, V, P, 3, dh, dw]."""
    buf = raw.data.numpy()
    dw, dh = raw.size
    desc = raw.descriptors()
    out = np.zeros((len(desc), 3, dh, dw), dtype=np.float32)
    for k, d in enumerate(desc):
        rows, cols = int(d["rows"]), int(d["cols"])
        if rows == 0:
            continue
        t = buf[d["taps"]:d["taps"] + 16 * (dw + dh)].view(np.int32)
        cx0, cx1, ax0, ax1 = (np.clip(t[i * dw:(i + 1) * dw], 0, cols - 1) if i < 2 else t[i * dw:(i + 1) * dw]
                              for i in range(4))
        ty = t[4 * dw:]
        ry0, ry1, by0, by1 = (np.clip(ty[i * dh:(i + 1) * dh], 0, rows - 1) if i < 2 else ty[i * dh:(i + 1) * dh]
                              for i in range(4))
        pix = buf[d["pixels"]:d["pixels"] + rows * cols * 3].reshape(rows, cols, 3).astype(np.int32)
        h = (pix[:, cx0] * ax0[None, :, None] + pix[:, cx1] * ax1[None, :, None]) >> 4        # [rows][dw][3]
        v = (((by0[:, None, None] * h[ry0]) >> 16) + ((by1[:, None, None] * h[ry1]) >> 16) + 2) >> 2
        out[k] = LUT[np.clip(v, 0, 255)].transpose(2, 0, 1)
    return out.reshape(raw.shape)


def _save(img, path, fmt=None, **kw):
    img.save(path, format=fmt, **kw)
    return str(path)


@pytest.fixture(scope="module")
def photo_set(tmp_path_factory):
    """Paths of the photo set: sizes from 1x1 to 4000x3000, strips, grey / RGBA / palette content, unreadable entries."""
    from PIL import Image
    d = tmp_path_factory.mktemp("photos")
    g = np.random.default_rng(11)

    def rgb(w, h):
        low = g.integers(0, 256, (max(2, h // 40), max(2, w // 40), 3), dtype=np.uint8)
        smooth = np.asarray(Image.fromarray(low).resize((w, h), Image.BICUBIC), dtype=np.int16)
        noise = g.integers(-20, 21, (h, w, 3))
        return Image.fromarray(np.clip(smooth + noise, 0, 255).astype(np.uint8))

    paths = [_save(rgb(w, h), d / f"p{w}x{h}.jpg", quality=90)
             for w, h in ((500, 375), (224, 224), (100, 80), (1, 1), (3000, 40), (40, 3000), (4000, 3000))]
    paths.append(_save(rgb(300, 200).convert("L"), d / "grey.jpg"))
    paths.append(_save(rgb(123, 77).convert("RGBA"), d / "rgba.png"))
    paths.append(_save(rgb(210, 150).convert("P"), d / "palette_as.jpg", fmt="PNG"))   # PNG content behind a .jpg name
    full = open(paths[0], "rb").read()
    trunc = d / "truncated.jpg"
    trunc.write_bytes(full[: len(full) // 2])
    paths += [str(trunc), str(d / "does_not_exist.jpg"), "unknown"]
    return paths


def samples_for(paths, B, V, P, seed=0):
    """B collate samples (user, item, ui sentences, photo paths [V][P], rating) whose photos cycle through `paths`."""
    rnd = np.random.default_rng(seed)
    sents = lambda n: [list(rnd.integers(3, 50, rnd.integers(6, 9))) for _ in range(n)]
    out = []
    for b in range(B):
        ph = [[paths[(b * V * P + v * P + p) % len(paths)] for p in range(P)] for v in range(V)]
        out.append((sents(3), sents(2), sents(2), ph, float(b % 5 + 1)))
    return out


@pytest.mark.parametrize("size", [(160, 120), (224, 224)])
def test_packed_buffer_reproduces_host_photos_bit_for_bit(photo_set, size):
    V, P = 4, 2
    dw, dh = size
    B = -(-len(photo_set) // (V * P))
    samples = samples_for(photo_set, B, V, P)
    gpu = batch_loader(samples, photo_size=size, resize_on_gpu=True)
    raw = gpu[6]
    assert isinstance(raw, RawPhotos) and raw.data.dtype == torch.uint8
    assert tuple(raw.shape) == (B, V, P, 3, dh, dw)
    got = kernel_in_numpy(raw)
    flat = [p for smp in samples for view in smp[3] for p in view]
    missing = [p in photo_set[-3:] for p in flat]                        # truncated, absent, 'unknown'
    assert list(raw.descriptors()["rows"] == 0) == missing
    # photo by photo against get_image (what the host collate stacks)
    for k, (p, miss) in enumerate(zip(flat, missing)):
        want = np.zeros((3, dh, dw), np.float32) if miss else get_image(p, size).astype(np.float32)
        assert np.array_equal(got.reshape(-1, 3, dh, dw)[k], want), p
    if dw == dh:
        # and the host collate itself (a non-square size cannot stack get_image's [3][dw][dh] zeros of a missing photo)
        host = batch_loader(samples, photo_size=size)
        assert tuple(host[6].shape) == tuple(raw.shape)
        assert np.array_equal(got, host[6].numpy())
        for a, b in zip(host[:6] + host[7:], gpu[:6] + gpu[7:]):
            assert torch.equal(a, b)
    else:
        readable = samples_for(photo_set[:-3], B, V, P)
        host = batch_loader(readable, photo_size=size)
        assert np.array_equal(kernel_in_numpy(batch_loader(readable, photo_size=size, resize_on_gpu=True)[6]),
                              host[6].numpy())


@pytest.mark.parametrize("size", [(224, 224), (160, 120)])
def test_upload_bound(photo_set, size):
    """No photo ships more pixel bytes than its float32 form (3*dh*dw*4); full compaction reaches it exactly."""
    dw, dh = size
    for p in photo_set:
        r = decode_for_gpu(p, size)
        if r is None:
            continue
        pix, taps = r
        assert pix.dtype == np.uint8 and pix.shape[2] == 3 and pix.flags.c_contiguous
        assert pix.nbytes <= 3 * dh * dw * 4, (p, pix.shape)
        assert pix.shape[0] <= 2 * dh and pix.shape[1] <= 2 * dw
        assert taps.dtype == np.int32 and taps.shape == (4 * dw + 4 * dh,)
    big = decode_for_gpu(photo_set[6], size)[0]                       # 4000x3000: every other tap a distinct pixel
    assert big.shape == (2 * dh, 2 * dw, 3)


def test_missing_photos_are_none(photo_set):
    for p in photo_set[-3:]:
        assert decode_for_gpu(p) is None


def test_raw_photos_pickle_pin_and_shape(photo_set):
    V, P = 1, 2
    raw = batch_loader(samples_for(photo_set[:4], 3, V, P), resize_on_gpu=True)[6]
    assert raw.shape == torch.Size((3, V, P, 3, 224, 224))
    back = pickle.loads(pickle.dumps(raw))
    assert back.shape == raw.shape and torch.equal(back.data, raw.data)
    assert np.array_equal(kernel_in_numpy(back), kernel_in_numpy(raw))
    if torch.cuda.is_available():          # pinning needs the device runtime
        pinned = raw.pin_memory()
        assert pinned.is_pinned() and pinned.shape == raw.shape and torch.equal(pinned.data, raw.data)
    assert raw.data.numel() >= len(raw.descriptors()) * DESC.itemsize


def test_raw_photos_refuse_the_cpu(photo_set):
    raw = batch_loader(samples_for(photo_set[:2], 1, 1, 1), resize_on_gpu=True)[6]
    with pytest.raises(RuntimeError, match="no CPU path"):
        raw.to("cpu")


@pytest.mark.parametrize("world", [2, 4])
def test_sharded_gpu_form_holds_only_this_ranks_photos(photo_set, world):
    V, P = 2, 1
    samples = samples_for(photo_set, 3, V, P, seed=4)         # 3 samples over 4 ranks: rank 3's chunk is empty
    for rank in range(world):
        host = batch_loader(samples, shard=(rank, world))
        gpu = batch_loader(samples, shard=(rank, world), resize_on_gpu=True)
        raw = gpu[6]
        assert isinstance(raw, RawPhotos)
        assert raw.geometry == (host[0].shape[0], V, P)
        assert len(raw.descriptors()) == host[0].shape[0] * V * P
        if host[0].shape[0]:
            assert np.array_equal(kernel_in_numpy(raw), host[6].numpy())
        else:
            assert raw.shape[0] == 0 and host[6].shape[0] == 0
        for a, b in zip(host[:6] + host[7:], gpu[:6] + gpu[7:]):
            assert torch.equal(a, b)
    if world == 4:
        assert batch_loader(samples, shard=(3, 4), resize_on_gpu=True)[6].geometry == (0, V, P)


def test_main_collate_ships_raw_photos_for_the_full_model(photo_set):
    from main import _Collate
    samples = samples_for(photo_set[:3], 2, 1, 1)
    full = _Collate(False)(samples)
    assert isinstance(full[6], RawPhotos) and full[6].shape == torch.Size((2, 1, 1, 3, 224, 224))
    assert np.array_equal(kernel_in_numpy(full[6]), batch_loader(samples)[6].numpy())
    r_only = _Collate(True)(samples)
    assert isinstance(r_only[6], torch.Tensor) and r_only[6].numel() == 0
    sharded = _Collate(False, rank=1, world=2)(samples)
    assert isinstance(sharded[6], RawPhotos) and sharded[6].geometry == (1, 1, 1) and len(sharded) == 9
