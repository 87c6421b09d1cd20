"""Photos resized on the GPU (umpr_photo_resize_u8, csrc/photos.hip) against the host form of the loader: the uploaded float32
photos, a full-model training step, the bf16 eval forward and a worker DataLoader are all bit-identical; malformed buffers
are argument errors."""
import numpy as np
import pytest
import torch

from test_photo_pack import photo_set, samples_for  # noqa: F401  (module fixture)
from umpr_amd.data import batch_loader
from umpr_amd.photos import DESC, RawPhotos

pytestmark = pytest.mark.gpu


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


@pytest.mark.parametrize("B,size", [(2, (224, 224)), (9, (224, 224)), (3, (160, 120))])
def test_raw_photos_to_device_equals_host_form(dev, photo_set, B, size):
    """B = 9 at V = 4, P = 2 is 72 photos: two launches of the kernel (64 descriptors per launch)."""
    V, P = 4, 2
    set_ = photo_set if size[0] == size[1] else photo_set[:-3]     # the host form cannot stack non-square missing photos
    samples = samples_for(set_, B, V, P, seed=B)
    host = batch_loader(samples, photo_size=size)[6]
    raw = batch_loader(samples, photo_size=size, resize_on_gpu=True)[6]
    want = host.to(dev)
    got = raw.to(dev)
    assert got.dtype == torch.float32 and got.shape == want.shape and got.is_contiguous()
    assert torch.equal(got, want)
    pinned = raw.pin_memory()
    assert pinned.is_pinned()
    got2 = pinned.to(dev, non_blocking=True)
    torch.cuda.synchronize()
    assert torch.equal(got2, want)


def _model(cfg, P, dev, seed=5):
    from umpr_amd.model import UMPR
    torch.manual_seed(seed)
    m = UMPR(cfg, P["embedding.weight"].numpy())
    m.load_state_dict(P)
    return m.to(dev)


def test_full_model_train_step_is_identical(dev, photo_set):
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_param_state
    from umpr_amd.train import train_step
    V, Pc = 2, 1
    samples = samples_for(photo_set, 3, V, Pc, seed=21)
    cfg = _cfg(review_net_only=False, views=["food", "inside"], photo_count=Pc)
    P = make_param_state(131, 50, 500, V, False, m_scale=0.05)
    runs = []
    for gpu_form in (False, True):
        batch = batch_loader(samples, resize_on_gpu=gpu_form)
        assert isinstance(batch[6], RawPhotos) == gpu_form
        m = _model(cfg, P, dev)
        opt = FusedAdam(m, 1e-3, 1e-3)
        pred, loss = train_step(m, opt, batch)
        torch.cuda.synchronize()
        runs.append((pred.detach().clone(), loss.detach().clone(), {k: v.detach().clone() for k, v in m.state_dict().items()}))
    assert torch.equal(runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1])
    for k in runs[0][2]:
        assert torch.equal(runs[0][2][k], runs[1][2][k]), k


def test_bf16_eval_forward_is_identical(dev, photo_set):
    from umpr_amd.synthetic import make_param_state
    V, Pc = 1, 2
    samples = samples_for(photo_set, 3, V, Pc, seed=22)
    cfg = _cfg(review_net_only=False, views=["food"], photo_count=Pc, dtype="bf16")
    P = make_param_state(132, 50, 500, V, False, m_scale=0.05)
    m = _model(cfg, P, dev).eval()
    outs = []
    with torch.no_grad():
        for gpu_form in (False, True):
            pred, loss = m(*batch_loader(samples, resize_on_gpu=gpu_form))
            outs.append((pred.clone(), loss.clone()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])


def test_worker_dataloader_feeds_model(dev, photo_set):
    """DataLoader(num_workers=2, pin_memory=True) with main.py's collate: RawPhotos cross the worker boundary, get pinned, and
    the model's eval outputs equal those on the host-form batches."""
    from torch.utils.data import DataLoader
    from main import _Collate
    from umpr_amd.synthetic import make_param_state
    V, Pc = 1, 1
    data = samples_for(photo_set, 8, V, Pc, seed=23)
    cfg = _cfg(review_net_only=False, views=["food"], photo_count=Pc)
    P = make_param_state(133, 50, 500, V, False, m_scale=0.05)
    m = _model(cfg, P, dev).eval()
    dl = DataLoader(data, batch_size=3, collate_fn=_Collate(False), num_workers=2, pin_memory=True)
    n = 0
    with torch.no_grad():
        for k, batch in enumerate(dl):
            assert isinstance(batch[6], RawPhotos) and batch[6].is_pinned()
            host = batch_loader(data[3 * k:3 * k + 3])
            pred, loss = m(*batch)
            rp, rl = m(*host)
            assert torch.equal(pred, rp) and torch.equal(loss, rl)
            n += 1
    assert n == 3


def test_malformed_buffer_is_an_argument_error(dev, photo_set):
    """Descriptors that point outside the buffer (or a buffer too small for its descriptors) fail before any launch."""
    from umpr_amd._lib import UmprHipError
    raw = batch_loader(samples_for(photo_set[:3], 1, 1, 3, seed=24), resize_on_gpu=True)[6]
    assert raw.to(dev).shape == (1, 1, 3, 3, 224, 224)
    nbytes = raw.data.numel()

    def corrupt(field, k, value):
        bad = RawPhotos(raw.data.clone(), raw.geometry, raw.size)
        bad.descriptors()[field][k] = value
        return bad

    cases = [corrupt("pixels", 0, nbytes - 10),                 # pixels run past the end
             corrupt("taps", 1, nbytes - 16),                    # tap tables run past the end
             corrupt("taps", 2, int(raw.descriptors()["taps"][2]) + 2),   # misaligned tables
             corrupt("rows", 0, 0),                              # rows = 0 but cols != 0
             corrupt("cols", 1, -3),
             RawPhotos(raw.data[:-1].clone(), raw.geometry, raw.size),    # buffer one byte short of the last photo
             RawPhotos(raw.data[:2 * DESC.itemsize].clone(), raw.geometry, raw.size)]   # too small for 3 descriptors
    for bad in cases:
        with pytest.raises(UmprHipError):
            bad.to(dev)
    torch.cuda.synchronize()
    assert torch.equal(raw.to(dev), batch_loader(samples_for(photo_set[:3], 1, 1, 3, seed=24))[6].to(dev))
