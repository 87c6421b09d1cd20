"""bench.py --dump-outputs on CPU with a stand-in model: one float32 .npy per output, parameter and gradient; tensors above
DUMP_SAMPLE elements are stored as the same seeded sample on every run, so two builds compare file for file."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def test_dump_outputs_writes_float32_arrays_and_a_fixed_sample(tmp_path):
    import bench
    torch.manual_seed(0)
    model = torch.nn.Sequential(torch.nn.Linear(300, 300), torch.nn.Linear(300, 1))
    x = torch.randn(5, 300)
    pred = model(x).squeeze(1)
    loss = (pred ** 2).mean()
    loss.backward()
    a, b = tmp_path / "a", tmp_path / "b"
    bench.dump_outputs(str(a), model, pred, loss, with_grads=True)
    bench.dump_outputs(str(b), model, pred, loss, with_grads=True)

    names = sorted(f[:-4] for f in os.listdir(a))
    want = ["loss", "pred"] + [p + n for n, _ in model.named_parameters() for p in ("grad.", "param.")]
    assert names == sorted(want)
    for n in names:
        x_a, x_b = np.load(a / (n + ".npy")), np.load(b / (n + ".npy"))
        assert x_a.dtype == np.float32 and np.array_equal(x_a, x_b), n
    np.testing.assert_array_equal(np.load(a / "pred.npy"), pred.detach().numpy())
    assert np.load(a / "loss.npy").shape == () and float(np.load(a / "loss.npy")) == float(loss.detach())
    np.testing.assert_array_equal(np.load(a / "param.1.weight.npy"), model[1].weight.detach().numpy())

    big = model[0].weight                      # 90 000 elements > DUMP_SAMPLE: a sample at fixed flat indices
    assert big.numel() > bench.DUMP_SAMPLE
    idx = np.unique(np.random.default_rng(0).integers(0, big.numel(), bench.DUMP_SAMPLE))
    np.testing.assert_array_equal(np.load(a / "param.0.weight.npy"), big.detach().reshape(-1).numpy()[idx])
    np.testing.assert_array_equal(np.load(a / "grad.0.weight.npy"), big.grad.reshape(-1).numpy()[idx])


def test_dump_outputs_without_gradients(tmp_path):
    import bench
    model = torch.nn.Linear(3, 1)
    with torch.no_grad():
        pred = model(torch.ones(2, 3)).squeeze(1)
    bench.dump_outputs(str(tmp_path), model, pred, pred.sum(), with_grads=False)
    assert sorted(os.listdir(tmp_path)) == ["loss.npy", "param.bias.npy", "param.weight.npy", "pred.npy"]
