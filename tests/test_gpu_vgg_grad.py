"""VGG16 gradients of the HIP backward against a float64 backward that replays the HIP forward's decisions
(tests/vgg_decisions.py), inside the network: the activation arena, the V-slot reuse of the Winograd weight gradient, the
gradient-slot rotation and the weight-gradient side stream of umpr_vgg16_features_bwd, and the classifier backward.

With the ReLU, max-pool and dropout decisions taken from the arena the backward is linear and smooth, so every parameter
gradient is held to a tight bound - 1e-4 relative L2 and every element within 1e-3 of the tensor's max - instead of the
fp32-vs-fp64 draw of the golden gate (test_gpu_parity.py: _compare_golden).  The same runs check the forward layer by
layer against float64 convolutions of the HIP layer inputs.  Every tensor's distance is logged to vgg_grad.log, beside the
parity tests' log.
"""
import os
import time

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import vgg_decisions as V
from test_gpu_parity import LOG as PARITY_LOG

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "vgg_grad.log")
REL_L2, REL_MAX = 1e-4, 1e-3          # per parameter gradient: relative L2, and max error / max |reference|
F4_MODE = int(os.environ.get("UMPR_WINO_F4", "2"))
# the training forward takes its ReLU / pool decisions at direct accuracy only on the 4x4 tile with the fix-up on
DECISIONS_FIXED = F4_MODE == 2 and os.environ.get("UMPR_WINO_FIX_KAPPA", "8") != "0"


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def _capture(monkeypatch):
    """Every (images, arena) pair _VGGFeatures produces while the test runs."""
    import umpr_amd.model as M
    runs = []
    orig = M._VGGFeatures.apply

    def apply(images, *params):
        pool5, acts = orig(images, *params)
        runs.append((images, acts))
        return pool5, acts

    monkeypatch.setattr(M._VGGFeatures, "apply", apply)
    return runs


def _images(n, seed):
    """random images; with n >= 3 the second-last is constant per channel (a flat photo) and the last all zero (a missing
    photo, src/dataset.py:142-143)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, 224, 224, generator=g)
    if n >= 3:
        x[n - 2] = torch.rand(3, 1, 1, generator=g)
        x[n - 1] = 0
    return x


def _vgg(dev, seed):
    """torchvision's initialisation, plus small random biases (with zero biases a zero image has no gradient at all)"""
    from umpr_amd.model import VGG16
    torch.manual_seed(seed)
    m = VGG16()
    with torch.no_grad():
        for mod in list(m.features) + list(m.classifier):
            if isinstance(mod, (torch.nn.Conv2d, torch.nn.Linear)):
                mod.bias.uniform_(-0.05, 0.05)
    return m.to(dev)


def _forward_check(tag, images, acts, params):
    """Each HIP conv output against relu(conv2d_fp64(HIP input)) at test_conv3x3's bounds, each pool output equal to the
    max of its HIP window, and (test_winograd_forward_decisions_are_taken_at_direct_accuracy's bounds) no ReLU sign or pool
    argmax that differs from the float64 one where the float64 margin is at least 4e-7 of max|y|.  The decision part is
    asserted only where the training forward fixes its decisions up (UMPR_WINO_F4=2, UMPR_WINO_FIX_KAPPA != 0); elsewhere
    the counts are logged."""
    ci, x = 0, images.double().cpu()
    bad, signs, args = [], 0, 0
    for b, blk in enumerate(V.VGG16_BLOCKS):
        for j in range(len(blk)):
            xin = x if ci == 0 else acts["pool"][b - 1] if j == 0 else acts["conv"][ci - 1]
            w, bias = params[2 * ci].detach().double().cpu(), params[2 * ci + 1].detach().double().cpu()
            y64 = F.conv2d(xin, w, bias, padding=1)
            r64, hip = torch.relu(y64), acts["conv"][ci]
            cin, cout, hw = w.shape[1], w.shape[0], y64.shape[-1]
            f4 = F4_MODE >= 2 and ((hw in (56, 28, 14) and cin >= 32) or (hw == 112 and cin >= 128 and cout >= 128))
            scale = float(y64.abs().max())
            tol = 2e-5 + 1e-5 * r64.abs() + (5e-6 * float(r64.abs().max()) if f4 else 0.0)
            err = (hip - r64).abs()
            n_bad = int((err > tol).sum())
            n_sign = int((((hip > 0) != (y64 > 0)) & (y64.abs() >= 4e-7 * scale)).sum())
            msg = f"{tag} fwd conv{ci}: max_err={float(err.max()):.3e} ({float(err.max()) / scale:.2e} of max|y|) bad={n_bad} wrong_sign={n_sign}"
            if j == len(blk) - 1:
                pool = acts["pool"][b]
                n_pool = int((F.max_pool2d(hip, 2, 2) != pool).sum())
                a_hip, _ = V.pool_argmax(hip)
                a64, m64 = V.pool_argmax(r64)
                k, C, H, W = r64.shape
                top2 = r64.reshape(k, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(k, C, H // 2, W // 2, 4).topk(2, -1).values
                clear = ((top2[..., 0] - top2[..., 1]) >= 4e-7 * scale) & (m64 > 0)
                n_arg = int(((a_hip != a64) & clear).sum())
                msg += f" | pool{b}: unequal={n_pool} clear windows={int(clear.sum())} wrong_argmax={n_arg}"
                args += n_arg
                if n_pool:
                    bad.append(f"pool{b}: {n_pool} outputs differ from the max of their HIP window")
            log(msg)
            signs += n_sign
            if n_bad:
                bad.append(f"conv{ci}: {n_bad} outputs off, max err {float(err.max()):.3e}")
            ci += 1
    log(f"{tag} forward decisions: {signs} wrong ReLU signs, {args} wrong pool argmax beyond 4e-7 max|y|"
        + ("" if DECISIONS_FIXED else " (not asserted in this mode)"))
    assert not bad, bad
    if DECISIONS_FIXED:
        assert signs == 0 and args == 0, (signs, args)


def _gate(tag, vgg, images, acts, d_out, masks):
    """Every VGG16 parameter gradient of the HIP backward against the decision-conditioned float64 backward of the chosen
    images (all images whose upstream gradient is nonzero); returns the reference."""
    t0 = time.time()
    ref = V.vgg16_backward(images, acts, [p.detach() for p in vgg.param_list()], d_out, masks)
    log(f"{tag}: fp64 reference backward of {images.shape[0]} images {time.time() - t0:.1f} s")
    outside = []
    for name, p, r in zip(V.VGG16_PARAM_NAMES, vgg.param_list(), ref):
        got = p.grad.detach().double().cpu()
        assert got.shape == r.shape and torch.isfinite(got).all(), name
        rel_l2 = float((got - r).norm() / r.norm())
        rel_max = float((got - r).abs().max() / r.abs().max())
        log(f"{tag} d{name}: rel_l2={rel_l2:.3e} max_err/max={rel_max:.3e} ref_max={float(r.abs().max()):.3e}")
        if not (rel_l2 <= REL_L2 and rel_max <= REL_MAX):       # every tensor is logged before the test fails
            outside.append((name, rel_l2, rel_max))
    assert not outside, outside
    return ref


def _run(tag, vgg, x, d_out, masks, sel, monkeypatch, dev):
    """HIP forward + backward of vgg on x (masks: injected dropout keep-masks or None), the forward check and the gradient
    gate of the images `sel` (d_out is zero on every other image)."""
    from umpr_amd._lib import lib
    runs = _capture(monkeypatch)
    vgg.zero_grad(set_to_none=True)
    vgg.dropout_masks = masks.to(dev) if masks is not None else None
    t0 = time.time()
    out = vgg(x.to(dev))
    torch.cuda.synchronize()
    assert len(runs) == 1
    images, arena = runs[0]
    acts = V.read_arena(arena, x.shape[0], sel, lib())
    out.backward(d_out.to(dev))
    torch.cuda.synchronize()
    log(f"== {tag}: HIP forward + backward of {x.shape[0]} images {time.time() - t0:.1f} s")
    xs = images[list(sel)].double().cpu()
    _forward_check(tag, xs, acts, vgg.param_list())
    ms = masks[:, list(sel)] if masks is not None else None
    return xs, acts, _gate(tag, vgg, xs, acts, d_out[list(sel)], ms)


@pytest.mark.parametrize("train", [False, True], ids=["eval", "train"])
@pytest.mark.parametrize("n", [1, 3, 8])
def test_vgg16_grads_vs_decision_reference(dev, monkeypatch, n, train):
    """Dense upstream gradient on n = 1 / 3 / 8 images (random, constant, all-zero), eval and train with injected dropout
    masks: all 32 parameter gradients against the float64 decision-conditioned backward, 1e-4 relative L2 and 1e-3 of max."""
    t0 = time.time()
    vgg = _vgg(dev, 100 + n)
    vgg.train(train)
    g = torch.Generator().manual_seed(200 + n)
    x = _images(n, 300 + n)
    masks = (torch.rand(2, n, 4096, generator=g) < 0.5).to(torch.uint8) if train else None
    d_out = torch.randn(n, 1000, generator=g)
    _run(f"dense n={n} {'train' if train else 'eval'}", vgg, x, d_out, masks, list(range(n)), monkeypatch, dev)
    log(f"dense n={n} {'train' if train else 'eval'}: test time {time.time() - t0:.1f} s")


def test_vgg16_grads_full_size_sparse_upstream(dev, monkeypatch):
    """64 images (BASELINE.json configs[1] per GPU), train mode with injected masks; the upstream gradient is nonzero only
    on images 0 (random, first of the batch), 33 (constant, across the 32-image boundary) and 63 (all zero, last): every
    HIP kernel runs at full size, and the other 61 images contribute exactly zero, so a three-image float64 reference is
    the reference of the whole batch-64 backward."""
    t0 = time.time()
    n, sel = 64, [0, 33, 63]
    vgg = _vgg(dev, 164).train()
    g = torch.Generator().manual_seed(264)
    x = torch.rand(n, 3, 224, 224, generator=g)
    x[33] = torch.rand(3, 1, 1, generator=g)
    x[63] = 0
    masks = (torch.rand(2, n, 4096, generator=g) < 0.5).to(torch.uint8)
    d_out = torch.zeros(n, 1000)
    d_out[sel] = torch.randn(len(sel), 1000, generator=g)
    _run("sparse n=64", vgg, x, d_out, masks, sel, monkeypatch, dev)
    log(f"sparse n=64: test time {time.time() - t0:.1f} s")


def test_vgg16_grad_gate_catches_one_wrong_pool4_route(dev, monkeypatch):
    """The bound sits far below one wrong routing decision: moving the route of ONE pool4 window (the one whose output
    gradient is largest) to the next element of its window moves every conv1_1..conv4_3 gradient by at least 10x its
    bound in relative L2 - except conv4_3's bias, whose gradient sums the moved value within the same channel.  So a
    pool tie-rule or window off-by-one error fails the gate without any kernel fault."""
    vgg = _vgg(dev, 7).eval()
    g = torch.Generator().manual_seed(8)
    x = _images(1, 9)
    d_out = torch.randn(1, 1000, generator=g)
    xs, acts, ref = _run("sensitivity n=1", vgg, x, d_out, None, [0], monkeypatch, dev)
    params = [p.detach() for p in vgg.param_list()]
    d_pools = {}
    V.vgg16_backward(xs, acts, params, d_out, None, d_pools=d_pools)
    arg, m = V.pool_argmax(acts["conv"][9])
    score = d_pools[3].abs() * (m > 0)
    win = tuple(int(i) for i in torch.nonzero(score == score.max())[0])
    moved = V.vgg16_backward(xs, acts, params, d_out, None, move=(3, win, (int(arg[win]) + 1) % 4))
    margins = []
    for k in range(19):                                     # conv1_1 .. conv4_3 weights and biases, conv4_3's bias excluded
        r = ref[k]
        rel_l2 = float((moved[k] - r).norm() / r.norm())
        rel_max = float((moved[k] - r).abs().max() / r.abs().max())
        log(f"sensitivity d{V.VGG16_PARAM_NAMES[k]}: one moved pool4 route changes it by rel_l2={rel_l2:.3e} "
            f"({rel_l2 / REL_L2:.0f}x the bound), max/max={rel_max:.3e}")
        margins.append((rel_l2 / REL_L2, V.VGG16_PARAM_NAMES[k]))
    log(f"sensitivity: smallest margin {min(margins)[0]:.1f}x ({min(margins)[1]}), window {win}")
    assert min(margins)[0] >= 10, min(margins)


@pytest.mark.parametrize("name", ["umpr_full_V1_B2", "umpr_full_V1_B2_randnM", "umpr_full_V4_B2", "umpr_full_V1_B2_drop",
                                  "umpr_full_V2_P2_B2"])
def test_vgg16_grads_on_golden_fixtures(dev, monkeypatch, name):
    """The five full golden fixtures through UMPR.forward, as test_umpr_full_golden runs them: the arena and images are
    captured around _VGGFeatures, the gradient at the VGG16 output with a tensor hook, and every VGG16 parameter gradient
    is held to the decision-conditioned float64 backward (beside, not instead of, the golden gate)."""
    from test_gpu_parity import _build
    from umpr_amd._lib import lib
    t0 = time.time()
    g, model, batch = _build(name, dev)
    vgg = model.visual_net.vgg16[0]
    masks = None
    if "drop_mask0" in g:
        model.train()
        masks = torch.from_numpy(np.stack([g["drop_mask0"], g["drop_mask1"]]))
        vgg.dropout_masks = masks.to(dev)
    else:
        model.eval()
    runs = _capture(monkeypatch)
    d_outs = []

    def on_output(mod, inp, out):          # returns None: the output itself is left as it is
        out.register_hook(lambda gr: d_outs.append(gr.detach().clone()))

    hook = vgg.register_forward_hook(on_output)
    try:
        pred, loss = model(*batch)
        torch.cuda.synchronize()
        assert len(runs) == 1
        images, arena = runs[0]
        n = images.shape[0]
        acts = V.read_arena(arena, n, range(n), lib())
        loss.backward()
        torch.cuda.synchronize()
    finally:
        hook.remove()
    assert len(d_outs) == 1
    xs = images.double().cpu()
    _forward_check(f"golden {name}", xs, acts, vgg.param_list())
    _gate(f"golden {name}", vgg, xs, acts, d_outs[0].cpu(), masks)
    log(f"golden {name} ({n} images): test time {time.time() - t0:.1f} s")
