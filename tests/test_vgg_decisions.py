"""CPU tests of the decision-conditioned VGG backward reference (tests/vgg_decisions.py) that the GPU gradient gates of
tests/test_gpu_vgg_grad.py compare the HIP backward with.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import vgg_decisions as V

# the VGG16-D block structure at reduced width and map size: 32x32 images -> a 1x1 pool5, a small classifier
BLOCKS = ((4, 4), (8, 8), (8, 8, 8), (16, 16, 16), (16, 16, 16))
HIDDEN, CLASSES = 24, 10


def _params(seed):
    g = torch.Generator().manual_seed(seed)
    ps, cin = [], 3
    for blk in BLOCKS:
        for c in blk:
            ps += [torch.randn(c, cin, 3, 3, generator=g, dtype=torch.float64) * (2.0 / (9 * c)) ** 0.5,
                   (torch.rand(c, generator=g, dtype=torch.float64) - 0.3) * 0.1]
            cin = c
    for fin, fout in ((cin, HIDDEN), (HIDDEN, HIDDEN), (HIDDEN, CLASSES)):
        ps += [torch.randn(fout, fin, generator=g, dtype=torch.float64) / fin ** 0.5,
               (torch.rand(fout, generator=g, dtype=torch.float64) - 0.3) * 0.1]
    return [p.requires_grad_(True) for p in ps]


def _images(seed, n):
    """random images, then a constant image (a flat photo) and an all-zero one (a missing photo)"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, 32, 32, generator=g, dtype=torch.float64)
    x[n - 2] = torch.rand(3, 1, 1, generator=g, dtype=torch.float64)
    x[n - 1] = 0
    return x


def _forward(x, ps, masks):
    """fp64 autograd forward of the reduced network; returns (output, activations in read_arena's format)"""
    acts = {"conv": [], "pool": [], "fc": [], "drop": []}
    h, ci = x, 0
    for blk in BLOCKS:
        for _ in blk:
            h = F.relu(F.conv2d(h, ps[2 * ci], ps[2 * ci + 1], padding=1))
            acts["conv"].append(h)
            ci += 1
        h = F.max_pool2d(h, 2, 2)
        acts["pool"].append(h)
    h = h.flatten(1)
    for j in range(3):
        h = F.linear(h, ps[26 + 2 * j], ps[27 + 2 * j])
        if j < 2:
            h = F.relu(h)
            acts["fc"].append(h)
            if masks is not None:
                h = h * masks[j] / 0.5
            acts["drop"].append(h)
    return h, {k: [t.detach() for t in v] for k, v in acts.items()}


@pytest.mark.parametrize("dropout", [False, True])
def test_reference_backward_equals_autograd(dropout):
    """The helper's backward, with the decisions read from the network's own fp64 activations, equals torch autograd of
    that network to 1e-12 of each tensor's max - every parameter, eval and dropout, ties and all-zero windows included."""
    n = 5
    x = _images(11, n)
    ps = _params(12)
    g = torch.Generator().manual_seed(13)
    masks = (torch.rand(2, n, HIDDEN, generator=g) < 0.5).double() if dropout else None
    out, acts = _forward(x, ps, masks)
    d_out = torch.randn(out.shape, generator=g, dtype=torch.float64)
    out.backward(d_out)
    # the routing rule is exercised: exact ties at a positive maximum (constant image) and all-zero windows (zero image)
    ties = zero = 0
    for ci in (1, 3, 6, 9, 12):
        y = acts["conv"][ci]
        win = y.reshape(n, y.shape[1], y.shape[2] // 2, 2, y.shape[3] // 2, 2).permute(0, 1, 2, 4, 3, 5).flatten(-2)
        top2 = win.topk(2, -1).values
        ties += int(((top2[..., 0] == top2[..., 1]) & (top2[..., 0] > 0)).sum())
        zero += int((top2[..., 0] == 0).sum())
    assert ties > 0 and zero > 0, (ties, zero)
    cls, d_pool5 = V.classifier_backward(acts["pool"][4].flatten(1), acts["fc"], acts["drop"], ps[26:], d_out, masks)
    feats = V.features_backward(x, acts["conv"], acts["pool"], ps[:26], d_pool5.reshape(acts["pool"][4].shape),
                                [len(b) for b in BLOCKS])
    for k, (got, p) in enumerate(zip(feats + cls, ps)):
        ref = p.grad
        scale = float(ref.abs().max())
        assert scale > 0, k
        err = float((got - ref).abs().max())
        assert err <= 1e-12 * scale, (k, err, scale)


def test_moved_route_changes_the_gradient():
    """Re-routing one pool window (the sensitivity hook of the GPU gates) changes every gradient below that pool and none
    above it - except the bias of the conv feeding the pool: its gradient sums the moved value over the same channel."""
    n = 3
    x = _images(21, n)
    ps = _params(22)
    out, acts = _forward(x, ps, None)
    d_out = torch.randn(out.shape, generator=torch.Generator().manual_seed(23), dtype=torch.float64)
    cls, d_pool5 = V.classifier_backward(acts["pool"][4].flatten(1), acts["fc"], acts["drop"], ps[26:], d_out)
    args = [x, acts["conv"], acts["pool"], ps[:26], d_pool5.reshape(acts["pool"][4].shape), [len(b) for b in BLOCKS]]
    base = V.features_backward(*args)
    # the block-4 window of image 0 with the largest maximum, moved to the next element of the window
    arg, m = V.pool_argmax(acts["conv"][9])
    c, yo, xo = [int(i) for i in torch.nonzero(m[0] == m[0].max())[0]]
    moved = V.features_backward(*args, move=(3, (0, c, yo, xo), (int(arg[0, c, yo, xo]) + 1) % 4))
    for k in range(26):
        d = float((moved[k] - base[k]).norm())
        if k < 19:
            assert d > 1e-6 * float(base[k].norm()), k
        else:
            assert d == 0, k


@pytest.mark.parametrize("n", [1, 3, 8, 64])
def test_arena_layout_matches_library(n):
    """The Python mirror of the arena layout: pool5 where the library says, the dropout regions inside its arena."""
    from umpr_amd._lib import lib
    L = V.arena_layout(n)
    assert L["pool_off"][4] * 4 == lib().size("umpr_vgg16_pool5_offset", n)
    assert L["end"] * 4 <= lib().size("umpr_vgg16_act_bytes", n)
    assert L["pool_off"][4] + n * 25088 == L["fc_off"][0]
