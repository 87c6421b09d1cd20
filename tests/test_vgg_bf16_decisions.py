"""CPU tests of the rounding-replaying bf16 VGG reference (tests/vgg_bf16_decisions.py) that the GPU gate of
tests/test_gpu_vgg_bf16_grad.py compares the bf16 HIP backward with: the reference itself against torch autograd, the
Python CB8-PF index map, the noise floor the gate's constants come from (measure_floor), and the gate's sensitivity to a
dropped ReLU mask and to one wrong pool route.  No GPU needed."""
import pytest
import torch
import torch.nn.functional as F

import vgg_bf16_decisions as B
import vgg_decisions as V

# a reduced network: two blocks on 16x16 images -> a 4x4 last pool
BLOCKS = ((8, 8), (16, 16, 16))
SIZES = [len(b) for b in BLOCKS]
HW = 16
VGG_SIZES = [len(b) for b in B.VGG16_BLOCKS]


def _params(seed, blocks=BLOCKS, dtype=torch.float64):
    return B.conv_params(seed, blocks, dtype=dtype)


def _images(seed, n, hw=HW):
    return B.images(seed, n, hw)


_sparse = B.sparse_upstream


class _RoundForward(torch.autograd.Function):
    """value rounded to bf16, gradient passed straight through"""

    @staticmethod
    def forward(ctx, x):
        return B.q(x)

    @staticmethod
    def backward(ctx, g):
        return g


class _RoundBackward(torch.autograd.Function):
    """value passed through, gradient rounded to bf16"""

    @staticmethod
    def forward(ctx, x):
        return x.clone()

    @staticmethod
    def backward(ctx, g):
        return B.q(g)


def _autograd_network(x, ps, blocks, rf, rb):
    """the network with rf at every forward rounding site (image, weights, stored activations) and rb at every backward
    one (the gradient arriving at the last pool, every data gradient leaving a convolution); returns (pool output, convs,
    pools)"""
    convs, pools = [], []
    h, ci = rf(x.double()), 0
    for blk in blocks:
        for _ in blk:
            if ci > 0:
                h = rb(h)
            h = rf(F.relu(F.conv2d(h, rf(ps[2 * ci]), ps[2 * ci + 1], padding=1)))
            convs.append(h.detach())
            ci += 1
        h = F.max_pool2d(h, 2, 2)
        pools.append(h.detach())
    return rb(h), convs, pools


def _close(got, ref, rel=1e-12):
    for k, (a, r) in enumerate(zip(got, ref)):
        scale = float(r.abs().max())
        assert scale > 0, k
        assert float((a - r).abs().max()) <= rel * scale, (k, float((a - r).abs().max()), scale)


def test_rounding_free_limit_is_the_fp32_paths_reference(monkeypatch):
    """With q the identity the bf16 reference is vgg_decisions.features_backward, and torch autograd, to float64 accuracy."""
    monkeypatch.setattr(B, "q", lambda t: t.detach().to(torch.float64))
    x = _images(1, 4).double()
    ps = [p.requires_grad_(True) for p in _params(2)]
    ident = lambda t: t   # noqa: E731
    out, convs, pools = _autograd_network(x, ps, BLOCKS, ident, ident)
    d = torch.randn(out.shape, generator=torch.Generator().manual_seed(3), dtype=torch.float64)
    out.backward(d)
    fconvs, fpools = B.features_forward_bf16(x, ps, SIZES)
    for a, r in zip(fconvs + fpools, convs + pools):
        assert torch.equal(a, r)
    got = B.features_backward_bf16(x, convs, pools, ps, d, SIZES)
    _close(got, V.features_backward(x, convs, pools, ps, d, SIZES))
    _close(got, [p.grad for p in ps])


def test_reference_rounds_where_straight_through_autograd_does():
    """The reference against torch autograd through the same network with a straight-through bf16 rounding at every
    rounding site - random, flat and all-zero images, so ties at a positive maximum and all-zero windows are routed too."""
    n = 5
    x = _images(11, n)
    ps = [p.requires_grad_(True) for p in _params(12)]
    out, convs, pools = _autograd_network(x, ps, BLOCKS, _RoundForward.apply, _RoundBackward.apply)
    d = torch.randn(out.shape, generator=torch.Generator().manual_seed(13), dtype=torch.float64)
    out.backward(d)
    fconvs, fpools = B.features_forward_bf16(x, ps, SIZES)
    for a, r in zip(fconvs + fpools, convs + pools):
        assert torch.equal(a, r) and torch.equal(B.q(a), a)
    ties = zero = 0
    for ci in (1, 4):
        y = convs[ci]
        win = y.reshape(n, y.shape[1], y.shape[2] // 2, 2, y.shape[3] // 2, 2).permute(0, 1, 2, 4, 3, 5).flatten(-2)
        top2 = win.topk(2, -1).values
        ties += int(((top2[..., 0] == top2[..., 1]) & (top2[..., 0] > 0)).sum())
        zero += int((top2[..., 0] == 0).sum())
    assert ties > 0 and zero > 0, (ties, zero)
    got = B.features_backward_bf16(x, convs, pools, ps, d, SIZES)
    _close(got, [p.grad for p in ps])
    # and the rounding matters: the unrounded backward on the same activations is further away than float64 noise
    plain = V.features_backward(B.q(x), convs, pools, [B.q(p) if p.dim() == 4 else p for p in ps], d, SIZES)
    assert max(l2 for l2, _ in B.distances(plain[:2], got[:2])) > 1e-5


def test_q_is_round_to_nearest_even():
    one, ulp = 1.0, 2.0 ** -7           # bf16 spacing in [1, 2)
    x = torch.tensor([one + ulp / 2, one + 3 * ulp / 2, one + ulp / 2 + 2.0 ** -20, -(one + ulp / 2), 0.0, 3.0e-39, one + ulp])
    want = torch.tensor([one, one + 2 * ulp, one + ulp, -one, 0.0, float(torch.tensor(3.0e-39).bfloat16()), one + ulp])
    assert torch.equal(B.q(x), want.double())
    r = torch.randn(10000, generator=torch.Generator().manual_seed(1)) * 100
    assert torch.equal(B.q(r), r.bfloat16().double())


@pytest.mark.parametrize("shape", [(2, 3, 14, 14), (1, 8, 2, 2), (3, 12, 4, 6), (2, 64, 14, 14)])
def test_index_map_self_check(shape):
    """The mask covers exactly N*C*H*W elements, decode inverts encode, and a pixel sits where the layout's description says."""
    N, C, H, W = shape
    lead, ptot = B.align64(W + 3), (N * (H + 1) + 1) * (W + 1)
    ps = B.align64(lead + ptot + 100)
    mask = B.pixel_mask(N, C, H, W, ps)
    assert tuple(mask.shape) == ((C + 7) // 8, ps, 8) and int(mask.sum()) == N * C * H * W
    x = B.q(torch.randn(shape, generator=torch.Generator().manual_seed(sum(shape))))
    x[0, 0, 0, 0] = 1.5
    buf = B.encode(x, ps)
    assert buf.dtype == torch.uint8 and buf.numel() == ((C + 7) // 8) * ps * 16 == 16 * mask[..., 0].numel()
    assert torch.equal(B.decode(buf, N, C, H, W), x)
    assert torch.equal(B.decode(buf, N, C, H, W, [N - 1]), x[N - 1:])
    assert B.nonzero_outside(buf, N, C, H, W) == 0
    t = buf.view(torch.int16).view(-1, ps, 8)
    assert bool((t[~mask] == 0).all())
    n, c, y, xx = N - 1, C - 1, H - 1, W - 2
    P = (n * (H + 1) + y + 1) * (W + 1) + xx + 1
    want = torch.tensor([float(x[n, c, y, xx])]).bfloat16().view(torch.int16)
    assert int(t[c // 8, lead + P, c % 8]) == int(want)
    assert int(t[0, lead + (W + 1) + 1, 0]) == 0x3FC0              # 1.5 at pixel (0, 0, 0) of channel 0
    # a stray value in a pad is seen
    t[0, lead + (W + 1), 0] = 0x3F80                               # column 0 of the first image row
    assert B.nonzero_outside(buf, N, C, H, W) == 1


@pytest.mark.parametrize("n", [1, 3, 64])
def test_bf16_arena_layout_matches_library(n):
    """arena_layout_bf16 ends where the library's arena ends, and every tensor's plane holds lead + all pixels"""
    from umpr_amd._lib import lib
    L = B.arena_layout_bf16(n, lib())
    assert len(L["conv_off"]) == 13 and len(L["pool_off"]) == 5
    for kind in ("conv", "pool"):
        for nb, (c, h, w) in zip(L[kind + "_bytes"], L[kind + "_shape"]):
            assert B.plane_stride(nb, c) >= B.align64(w + 3) + (n * (h + 1) + 1) * (w + 1)


# ------------------------------------------------------------------------------------------------ noise floor, full size
def measure_floor(seed=100):
    """The run behind FLOOR_MEASURED: a full-size VGG16 at 224x224, the arena made by features_forward_bf16, on one random
    image and on the flat-plus-zero pair, a dense and a sparse gradient at pool5; the backward with float64 and with float32
    accumulation.  Returns {case: [(relative L2, max error / max |ref|)] * 26}."""
    ps = _params(seed, B.VGG16_BLOCKS, dtype=torch.float32)
    out = {}
    for tag, x in (("random", _images(seed + 1, 1, 224)), ("flat+zero", _images(seed + 2, 3, 224)[1:])):
        convs, pools = B.features_forward_bf16(x, ps, VGG_SIZES)
        g = torch.Generator().manual_seed(seed + 3)
        for kind, d in (("dense", torch.randn(pools[-1].shape, generator=g)), ("sparse", _sparse(pools[-1].shape, seed + 4))):
            ref = B.features_backward_bf16(x, convs, pools, ps, d, VGG_SIZES)
            f32 = B.features_backward_bf16(x, convs, pools, ps, d, VGG_SIZES, acc_dtype=torch.float32)
            out[f"{tag} {kind}"] = B.distances(f32, ref)
    return out


def gate_outside(got, ref, names=B.VGG16_PARAM_NAMES):
    """[(name, relative L2, max error / max |ref|)] of the tensors outside the gate (B.gate of each name)"""
    bad = []
    for name, (l2, mx) in zip(names, B.distances(got, ref)):
        b_l2, b_max = B.gate(name)
        if not (l2 <= b_l2 and mx <= b_max):
            bad.append((name, l2, mx))
    return bad


@pytest.fixture(scope="module")
def full_size():
    """one random full-size image, its arena, a sparse gradient at pool5 and the float64 reference backward"""
    ps = _params(300, B.VGG16_BLOCKS, dtype=torch.float32)
    x = _images(301, 1, 224)
    convs, pools = B.features_forward_bf16(x, ps, VGG_SIZES)
    d = _sparse(pools[-1].shape, 302)
    d_pools = {}
    ref = B.features_backward_bf16(x, convs, pools, ps, d, VGG_SIZES, d_pools=d_pools)
    return {"ps": ps, "x": x, "convs": convs, "pools": pools, "d": d, "ref": ref, "d_pools": d_pools}


def test_noise_floor_is_inside_the_gate():
    """Two correct implementations of the same bf16 backward - float64 and float32 accumulation on the same arena - at full
    size: every one of the 26 distances is printed, and is inside the gate whose constants are 4x the floor recorded in
    the helper (a fresh sample of the same measurement, on other seeds than the recorded one)."""
    floor = measure_floor(seed=500)
    for case, ds in floor.items():
        for name, (l2, mx) in zip(B.VGG16_PARAM_NAMES, ds):
            print(f"floor {case} d{name}: rel_l2={l2:.3e} max_err/max={mx:.3e} gate {B.gate(name)[0]:.3e} / {B.gate(name)[1]:.3e}")
    for case, ds in floor.items():
        for name, (l2, mx) in zip(B.VGG16_PARAM_NAMES, ds):
            assert l2 <= B.gate(name)[0] and mx <= B.gate(name)[1], (case, name, l2, mx)


def test_recorded_floor_and_gate_constants_belong_together():
    """REL_L2_BF16 / REL_MAX_BF16 are 4x the largest recorded distance of each tensor, never below the fp32 gate"""
    assert sorted(B.FLOOR_MEASURED) == sorted(["random dense", "random sparse", "flat+zero dense", "flat+zero sparse"])
    for k, name in enumerate(B.VGG16_PARAM_NAMES[:26]):
        l2 = max(B.FLOOR_MEASURED[c][k][0] for c in B.FLOOR_MEASURED)
        mx = max(B.FLOOR_MEASURED[c][k][1] for c in B.FLOOR_MEASURED)
        assert B.REL_L2_BF16[name] == max(4 * l2, B.FP32_REL_L2) and B.REL_MAX_BF16[name] == max(4 * mx, B.FP32_REL_MAX)
        assert B.gate(name) == (B.REL_L2_BF16[name], B.REL_MAX_BF16[name])


# ------------------------------------------------------------------------------------------------ sensitivity
def _reduced_case():
    x = _images(21, 3)
    ps = _params(22)
    convs, pools = B.features_forward_bf16(x, ps, SIZES)
    d = torch.randn(pools[-1].shape, generator=torch.Generator().manual_seed(23))
    names = [f"conv{i}.{t}" for i in range(sum(SIZES)) for t in ("weight", "bias")]
    return x, ps, convs, pools, d, names


def _loosest(names):
    """on the reduced network every tensor is held to the LOOSEST pair of the full-size constants: a defect outside it is
    outside every tensor's own gate"""
    return [(n, max(B.REL_L2_BF16.values()), max(B.REL_MAX_BF16.values())) for n in names]


def _outside_loosest(got, ref, names):
    return [(n, l2, mx) for (n, b_l2, b_max), (l2, mx) in zip(_loosest(names), B.distances(got, ref))
            if not (l2 <= b_l2 and mx <= b_max)]


def test_gate_sensitivity_on_the_reduced_network():
    """The float32-accumulating backward (the stand-in for a correct kernel) passes the gate; the same backward without the
    ReLU mask of one mid-network layer, or with one window of the first pool routed to its neighbour, does not."""
    x, ps, convs, pools, d, names = _reduced_case()
    ref = B.features_backward_bf16(x, convs, pools, ps, d, SIZES)
    args = (x, convs, pools, ps, d, SIZES)
    assert not _outside_loosest(B.features_backward_bf16(*args, acc_dtype=torch.float32), ref, names)
    dropped = B.features_backward_bf16(*args, acc_dtype=torch.float32, drop_mask_at=2)
    bad = [n for n, _, _ in _outside_loosest(dropped, ref, names)]
    assert set(bad) >= {f"conv{i}.{t}" for i in (0, 1, 2) for t in ("weight", "bias")}, bad
    assert not [n for n in bad if n.startswith(("conv3", "conv4"))], bad
    d_pools = {}
    sp = _sparse(pools[-1].shape, 24, 8)
    ref = B.features_backward_bf16(x, convs, pools, ps, sp, SIZES, d_pools=d_pools)
    arg, m = B.pool_argmax(convs[1])
    score = d_pools[0].abs() * (m > 0)
    win = tuple(int(i) for i in torch.nonzero(score == score.max())[0])
    args = (x, convs, pools, ps, sp, SIZES)
    assert not _outside_loosest(B.features_backward_bf16(*args, acc_dtype=torch.float32), ref, names)
    moved = B.features_backward_bf16(*args, acc_dtype=torch.float32, move=(0, win, (int(arg[win]) + 1) % 4))
    bad = [n for n, _, _ in _outside_loosest(moved, ref, names)]
    assert set(bad) >= {"conv0.weight", "conv0.bias", "conv1.weight"}, bad


def test_gate_passes_the_stand_in_at_full_size(full_size):
    f = full_size
    got = B.features_backward_bf16(f["x"], f["convs"], f["pools"], f["ps"], f["d"], VGG_SIZES, acc_dtype=torch.float32)
    assert not gate_outside(got, f["ref"])


def test_gate_catches_one_wrong_pool4_route_at_full_size(full_size):
    """One pool-4 window - the one carrying the largest upstream gradient, with a gradient at pool5 that is non-zero on a few
    dozen entries - routed to the next element of its window: every gradient below it leaves its own gate, except the bias of
    the conv feeding that pool (its gradient sums the moved value within the same channel)."""
    f = full_size
    arg, m = B.pool_argmax(f["convs"][9])
    score = f["d_pools"][3].abs() * (m > 0)
    win = tuple(int(i) for i in torch.nonzero(score == score.max())[0])
    moved = B.features_backward_bf16(f["x"], f["convs"], f["pools"], f["ps"], f["d"], VGG_SIZES, acc_dtype=torch.float32,
                                     move=(3, win, (int(arg[win]) + 1) % 4))
    bad = {n: (l2, mx) for n, l2, mx in gate_outside(moved, f["ref"])}
    for name, (l2, mx) in zip(B.VGG16_PARAM_NAMES, B.distances(moved, f["ref"])):
        print(f"moved pool4 route d{name}: rel_l2={l2:.3e} ({l2 / B.gate(name)[0]:.1f}x the bound) max_err/max={mx:.3e}")
    assert set(bad) == set(B.VGG16_PARAM_NAMES[:19]), sorted(set(B.VGG16_PARAM_NAMES[:19]) ^ set(bad))


def test_gate_catches_a_dropped_relu_mask_at_full_size(full_size):
    """The backward without the ReLU mask on conv3_2's output (features.12): every gradient below leaves its gate, none above."""
    f = full_size
    dropped = B.features_backward_bf16(f["x"], f["convs"], f["pools"], f["ps"], f["d"], VGG_SIZES, acc_dtype=torch.float32,
                                       drop_mask_at=5)
    bad = {n for n, _, _ in gate_outside(dropped, f["ref"])}
    assert bad == set(B.VGG16_PARAM_NAMES[:12]), sorted(bad ^ set(B.VGG16_PARAM_NAMES[:12]))
