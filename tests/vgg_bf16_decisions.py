"""Rounding-replaying reference of the bf16 VGG16 feature stack (test helper, not a test module).

The bf16 path (umpr_vgg16_bf16_features_fwd / _bwd, bf16_conv.hip) keeps activations and data gradients in bf16 in the
library's CB8-PF layout and accumulates in fp32.  As in tests/vgg_decisions.py the backward becomes linear once the
forward's decisions are fixed, and they are all stored in the bf16 activation arena (api.hip: vgg_b16_layout).  What this
helper adds is the ROUNDING: it rounds to bf16 exactly where the kernels do - the image and the weights as MFMA operands,
every stored activation, the incoming gradient, every stored data gradient - and keeps everything else in float64.  The
only place where the kernels and this reference may then differ is the rounding of each stored data gradient: the fp32
summation order moves a share of the values across a rounding boundary by one bf16 step.

It also holds an index map of the CB8-PF layout written from the layout's description (header comment of bf16_conv.hip,
umpr_pf), independent of the library's converters:
    tensor = [planes = ceil(C / 8)][plane stride ps][8] bf16;  row pitch W + 1;  rows = N (H + 1) + 1;
    pixel (n, y, x) at P = (n (H + 1) + y + 1)(W + 1) + x + 1, stored `lead` = align64(W + 3) pixels into its plane;
    ps = umpr_bf16_tensor_bytes / (16 planes).

Noise floor of the gradient gate, measured by tests/test_vgg_bf16_decisions.py: measure_floor(seed=100): a full-size VGG16
at 224x224 (torchvision initialisation, biases in +-0.05), the arena made by features_forward_bf16, and the distance between
the float64-accumulating and the float32-accumulating run of features_backward_bf16 on that arena - two correct
implementations of the same bf16 backward.  Largest of the 26 parameter gradients (always conv1_1 / conv1_2, the bottom):
    one random image, dense gradient at pool5    : relative L2 6.03e-3, max error / max |ref| 7.06e-3
    one random image, 32 non-zero entries        : relative L2 3.86e-3, max error / max |ref| 4.56e-3
    flat + zero image, dense                     : relative L2 5.35e-3, max error / max |ref| 5.19e-3
    flat + zero image, 32 non-zero entries       : relative L2 4.01e-3, max error / max |ref| 5.30e-3
and per tensor, top to bottom (random image, dense): features.28 3e-8, .26 1.7e-5, .24 1.2e-4, .21 4.6e-4, .19 9e-4, .17 1.6e-3,
.14 2.4e-3, .12 3.1e-3, .10 3.6e-3, .7 4.5e-3, .5 5.7e-3, .2 5.8e-3, .0 6.0e-3; all figures are in FLOOR_MEASURED.
This is well above 2e-3 and NOT a quadrature sum of small independent flips: a relative difference eps in a gradient that is
about to be stored moves a share eps / 2^-8 of its values across a rounding boundary, each by one bf16 step, which is a
relative L2 difference of sqrt(eps 2^-8) - larger than eps while eps < 2^-8.  The recursion starts at fp32 summation noise
under the top layer and climbs towards its fixed point, a fraction of one bf16 step (2^-8 = 3.9e-3), within five layers
(the forward shows the same: test_gpu_bf16.py: test_vgg16_bf16_vs_rounded_operand_oracle (b)).  So the gate keeps PER-TENSOR
constants, REL_L2_BF16 / REL_MAX_BF16 = 4x the largest of the four measured values of that tensor: the kernels' MFMA and
split-K order is a third summation order, and one CPU sample underestimates the spread.  That is 2.4e-2 / 2.8e-2 at the
bottom of the network, against 0.5 in the comparison with the fp32 path; one wrong pool-4 route or one dropped ReLU mask
lies outside it for every tensor below the defect (test_vgg_bf16_decisions.py).  Under the top two layers nothing has been
re-rounded yet and the measured value is fp32 summation noise alone (down to 0): there the constant is the fp32 path's own
gate, FP32_REL_L2 / FP32_REL_MAX (see below), which no tensor's constant goes under.
"""
import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

from vgg_decisions import VGG16_BLOCKS, VGG16_PARAM_NAMES, pool_argmax, pool_backward  # noqa: F401  (re-exported)

# ---- measured floor and the gate derived from it (see the module docstring; reproduce with measure_floor) ------------
# {case: [(relative L2, max error / max |ref|)] in VGG16_PARAM_NAMES order}, float32- against float64-accumulating backward
FLOOR_MEASURED = {
    "random dense": [
        (5.95e-03, 5.46e-03), (6.03e-03, 7.04e-03), (5.76e-03, 6.03e-03), (5.64e-03, 5.14e-03),
        (5.69e-03, 7.04e-03), (5.70e-03, 7.06e-03), (4.47e-03, 4.40e-03), (4.47e-03, 4.38e-03),
        (3.62e-03, 3.96e-03), (3.64e-03, 3.80e-03), (3.05e-03, 3.48e-03), (3.09e-03, 3.44e-03),
        (2.41e-03, 2.17e-03), (2.42e-03, 2.19e-03), (1.58e-03, 1.67e-03), (1.58e-03, 1.66e-03),
        (9.14e-04, 9.05e-04), (9.23e-04, 9.02e-04), (4.59e-04, 6.52e-04), (4.67e-04, 6.31e-04),
        (1.19e-04, 2.40e-04), (1.21e-04, 2.47e-04), (1.67e-05, 7.02e-05), (1.65e-05, 6.91e-05),
        (2.81e-08, 7.86e-08), (0.00e+00, 0.00e+00),
    ],
    "random sparse": [
        (3.86e-03, 4.56e-03), (3.65e-03, 4.29e-03), (3.48e-03, 3.10e-03), (3.40e-03, 3.02e-03),
        (3.26e-03, 2.76e-03), (3.26e-03, 2.87e-03), (2.79e-03, 3.04e-03), (2.81e-03, 2.99e-03),
        (2.47e-03, 2.93e-03), (2.50e-03, 2.94e-03), (1.79e-03, 1.62e-03), (1.78e-03, 1.62e-03),
        (9.94e-04, 1.14e-03), (1.01e-03, 1.22e-03), (5.07e-04, 5.05e-04), (5.20e-04, 4.91e-04),
        (2.19e-04, 2.74e-04), (2.37e-04, 3.04e-04), (5.71e-05, 1.42e-04), (6.60e-05, 1.40e-04),
        (1.20e-05, 6.71e-05), (1.17e-05, 6.45e-05), (8.24e-08, 1.96e-07), (1.34e-08, 3.21e-08),
        (0.00e+00, 0.00e+00), (0.00e+00, 0.00e+00),
    ],
    "flat+zero dense": [
        (4.70e-03, 4.92e-03), (5.35e-03, 5.19e-03), (4.68e-03, 4.88e-03), (4.84e-03, 4.62e-03),
        (3.33e-03, 3.32e-03), (3.84e-03, 3.35e-03), (2.81e-03, 3.50e-03), (3.04e-03, 4.34e-03),
        (2.34e-03, 2.85e-03), (2.62e-03, 3.28e-03), (1.80e-03, 2.04e-03), (1.85e-03, 1.91e-03),
        (1.34e-03, 1.28e-03), (1.36e-03, 1.17e-03), (9.49e-04, 9.55e-04), (9.36e-04, 8.69e-04),
        (5.29e-04, 6.43e-04), (5.41e-04, 5.90e-04), (2.64e-04, 3.96e-04), (2.77e-04, 3.70e-04),
        (8.91e-05, 2.59e-04), (9.72e-05, 2.78e-04), (6.45e-06, 3.88e-05), (6.59e-06, 3.13e-05),
        (4.10e-08, 1.56e-07), (1.38e-09, 9.48e-09),
    ],
    "flat+zero sparse": [
        (4.01e-03, 5.30e-03), (3.63e-03, 4.09e-03), (3.39e-03, 3.09e-03), (3.44e-03, 3.63e-03),
        (2.44e-03, 2.04e-03), (3.08e-03, 3.49e-03), (2.53e-03, 2.23e-03), (2.81e-03, 3.06e-03),
        (2.59e-03, 3.01e-03), (2.75e-03, 3.76e-03), (1.79e-03, 1.34e-03), (1.86e-03, 1.45e-03),
        (1.22e-03, 8.44e-04), (1.20e-03, 8.95e-04), (6.24e-04, 7.25e-04), (6.12e-04, 6.47e-04),
        (2.85e-04, 5.36e-04), (2.75e-04, 5.74e-04), (8.62e-05, 3.06e-04), (8.13e-05, 3.06e-04),
        (2.94e-06, 1.58e-05), (3.33e-06, 1.64e-05), (7.22e-08, 2.38e-07), (9.87e-09, 3.43e-08),
        (0.00e+00, 0.00e+00), (0.00e+00, 0.00e+00),
    ],
}
# No tensor is held tighter than the fp32 path's own gate (tests/test_gpu_vgg_grad.py: REL_L2, REL_MAX).  Near the top of the
# network no data gradient has been re-rounded yet and the recorded distance (1e-8 .. 1e-5) is pure fp32 summation noise of
# the CPU's blocked order; products of bf16 values are exact in fp32, so the kernels' weight-gradient sums - up to n x 50176
# terms over MFMA chunks and split-K slabs - differ from float64 as the fp32 kernels' sums do, and that bound is theirs.
FP32_REL_L2, FP32_REL_MAX = 1e-4, 1e-3
REL_L2_BF16 = {name: max(4 * max(FLOOR_MEASURED[c][k][0] for c in FLOOR_MEASURED), FP32_REL_L2)
               for k, name in enumerate(VGG16_PARAM_NAMES[:26])}
REL_MAX_BF16 = {name: max(4 * max(FLOOR_MEASURED[c][k][1] for c in FLOOR_MEASURED), FP32_REL_MAX)
                for k, name in enumerate(VGG16_PARAM_NAMES[:26])}


def gate(name):
    """(relative L2 bound, max error / max |ref| bound) of the gradient of parameter `name`"""
    return REL_L2_BF16[name], REL_MAX_BF16[name]


def q(t):
    """Round-to-nearest-even to bf16, kept in float64.  (Values pass through float32 first; every value rounded here is
    either a float32 already or a float64 sum whose float32 rounding sits 2^16 times finer than the bf16 grid.)"""
    f = t.detach().to(torch.float32).contiguous()
    bits = f.view(torch.int32)
    r = (bits + 0x7FFF + ((bits >> 16) & 1)) & -65536         # add half an ulp minus one, plus the kept part's last bit
    return r.view(torch.float32).to(torch.float64)


# ---- CB8-PF index map ------------------------------------------------------------------------------------------------
def align64(v):
    return (v + 63) // 64 * 64


def planes_of(C):
    return (C + 7) // 8


def plane_stride(nbytes, C):
    """pixels per plane of a CB8-PF tensor of `nbytes` bytes (umpr_bf16_tensor_bytes) with C channels"""
    assert nbytes % (16 * planes_of(C)) == 0, (nbytes, C)
    return nbytes // (16 * planes_of(C))


def pixel_index(N, H, W):
    """index into a plane ([ps] pixels, lead guard included) of pixel (n, y, x): LongTensor [N][H][W]"""
    n = torch.arange(N).view(N, 1, 1)
    y = torch.arange(H).view(1, H, 1)
    x = torch.arange(W).view(1, 1, W)
    return align64(W + 3) + (n * (H + 1) + y + 1) * (W + 1) + x + 1


def pixel_mask(N, C, H, W, ps):
    """bool [planes][ps][8]: true exactly on the real pixels of the real channels"""
    idx = pixel_index(N, H, W).reshape(-1)
    assert int(idx.max()) < ps, (int(idx.max()), ps)
    pix = torch.zeros(ps, dtype=torch.bool)
    pix[idx] = True
    ch = (torch.arange(planes_of(C) * 8) < C).view(planes_of(C), 1, 8)
    return pix.view(1, ps, 1) & ch


def _bf16_bits_to_f64(bits16):
    return ((bits16.to(torch.int32) & 0xFFFF) << 16).view(torch.float32).to(torch.float64)


def decode(buf, N, C, H, W, images=None):
    """float64 [k][C][H][W] (k = len(images), default all N) from the bytes of a CB8-PF tensor (uint8 tensor, any device)"""
    pl = planes_of(C)
    ps = plane_stride(buf.numel(), C)
    t = buf.view(torch.int16).view(pl, ps, 8)
    idx = pixel_index(N, H, W)
    if images is not None:
        idx = idx[list(images)]
    k = idx.shape[0]
    px = t.index_select(1, idx.reshape(-1).to(buf.device))                  # [pl][k H W][8]
    px = px.view(pl, k, H, W, 8).permute(1, 0, 4, 2, 3).reshape(k, pl * 8, H, W)[:, :C]
    return _bf16_bits_to_f64(px.contiguous()).cpu()


def encode(x, ps):
    """bytes (uint8 [planes * ps * 16]) of the CB8-PF tensor holding x [N][C][H][W], whose values must be bf16-exact:
    zeros everywhere but on the real pixels of the real channels"""
    N, C, H, W = x.shape
    pl = planes_of(C)
    f = x.detach().to("cpu", torch.float32).contiguous()
    bits = f.view(torch.int32)
    assert bool(((bits & 0xFFFF) == 0).all()), "encode: values are not bf16-exact"
    hi = (bits >> 16).to(torch.int16)                                      # arithmetic shift: the top 16 bits, as int16
    full = torch.zeros(N, pl * 8, H, W, dtype=torch.int16)
    full[:, :C] = hi
    t = torch.zeros(pl, ps, 8, dtype=torch.int16)
    t[:, pixel_index(N, H, W).reshape(-1)] = full.view(N, pl, 8, H, W).permute(1, 0, 3, 4, 2).reshape(pl, N * H * W, 8)
    return t.view(torch.uint8).reshape(-1)


def nonzero_outside(buf, N, C, H, W):
    """number of elements of the CB8-PF tensor `buf` (uint8, any device) outside pixel_mask that are not zero (+0 or -0)"""
    pl = planes_of(C)
    ps = plane_stride(buf.numel(), C)
    t = buf.view(torch.int16).view(pl, ps, 8)
    outside = ~pixel_mask(N, C, H, W, ps).to(buf.device)
    return int((((t & 0x7FFF) != 0) & outside).sum())


# ---- the bf16 activation arena ---------------------------------------------------------------------------------------
def arena_layout_bf16(n, lib, blocks=VGG16_BLOCKS, hw=224):
    """Byte offsets and sizes of the 13 conv and 5 pool CB8-PF tensors of the bf16 activation arena (api.hip:
    vgg_b16_layout): each umpr_bf16_tensor_bytes(n, C, hw, hw) rounded up to 1024; the end is the library's arena size."""
    L = {"conv_off": [], "conv_bytes": [], "conv_shape": [], "pool_off": [], "pool_bytes": [], "pool_shape": []}
    off = 0
    for blk in blocks:
        for c in blk:
            nb = lib.size("umpr_bf16_tensor_bytes", n, c, hw, hw)
            L["conv_off"].append(off)
            L["conv_bytes"].append(nb)
            L["conv_shape"].append((c, hw, hw))
            off += (nb + 1023) // 1024 * 1024
        hw //= 2
        nb = lib.size("umpr_bf16_tensor_bytes", n, blk[-1], hw, hw)
        L["pool_off"].append(off)
        L["pool_bytes"].append(nb)
        L["pool_shape"].append((blk[-1], hw, hw))
        off += (nb + 1023) // 1024 * 1024
    L["end"] = off
    assert off == lib.size("umpr_vgg16_bf16_act_bytes", n), (off, lib.size("umpr_vgg16_bf16_act_bytes", n))
    return L


def arena_tensors(acts, n, lib):
    """[(name, byte view, (C, H, W))] of the arena's 18 tensors, conv0..conv12 then pool0..pool4"""
    L = arena_layout_bf16(n, lib)
    assert acts.dtype == torch.uint8 and acts.numel() >= L["end"], (acts.dtype, acts.numel(), L["end"])
    out = []
    for kind in ("conv", "pool"):
        for i, (o, nb, s) in enumerate(zip(L[kind + "_off"], L[kind + "_bytes"], L[kind + "_shape"])):
            out.append((f"{kind}{i}", acts[o:o + nb], s))
    return out


def read_arena_bf16(acts, n, images, lib):
    """float64 CPU copies of the chosen images' activations from the bf16 arena `acts` (uint8, as _VGGFeaturesBF16 keeps it),
    decoded with the Python index map: {"conv": 13 post-ReLU conv outputs [k][C][H][W], "pool": 5 pool outputs}"""
    ts = arena_tensors(acts, n, lib)
    dec = [decode(buf, n, s[0], s[1], s[2], images) for _, buf, s in ts]
    return {"conv": dec[:13], "pool": dec[13:]}


# ---- the rounding-replaying network ----------------------------------------------------------------------------------
def features_forward_bf16(images, conv_params, block_sizes, acc_dtype=torch.float64):
    """conv3x3(pad 1)+ReLU blocks, each closed by a 2x2 max-pool, as the bf16 path computes them: every layer - the first
    included, conv1_bf16_fwd_kernel rounds the image and the weights - is q(relu(conv(q(x), q(w)) + b)), a pool is the
    window maximum.  Returns (convs, pools) in float64.  acc_dtype=torch.float32 accumulates the same rounded operands in
    float32 (another summation order of the same network)."""
    cv = lambda t: t.detach().to("cpu", torch.float64)   # noqa: E731
    convs, pools = [], []
    h, ci = q(cv(images)), 0
    for nb in block_sizes:
        for _ in range(nb):
            w, b = q(cv(conv_params[2 * ci])), cv(conv_params[2 * ci + 1])
            z = F.conv2d(h.to(acc_dtype), w.to(acc_dtype), b.to(acc_dtype), padding=1)
            h = q(torch.relu(z).to(torch.float64))
            convs.append(h)
            ci += 1
        h = F.max_pool2d(h, 2, 2)
        pools.append(h)
    return convs, pools


def features_backward_bf16(images, convs, pools, conv_params, d_pool, block_sizes, move=None, acc_dtype=torch.float64,
                           drop_mask_at=None, d_pools=None):
    """Backward of that network as umpr_vgg16_bf16_features_bwd runs it, every decision taken from the given (arena)
    activations: the incoming gradient is q(d_pool); pool_backward routes it; dw = conv2d_weight(xin, gz) and db = gz.sum
    stay unrounded (xin of conv 0 is q(images)); dx = q(conv2d_input(gz, q(w))), then the ReLU mask xin > 0 where the
    input is a conv output (j > 0).  Returns [dw0, db0, dw1, db1, ...] in float64.
    acc_dtype=torch.float32: the same backward with float32 convolutions and sums on the same rounded operands - a second
    summation order (the noise floor, and the CPU stand-in for a correct kernel).  move = (block, window index, element)
    re-routes one pool window (vgg_decisions.pool_backward); drop_mask_at = ci omits the ReLU mask on conv ci's output
    (sensitivity tests only).  A dict `d_pools` receives the (rounded) gradient w.r.t. every pool output, keyed by block."""
    cv = lambda t: t.detach().to("cpu", torch.float64)   # noqa: E731
    acc = lambda t: t.to(acc_dtype)   # noqa: E731
    assert len(convs) == sum(block_sizes) and len(pools) == len(block_sizes) and len(conv_params) == 2 * len(convs)
    grads = [None] * len(conv_params)
    g = q(cv(d_pool))
    ci = len(convs) - 1
    for b in reversed(range(len(block_sizes))):
        if d_pools is not None:
            d_pools[b] = g
        g = pool_backward(cv(convs[ci]), g, move[1:] if move is not None and move[0] == b else None)
        for j in reversed(range(block_sizes[b])):
            xin = q(cv(images)) if ci == 0 else cv(pools[b - 1]) if j == 0 else cv(convs[ci - 1])
            w = q(cv(conv_params[2 * ci]))
            grads[2 * ci] = conv2d_weight(acc(xin), w.shape, acc(g), padding=1).to(torch.float64)
            grads[2 * ci + 1] = acc(g).sum((0, 2, 3)).to(torch.float64)
            if ci == 0:
                break
            g = q(conv2d_input(xin.shape, acc(w), acc(g), padding=1).to(torch.float64))
            if j > 0 and drop_mask_at != ci - 1:     # input is a conv output: its ReLU; the pool backward masks a pool input
                g = g * (xin > 0)
            ci -= 1
    return grads


def conv_params(seed, blocks=VGG16_BLOCKS, bias=0.05, dtype=torch.float32):
    """[w0, b0, w1, b1, ...] of a conv stack on 3-channel images: torchvision's VGG initialisation (kaiming normal, fan-out)
    plus small random biases - with zero biases a zero image has no gradient at all (test_gpu_vgg_grad.py: _vgg)"""
    g = torch.Generator().manual_seed(seed)
    ps, cin = [], 3
    for blk in blocks:
        for c in blk:
            ps += [(torch.randn(c, cin, 3, 3, generator=g) * (2.0 / (9 * c)) ** 0.5).to(dtype),
                   ((torch.rand(c, generator=g) * 2 - 1) * bias).to(dtype)]
            cin = c
    return ps


def images(seed, n, hw=224):
    """random images; with n >= 3 the second-last is constant per channel (a flat photo) and the last all zero (a missing
    photo), as _images of test_gpu_vgg_grad.py"""
    g = torch.Generator().manual_seed(seed)
    x = torch.rand(n, 3, hw, hw, generator=g)
    if n >= 3:
        x[n - 2] = torch.rand(3, 1, 1, generator=g)
        x[n - 1] = 0
    return x


def sparse_upstream(shape, seed, entries=32):
    """an upstream gradient that is non-zero (randn) on `entries` random positions only"""
    g = torch.Generator().manual_seed(seed)
    d = torch.zeros(shape)
    flat = d.view(-1)
    flat[torch.randperm(flat.numel(), generator=g)[:entries]] = torch.randn(entries, generator=g)
    return d


def distances(got, ref):
    """[(relative L2, max error / max |ref|)] per tensor"""
    out = []
    for a, r in zip(got, ref):
        a, r = a.detach().double().cpu().reshape(r.shape), r.double()
        out.append((float((a - r).norm() / r.norm()), float((a - r).abs().max() / r.abs().max())))
    return out
