"""Decision-conditioned reference of the VGG16 backward (test helper, not a test module).

Once the forward's decisions are fixed - which ReLU outputs are positive, which element of each 2x2 window the max-pool
picked, which dropout units were kept - the backward of the network is linear in the upstream gradient and smooth in
every value.  All of those decisions are stored in the fp32 activation arena of umpr_vgg16_features_fwd /
umpr_vgg16_classifier_fwd (api.hip: vgg_layout).  The functions here read that arena back and run the backward in
float64 on the CPU with the HIP activations as the layer inputs, so that forward rounding stays out of the comparison and
a HIP gradient can be held to a tight elementwise bound instead of a draw over which decision lands on which side.

The feature part is generic in channel counts and map size (tests/test_vgg_decisions.py runs it on a reduced network
against torch autograd); the arena reader is VGG16-D at 224x224.
"""
import torch
from torch.nn.grad import conv2d_input, conv2d_weight

# VGG16-D: output channels of each convolution, grouped by block (a 2x2 max-pool closes every block)
VGG16_BLOCKS = ((64, 64), (128, 128), (256, 256, 256), (512, 512, 512), (512, 512, 512))
VGG16_HIDDEN = 4096
# parameter names of VGG16.param_list() order (features.N / classifier.N of torchvision's layer list)
VGG16_PARAM_NAMES = [f"features.{i}.{t}" for i in (0, 2, 5, 7, 10, 12, 14, 17, 19, 21, 24, 26, 28) for t in ("weight", "bias")] + \
                    [f"classifier.{i}.{t}" for i in (0, 3, 6) for t in ("weight", "bias")]
# max-pool window elements in the order the HIP pool kernels test them (conv3x3.hip: maxpool2_bwd_relu_kernel)
WINDOW_ORDER = ((0, 0), (0, 1), (1, 0), (1, 1))


def arena_layout(n, blocks=VGG16_BLOCKS, hw=224, hidden=VGG16_HIDDEN):
    """Float offsets of the conv / pool / fc / dropout regions of the fp32 activation arena (api.hip: vgg_layout); the
    transformed-input (V) slots that follow them are not described.  Every region is [n][C][H][W] or [n][hidden]."""
    L = {"conv_off": [], "conv_shape": [], "pool_off": [], "pool_shape": []}
    off = 0
    for blk in blocks:
        for c in blk:
            L["conv_off"].append(off)
            L["conv_shape"].append((c, hw, hw))
            off += n * c * hw * hw
        hw //= 2
        L["pool_off"].append(off)
        L["pool_shape"].append((blk[-1], hw, hw))
        off += n * blk[-1] * hw * hw
    L["fc_off"] = [off, off + n * hidden]
    off += 2 * n * hidden
    L["drop_off"] = [off, off + n * hidden]
    off += 2 * n * hidden
    L["end"] = off
    return L


def read_arena(acts, n, images, lib=None):
    """float64 CPU copies of the chosen images' activations from the arena `acts` (flat fp32, as _VGGFeatures returns it):
    {"conv": 13 post-ReLU conv outputs [k][C][H][W], "pool": 5 pool outputs, "fc": fc1 / fc2 ReLU outputs [k][4096],
    "drop": their dropout outputs} with k = len(images).  With `lib` (umpr_amd._lib.lib()) the layout is checked against
    the library's own: pool5 offset equal, end of the dropout regions inside umpr_vgg16_act_bytes."""
    L = arena_layout(n)
    if lib is not None:
        assert L["pool_off"][4] * 4 == lib.size("umpr_vgg16_pool5_offset", n), "arena layout: pool5 offset differs from the library's"
        assert L["end"] * 4 <= lib.size("umpr_vgg16_act_bytes", n), "arena layout runs past umpr_vgg16_act_bytes"
    assert acts.dtype == torch.float32 and acts.numel() >= L["end"], (acts.dtype, acts.numel(), L["end"])
    idx = torch.as_tensor(list(images), dtype=torch.long, device=acts.device)

    def region(off, shape):
        numel = 1
        for s in shape:
            numel *= s
        return acts[off:off + n * numel].view(n, *shape).index_select(0, idx).double().cpu()

    return {"conv": [region(o, s) for o, s in zip(L["conv_off"], L["conv_shape"])],
            "pool": [region(o, s) for o, s in zip(L["pool_off"], L["pool_shape"])],
            "fc": [region(o, (VGG16_HIDDEN,)) for o in L["fc_off"]],
            "drop": [region(o, (VGG16_HIDDEN,)) for o in L["drop_off"]]}


def pool_argmax(y):
    """(index 0..3 into WINDOW_ORDER, maximum) of every 2x2 window of y [k][C][H][W]: the FIRST maximum in window order,
    i.e. a later element takes over only if strictly greater (torch's tie rule and the HIP kernels')."""
    k, C, H, W = y.shape
    win = y.reshape(k, C, H // 2, 2, W // 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(k, C, H // 2, W // 2, 4)
    m = win[..., 0].clone()
    arg = torch.zeros(m.shape, dtype=torch.long)
    for j in (1, 2, 3):
        gt = win[..., j] > m
        m = torch.where(gt, win[..., j], m)
        arg[gt] = j
    return arg, m


def pool_backward(y, g, move=None):
    """Gradient w.r.t. the pre-activation of the conv whose post-ReLU output y feeds a 2x2 max-pool, from the gradient g
    w.r.t. the pool output: g goes to the window's first maximum, and nowhere if that maximum is not > 0 (the ReLU).
    `move` = ((img, c, yo, xo), j) routes that one window to element j instead (sensitivity tests only)."""
    arg, m = pool_argmax(y)
    if move is not None:
        arg[move[0]] = move[1]
    gm = torch.where(m > 0, g, torch.zeros((), dtype=g.dtype))
    k, C, Ho, Wo = g.shape
    out = torch.zeros(k, C, Ho, Wo, 4, dtype=g.dtype)
    out.scatter_(-1, arg.unsqueeze(-1), gm.unsqueeze(-1))
    return out.reshape(k, C, Ho, Wo, 2, 2).permute(0, 1, 2, 4, 3, 5).reshape(k, C, 2 * Ho, 2 * Wo)


def features_backward(images, convs, pools, conv_params, d_pool, block_sizes, move=None, dtype=torch.float64, d_pools=None):
    """Backward of conv3x3(pad 1)+ReLU blocks, each closed by a 2x2 max-pool, with every decision taken from the given
    activations.  images [k][C0][H][W]; convs: post-ReLU conv outputs; pools: pool outputs; conv_params: [w0, b0, w1, b1,
    ...]; d_pool: gradient w.r.t. the last pool output; block_sizes: convolutions per block.  `move` = (block, window
    index, element) re-routes one pool window (see pool_backward).  Returns [dw0, db0, dw1, db1, ...] in `dtype`; a dict
    `d_pools` receives the gradient w.r.t. every pool output, keyed by block."""
    cv = lambda t: t.detach().to("cpu", dtype)   # noqa: E731
    assert len(convs) == sum(block_sizes) and len(pools) == len(block_sizes) and len(conv_params) == 2 * len(convs)
    grads = [None] * len(conv_params)
    g = cv(d_pool)
    ci = len(convs) - 1
    for b in reversed(range(len(block_sizes))):
        if d_pools is not None:
            d_pools[b] = g
        g = pool_backward(cv(convs[ci]), g, move[1:] if move is not None and move[0] == b else None)
        for j in reversed(range(block_sizes[b])):
            xin = cv(images) if ci == 0 else cv(pools[b - 1]) if j == 0 else cv(convs[ci - 1])
            w = cv(conv_params[2 * ci])
            grads[2 * ci] = conv2d_weight(xin, w.shape, g, padding=1)
            grads[2 * ci + 1] = g.sum((0, 2, 3))
            if ci == 0:
                break
            g = conv2d_input(xin.shape, w, g, padding=1)
            if j > 0:                   # input is a conv output: its ReLU; a pool input is masked by the pool backward
                g = g * (xin > 0)
            ci -= 1
    return grads


def classifier_backward(pool5, fc, drop, fc_params, d_out, masks=None, p=0.5, dtype=torch.float64, device="cpu"):
    """Backward of Linear-ReLU-Dropout-Linear-ReLU-Dropout-Linear.  pool5 [k][F]; fc: the two ReLU outputs; drop: their
    dropout outputs (read only with masks); fc_params [W1, b1, W2, b2, W3, b3]; masks: keep-masks [2][k][hidden] (0/1) or
    None when no dropout ran.  Returns ([dW1, db1, dW2, db2, dW3, db3], gradient w.r.t. pool5), computed on `device`."""
    cv = lambda t: t.detach().to(device, dtype)   # noqa: E731
    grads = [None] * 6
    g = cv(d_out)
    for j in (2, 1, 0):
        if j < 2:
            if masks is not None:
                g = g * cv(masks[j]) / (1.0 - p)
            g = g * (cv(fc[j]) > 0)
        xin = cv(pool5) if j == 0 else cv(drop[j - 1]) if masks is not None else cv(fc[j - 1])
        grads[2 * j] = g.t() @ xin
        grads[2 * j + 1] = g.sum(0)
        g = g @ cv(fc_params[2 * j])
    return grads, g


def vgg16_backward(images, acts, params, d_out, masks=None, move=None, dtype=torch.float64, d_pools=None):
    """The 32 VGG16 parameter gradients (VGG16.param_list() order) for the images whose activations `acts` holds
    (read_arena), from the gradient d_out [k][1000] at the network's output, or - d_out of shape [k][25088] - at pool5
    (the classifier gradients are then None).  masks: the dropout keep-masks of those images [2][k][4096], None when the
    classifier ran without dropout."""
    if d_out.shape[-1] == 512 * 7 * 7:
        cls, d_pool5 = [None] * 6, d_out
    else:
        cls, d_pool5 = classifier_backward(acts["pool"][4].flatten(1), acts["fc"], acts["drop"], params[26:], d_out, masks,
                                           dtype=dtype)
    feats = features_backward(images, acts["conv"], acts["pool"], params[:26], d_pool5.reshape(-1, 512, 7, 7),
                              [len(b) for b in VGG16_BLOCKS], move, dtype, d_pools)
    return feats + cls
