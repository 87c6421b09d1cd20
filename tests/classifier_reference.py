"""Float64 reference of the VGG16 classifier (test helper, not a test module; on the CPU unless a caller names a device).

The classifier is Linear-ReLU-Dropout-Linear-ReLU-Dropout-Linear (25088 -> 4096 -> 4096 -> 1000).  Its decisions - which ReLU
outputs are positive, which dropout units were kept - are stored in the activation arena (fc and drop regions) and in the mask
bytes, so the references here never take a decision of their own:
  * layer_forward computes ONE layer from that layer's own HIP input (pool5; fc[j-1] in eval; drop[j-1] when dropout ran), so a
    ReLU sign that lands differently upstream cannot leak into the next layer's verdict;
  * the backward is vgg_decisions.classifier_backward on the arena's fc / drop regions and the masks the call used;
  * both run in float64 (the reference; the GPU tests run it on the device, where the 103 M-element dW1 is then compared as
    well) and in float32 on the CPU (the yardstick), and a HIP tensor is held to K x the distance the yardstick has from the
    reference (coattn_decisions.gate: K = 4, never above 14, floor 2^-22).
The bf16 forms round the operands of every product to bf16 (as _QLinear of tests/test_gpu_bf16.py does) and multiply in float64.
tests/test_classifier_reference.py checks all of it against float64 autograd on the CPU at reduced widths;
tests/test_gpu_classifier.py and tests/test_gpu_bf16.py use it on the GPU at the ABI's widths.
"""
from types import SimpleNamespace

import numpy as np
import torch

import vgg_decisions as V
from coattn_decisions import FLOOR, K_MAX, K_START, distances, gate   # noqa: F401  (shared, not copied)

DIMS = ((25088, 4096), (4096, 4096), (4096, 1000))      # (in, out) of the three layers: fixed by the ABI
P_DROP = 0.5
FWD_NAMES = ("fc1", "fc2", "out")
GRAD_NAMES = ("dW1", "db1", "dW2", "db2", "dW3", "db3")
GOLDEN64 = 0x9E3779B97F4A7C15
MASK64 = (1 << 64) - 1

K = K_START
# Per-tensor gate factors above K_START: ceil(1.25 x worst measured ratio), never above K_MAX, with the measurement and the
# summation structure that explains it in profiles/r06_a_classifier_gemm_gates.txt.  Empty: nothing needed a raise.
K_OF = {}


def k_of(name):
    """the gate factor of one tensor: K unless K_OF raises it (never above K_MAX)"""
    k = K_OF.get(name, K)
    assert k <= K_MAX, (name, k)
    return k


# ------------------------------------------------------------------------------------------------------- cases
# Row counts n: the smallest at which each mechanism of fc_small.hip / api.hip can fail (the widths are fixed, n is the only size)
#   1, 2         one row; one pair of fc_dw's batch loop
#   31, 32, 33   TM 1 -> 2 row tiles; an odd pair tail; a second tile holding one row
#   63, 64, 65   TM 2 -> 4
#   127, 128     the last size fc_small takes
#   129, 160     the generic GEMM: dW has K = n = 129 = 8 stages + 1, the 128-row M tile has one row in use
ROWS = (1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160)
GEN_SEEDS = {"gen0": 0x5EED0000C1A55, "gen1": 0x5EED0000C1A56}      # s and s + 1
# (n, mode, kind).  mode: eval (train = 0, use_masks = 0) | masks (use_masks = 1, injected Bernoulli(0.5) bytes) | gen0 / gen1
# (train = 1, use_masks = 0, masks generated from GEN_SEEDS).  kind: dense (d_out = randn) | row32 (d_out zero except row 32) |
# zero (d_out all zero) | ordinary (dense, and no special pool5 row: with the last row all zero the odd tail row of fc_dw* adds
# nothing to dW1 and a dropped tail shows in dW2 / dW3 only - here it shows in dW1 as well).
CASES = [(n, "eval", "dense") for n in ROWS] + [(n, "masks", "dense") for n in (1, 33, 64, 127, 129)] + \
        [(n, m, "dense") for n in (33, 64) for m in ("gen0", "gen1")] + \
        [(33, "eval", "row32"), (33, "masks", "row32"), (5, "eval", "zero"), (33, "eval", "ordinary"), (127, "masks", "ordinary")]
case_id = lambda c: "-".join(map(str, c))       # noqa: E731

_WEIGHTS = {}


def weights32(dims=DIMS, seed=11):
    """The float32 parameters [W1, b1, W2, b2, W3, b3] of test_classifier_bf16_through_c_abi's distribution: W = randn *
    (2 / fin)^0.5, b = 0.1 randn.  Built once per process and shared; nothing modifies them."""
    key = (tuple(dims), seed)
    if key not in _WEIGHTS:
        g = torch.Generator().manual_seed(seed)
        p32 = []
        for fin, fout in dims:
            p32 += [torch.randn(fout, fin, generator=g) * (2.0 / fin) ** 0.5, torch.randn(fout, generator=g) * 0.1]
        _WEIGHTS[key] = [p32, None]
    return _WEIGHTS[key][0]


_DEV_WEIGHTS = {}


def device_weights(dev):
    """weights32() on the device `dev`: one copy per process, shared by every GPU test module that runs the classifier"""
    if dev not in _DEV_WEIGHTS:
        _DEV_WEIGHTS[dev] = [p.to(dev) for p in weights32()]
    return _DEV_WEIGHTS[dev]


def weights(dims=DIMS, seed=11):
    """(weights32, their float64 copies), both cached"""
    p32 = weights32(dims, seed)
    entry = _WEIGHTS[(tuple(dims), seed)]
    if entry[1] is None:
        entry[1] = [p.double() for p in p32]
    return p32, entry[1]


def make_case(n, mode, kind, dims=DIMS, seed=None):
    """The seeded inputs of one case: pool5 = relu(randn) (about half zeros, as a pooled feature map is; with n >= 3 the last row
    all zero and the second-last constant; rows 0 and 1 in kind row32), d_out as `kind` says, injected masks in mode `masks`, the
    seed in modes gen*."""
    g = torch.Generator().manual_seed(7000 + 13 * n + len(mode) + 3 * len(kind) if seed is None else seed)
    hidden = dims[0][1]
    pool5 = torch.relu(torch.randn(n, dims[0][0], generator=g))
    if n >= 3 and kind != "ordinary":   # kind row32: rows 0 and 1 instead, so that the only contributing row is an ordinary one
        pool5[0 if kind == "row32" else n - 1] = 0
        pool5[1 if kind == "row32" else n - 2] = 0.75
    d_out = torch.randn(n, dims[2][1], generator=g)
    if kind == "row32":
        assert n == 33
        d_out[:32] = 0
    elif kind == "zero":
        d_out.zero_()
    else:
        assert kind in ("dense", "ordinary"), kind
    masks = (torch.rand(2, n, hidden, generator=g) < 0.5).to(torch.uint8) if mode == "masks" else None
    return SimpleNamespace(n=n, mode=mode, kind=kind, tag=f"cls n{n} {mode} {kind}", pool5=pool5, d_out=d_out, masks=masks,
                           train=int(mode.startswith("gen")), use_masks=int(mode == "masks"), seed=GEN_SEEDS.get(mode, 0),
                           dropout=mode != "eval")


# ------------------------------------------------------------------------------------------------------- forward
def layer_forward(x, W, b, relu, dtype=torch.float64, device="cpu"):
    """One layer from its own input: act(x W^T + b) in `dtype` (float64: the reference; float32 on the CPU: the yardstick)."""
    cv = lambda t: t.detach().to(device, dtype)          # noqa: E731
    y = cv(x) @ cv(W).t() + cv(b)
    return torch.relu(y) if relu else y


def bf16_round(x):
    """x rounded to bf16 (round to nearest even), as float32"""
    return x.detach().float().bfloat16().float()


def layer_forward_bf16(x, W, b, relu, device="cpu"):
    """The same with both operands of the product rounded to bf16, multiplied in float64; the bias stays unrounded."""
    y = bf16_round(x).to(device).double() @ bf16_round(W).to(device).double().t() + b.detach().to(device).double()
    return torch.relu(y) if relu else y


def dropout_forward(fc, mask, p=P_DROP):
    """where(mask, fc / (1 - p), 0) in fc's dtype: at p = 0.5 the scale is a power of two, the product exact"""
    return torch.where(mask.bool(), fc * (1.0 / (1.0 - p)), torch.zeros((), dtype=fc.dtype, device=fc.device))


def layer_inputs(pool5, fc, drop, dropout):
    """the HIP input of each of the three layers: pool5; fc[j-1] in eval; drop[j-1] when dropout ran"""
    return [pool5] + [drop[j] if dropout else fc[j] for j in (0, 1)]


def classifier_forward(pool5, params, masks=None, dtype=torch.float64):
    """The whole chain in `dtype`, every layer fed by the previous one: (fc [2], drop [2] or None, out)."""
    fc, drop, x = [], [], pool5
    for j in range(3):
        x = layer_forward(x, params[2 * j], params[2 * j + 1], j < 2, dtype)
        if j < 2:
            fc.append(x)
            if masks is not None:
                x = dropout_forward(x, masks[j])
                drop.append(x)
    return fc, (drop if masks is not None else None), x


def classifier_backward(pool5, fc, drop, params, d_out, masks=None, dtype=torch.float64, device="cpu"):
    """vgg_decisions.classifier_backward: ([dW1, db1, dW2, db2, dW3, db3], d_pool5) in `dtype`, decisions from fc / masks"""
    return V.classifier_backward(pool5, fc, drop, params, d_out, masks, p=P_DROP, dtype=dtype, device=device)


def classifier_backward_bf16(pool5, fc, drop, params, d_out, masks=None, device="cpu"):
    """The backward with the operands of every product rounded to bf16 (the gradient at a layer's output, the layer's input, the
    weights) and multiplied in float64; bias gradients, the dropout scale and the ReLU mask stay unrounded.  Decisions and layer
    inputs from fc / drop / masks, as in classifier_backward."""
    cv = lambda t: t.detach().to(device).double()     # noqa: E731
    q = lambda t: bf16_round(t).to(device).double()   # noqa: E731
    grads = [None] * 6
    g = cv(d_out)
    for j in (2, 1, 0):
        if j < 2:
            if masks is not None:
                g = g * cv(masks[j]) / (1.0 - P_DROP)
            g = g * (cv(fc[j]) > 0)
        xin = pool5 if j == 0 else drop[j - 1] if masks is not None else fc[j - 1]
        gq = q(g.float())                        # the kernels hold g in fp32 before rounding it
        grads[2 * j] = gq.t() @ q(xin)
        grads[2 * j + 1] = g.float().double().sum(0)
        g = (gq @ q(params[2 * j])).float().double()
    return grads, g


# ------------------------------------------------------------------------------------------------------- generated masks
def _hash32(x):
    x = x.copy()
    x ^= x >> np.uint32(16)
    x *= np.uint32(0x7feb352d)
    x ^= x >> np.uint32(15)
    x *= np.uint32(0x846ca68b)
    x ^= x >> np.uint32(16)
    return x


def generated_masks(seed, n, hidden=DIMS[0][1]):
    """The keep-masks [2][n][hidden] (uint8) a train = 1, use_masks = 0 forward generates: a pure function of (seed, layer, element
    index) - layer j uses seed + (j + 1) * 0x9E3779B97F4A7C15 (mod 2^64), element i = row * hidden + column goes through the
    counter hash of dropout_fwd_kernel (text_ops.hip), kept when the hashed 24-bit uniform is >= 0.5."""
    out = []
    for j in range(2):
        s = (seed + GOLDEN64 * (j + 1)) & MASK64
        i = np.arange(n * hidden, dtype=np.uint64)
        lo, hi = (i & np.uint64(0xFFFFFFFF)).astype(np.uint32), (i >> np.uint64(32)).astype(np.uint32)
        with np.errstate(over="ignore"):
            h = _hash32(lo * np.uint32(0x9E3779B9) + np.uint32(s & 0xFFFFFFFF)) ^ \
                _hash32(hi + np.uint32(s >> 32) + np.uint32(0x85ebca6b))
            u24 = _hash32(h) >> np.uint32(8)
        out.append(torch.from_numpy((u24 >= np.uint32(1 << 23)).astype(np.uint8)).reshape(n, hidden))
    return torch.stack(out)


def mask_conditions(m, other=None):
    """The conditions generated masks m [2][n][hidden] must meet, as a list of failures (empty: all met).  Every byte 0 or 1; keep
    fraction of each layer within 5 sigma of 0.5 (2.5 / sqrt(n hidden)); each row's within 5 sigma (2.5 / sqrt(hidden)); no two rows
    equal, over both layers; the two layers agree on a fraction within 5 sigma of 0.5, and so does each layer with `other` (the
    masks of the next seed)."""
    m = m.cpu()
    _, n, hidden = m.shape
    bad = []
    if not bool((m <= 1).all()):
        bad.append(f"{int((m > 1).sum())} bytes are neither 0 or 1")
        return bad
    f = m.float()
    lim, lim_row = 2.5 / (n * hidden) ** 0.5, 2.5 / hidden ** 0.5
    for j in range(2):
        keep = float(f[j].mean())
        if abs(keep - 0.5) > lim:
            bad.append(f"layer {j}: keep fraction {keep:.5f} outside 0.5 +- {lim:.5f}")
        rows = f[j].mean(1)
        if float((rows - 0.5).abs().max()) > lim_row:
            bad.append(f"layer {j}: a row's keep fraction {float(rows[(rows - 0.5).abs().argmax()]):.4f} outside 0.5 +- {lim_row:.4f}")
    if torch.unique(m.reshape(2 * n, hidden), dim=0).shape[0] != 2 * n:
        bad.append("two rows are equal")
    pairs = [("layers 0 and 1", m[0], m[1])]
    if other is not None:
        pairs += [(f"layer {j} of the two seeds", m[j], other.cpu()[j]) for j in range(2)]
    for what, a, b in pairs:
        agree = float((a == b).float().mean())
        if abs(agree - 0.5) > lim:
            bad.append(f"{what} agree on {agree:.5f}, outside 0.5 +- {lim:.5f}")
    return bad
