"""The bf16 VGG16 feature stack (umpr_vgg16_bf16_features_fwd / _bwd) inside the network, through the C ABI as
_VGGFeaturesBF16 calls it, against the rounding-replaying float64 reference of tests/vgg_bf16_decisions.py.

Forward: every tensor of the bf16 activation arena is decoded with the Python CB8-PF index map; each conv output is held to
q(relu(conv64(q(its arena input), q(w)) + b)) - conv 0 (conv1_bf16_fwd_kernel) from the fp32 images - at the bounds of
test_vgg16_bf16_vs_rounded_operand_oracle (a), each pool to the exact maximum of its arena window, every element outside the
real pixels to exact zero (zero_guards_multi_kernel and the zero_guards = false form of every layer, on an arena that starts
as 0xFF bytes), pool5 to the decoded last pool.
Backward: all 26 gradients - the multi-layer weight packer, conv1_bf16_wgrad_kernel + wgrad1_reduce_kernel, the three-slot
gradient rotation and the weight-gradient side stream - against features_backward_bf16 on the decoded arena, at the
per-tensor gate REL_L2_BF16 / REL_MAX_BF16 (4x the measured distance between two correct implementations).  The workspace is
exactly the queried size with a canary behind it.  Every distance is logged to vgg_bf16_grad.log before anything is asserted.

Measured on the MI355X (n = 1 and 3, dense and sparse): the largest distance is dfeatures.0.bias at n = 1, sparse - relative L2
7.9e-3 against its bound 2.41e-2, max error / max 1.14e-2 against 2.82e-2; no tensor is above 0.33x of its relative-L2 bound or
0.41x of its max bound.  Forward: relative L2 1.0e-5 .. 7.3e-5 (bound 1e-4), 3e-6 .. 1.6e-4 of the
outputs one bf16 step away (bound 5e-4), no non-zero pad or guard element, pools and pool5 exact.
"""
import os
import time

import pytest
import torch
import torch.nn.functional as F

import vgg_bf16_decisions as B
from test_gpu_parity import LOG as PARITY_LOG

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "vgg_bf16_grad.log")          # beside the parity tests' log
SIZES = [len(b) for b in B.VGG16_BLOCKS]
CANARY = 1 << 16           # bytes / floats behind every buffer a call writes
FWD_REL_L2, FWD_ONE_STEP = 1e-4, 5e-4      # test_gpu_bf16.py: test_vgg16_bf16_vs_rounded_operand_oracle (a)


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


@pytest.fixture(scope="module")
def L():
    from umpr_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def poison_lds(L, dev):
    sink = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("umpr_debug_poison_lds", sink, st())
    yield


def _bytes(dev, nbytes):
    """(0xFF-filled buffer of nbytes, the 0xFF canary behind it)"""
    t = torch.full((nbytes + CANARY,), 0xFF, dtype=torch.uint8, device=dev)
    return t[:nbytes], t[nbytes:]


def _floats(dev, numel):
    """(NaN-filled fp32 buffer, the NaN canary behind it)"""
    t = torch.full((numel + CANARY,), float("nan"), device=dev)
    return t[:numel], t[numel:]


@pytest.fixture(scope="module", params=[1, 3], ids=["n1", "n3"])
def case(request, L, dev):
    """One HIP forward of n images (n = 1: random; n = 3: random, flat per channel, all zero) into an arena that starts as
    0xFF bytes, and the decoded arena.  Shared by the forward check and both backward cases; nothing in it is changed."""
    from umpr_amd.model import _ptr_array
    n = request.param
    ps = [p.to(dev) for p in B.conv_params(700 + n)]
    x = B.images(710 + n, n).to(dev)
    acts, acts_canary = _bytes(dev, L.size("umpr_vgg16_bf16_act_bytes", n))
    wsb = L.size("umpr_vgg16_bf16_fwd_ws_bytes", n)
    ws, ws_canary = _bytes(dev, wsb)
    pool5, pool5_canary = _floats(dev, n * 25088)
    keep, parr = _ptr_array(ps + ps[:6])                      # the 32-pointer table; the classifier slots are not read
    t0 = time.time()
    L.call("umpr_vgg16_bf16_features_fwd", x, parr, n, acts, pool5, ws, wsb, st())
    torch.cuda.synchronize()
    log(f"== n={n}: HIP forward {time.time() - t0:.2f} s")
    t0 = time.time()
    arena = B.read_arena_bf16(acts, n, range(n), L)
    log(f"n={n}: arena decoded in {time.time() - t0:.1f} s")
    c = {"n": n, "ps": ps, "ps_cpu": [p.cpu() for p in ps], "x": x, "x_cpu": x.cpu(), "acts": acts,
         "pool5": pool5.view(n, 25088), "arena": arena, "parr": parr, "keep": keep,
         "canaries": {"arena": acts_canary, "forward workspace": ws_canary, "pool5": pool5_canary}}
    yield c
    c.clear()


def test_forward_arena_layer_by_layer(case, L):
    n, arena = case["n"], case["arena"]
    tag = f"n={n} fwd"
    bad = []
    for name, canary in case["canaries"].items():
        intact = bool((canary == 0xFF).all()) if canary.dtype == torch.uint8 else bool(torch.isnan(canary).all())
        if not intact:
            bad.append(f"{name}: canary written")
    # every element of the 18 tensors that is not a real pixel of a real channel: exactly zero
    for name, buf, (c, h, w) in B.arena_tensors(case["acts"], n, L):
        nz = B.nonzero_outside(buf, n, c, h, w)
        log(f"{tag} {name}: {nz} non-zero elements outside the real pixels")
        if nz:
            bad.append(f"{name}: {nz} non-zero pad / guard elements")
    t0 = time.time()
    ci = 0
    for b, nb in enumerate(SIZES):
        for j in range(nb):
            xin = B.q(case["x_cpu"]) if ci == 0 else arena["pool"][b - 1] if j == 0 else arena["conv"][ci - 1]
            w, bias = B.q(case["ps_cpu"][2 * ci]), case["ps_cpu"][2 * ci + 1].double()
            ref = B.q(torch.relu(F.conv2d(xin, w, bias, padding=1)))
            hip = arena["conv"][ci]
            finite = bool(torch.isfinite(hip).all())
            e = float((hip - ref).norm() / ref.norm())
            diff = hip != ref
            frac = float(diff.double().mean())
            log(f"{tag} conv{ci}: relL2 {e:.2e}, outputs one bf16 step away {frac:.1e}, max|err| {float((hip - ref).abs().max()):.2e}")
            if not (finite and e <= FWD_REL_L2 and frac <= FWD_ONE_STEP):
                bad.append(f"conv{ci}: relL2 {e:.2e} differing {frac:.1e} finite {finite}")
            ci += 1
        n_pool = int((F.max_pool2d(arena["conv"][ci - 1], 2, 2) != arena["pool"][b]).sum())
        log(f"{tag} pool{b}: {n_pool} outputs differ from the maximum of their arena window")
        if n_pool:
            bad.append(f"pool{b}: {n_pool} outputs differ from the maximum of their window")
    log(f"{tag}: float64 teacher-forced forward of {n} images {time.time() - t0:.1f} s")
    n5 = int((case["pool5"].cpu().double() != arena["pool"][4].flatten(1)).sum())
    log(f"{tag} pool5 fp32: {n5} values differ from the decoded last pool in flatten order")
    if n5:
        bad.append(f"pool5: {n5} values differ")
    assert not bad, bad


@pytest.mark.parametrize("upstream", ["dense", "sparse"])
def test_backward_vs_rounding_replaying_reference(case, L, dev, upstream):
    """All 26 feature gradients of umpr_vgg16_bf16_features_bwd against features_backward_bf16(acc_dtype=float64) on the
    decoded arena; dense: randn at pool5, sparse: 32 non-zero entries.  Workspace of exactly umpr_vgg16_bf16_bwd_ws_bytes,
    0xFF-filled, with a canary behind it; gradient buffers NaN-filled with a canary each."""
    from umpr_amd.model import _ptr_array
    n, arena = case["n"], case["arena"]
    tag = f"n={n} {upstream}"
    g = torch.Generator().manual_seed(720 + n)
    d = torch.randn(n, 25088, generator=g) if upstream == "dense" else B.sparse_upstream((n, 25088), 730 + n)
    grads, canaries = zip(*[_floats(dev, p.numel()) for p in case["ps"]])
    wsb = L.size("umpr_vgg16_bf16_bwd_ws_bytes", n)
    ws, ws_canary = _bytes(dev, wsb)
    keep_g, garr = _ptr_array(list(grads) + list(grads[:6]))
    arena_before = case["acts"].clone()
    d_dev = d.to(dev)
    t0 = time.time()
    L.call("umpr_vgg16_bf16_features_bwd", case["x"], case["parr"], n, case["acts"], d_dev, garr, ws, wsb, st())
    torch.cuda.synchronize()
    log(f"== {tag}: HIP backward {time.time() - t0:.2f} s")
    t0 = time.time()
    ref = B.features_backward_bf16(case["x_cpu"], arena["conv"], arena["pool"], case["ps_cpu"], d.view(n, 512, 7, 7), SIZES)
    log(f"{tag}: float64 reference backward of {n} images {time.time() - t0:.1f} s")
    outside = []
    for name, gr, (l2, mx), r in zip(B.VGG16_PARAM_NAMES, grads, B.distances(grads, ref), ref):
        finite = bool(torch.isfinite(gr).all())
        b_l2, b_max = B.gate(name)
        log(f"{tag} d{name}: rel_l2={l2:.3e} (bound {b_l2:.2e}) max_err/max={mx:.3e} (bound {b_max:.2e}) "
            f"ref_max={float(r.abs().max()):.3e} finite={finite}")
        if not (finite and l2 <= b_l2 and mx <= b_max):               # every tensor is logged before the test fails
            outside.append((name, l2, mx, finite))
    written = [f"d{name}" for name, cn in zip(B.VGG16_PARAM_NAMES, canaries) if not bool(torch.isnan(cn).all())]
    if not bool((ws_canary == 0xFF).all()):
        written.append("backward workspace")
    if not torch.equal(arena_before, case["acts"]):
        written.append("the activation arena itself")
    log(f"{tag}: written outside their bounds: {written or 'nothing'}")
    assert not outside, outside
    assert not written, written
