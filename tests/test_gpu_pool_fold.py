"""Pool backward folded into its readers (pools 2-5 of the fp32 VGG16 backward, UMPR_POOL_FOLD): the Winograd gradient readers get
the conv output and the POOLED gradient and form the un-pooled gradient themselves.  Nothing may change: every comparison of a
folded run with the un-folded kernels is BITWISE.

Whole backward: umpr_vgg16_features_fwd + umpr_vgg16_features_bwd through the C ABI at n = 1, 2, 3 images (n = 3: the slot
rotation wraps with an odd tile count, T = 3 * 49 tiles at 28x28 is not a multiple of the 128-wide GEMM column).  The switch is read
when the library loads, so the UMPR_POOL_FOLD=0 run is a job of tools/run_gpu_children.py: this file's
test_whole_backward_runs in a child process, which leaves the sha256 of the 26 gradients beside the jobs' logs.  Images: seeded
noise, an all-zero image (every window ties and no maximum is > 0), a constant positive image (every window ties at a positive
value: the first-maximum rule decides) and an image with a constant border.

Per layer: umpr_debug_wino_pool_fold runs the Winograd readers on shapes the plan would give to other kernels - the one debug entry
point this needs, declared in include/umpr_hip.h and in the signature table of umpr_amd/_lib.py (tests/test_cabi_symbols.py pins
header <-> table <-> exports).  fold = 1 against fold = 0 (umpr_maxpool2_bwd_relu first, the same kernels on its output): bitwise.
fold = 1 against umpr_maxpool2_bwd_relu + umpr_conv3x3_bwd_data / umpr_conv3x3_bwd_weight, which run whatever the plan names for
the shape (the generic / direct kernels here): within TOL of the reference's largest magnitude.  TOL = 2e-5: the 4x4 tile's fp32
result is at most 1.2e-6 of max|y| from float64 at 4608 reduction terms (winograd.hip, tools/wino_points.py), the direct kernels'
2e-7; 2e-5 leaves an order of magnitude over their sum and is three orders of magnitude below what one mis-routed window does (one
element of dy, ~max|dy|, times one filter tap, ~0.1 of the largest output).
Shapes (Cin, Cout, H): (32, 32, 8) one tile row of two 4x4 tiles; (32, 160, 12) Cout not a multiple of 128; (64, 64, 14) edge tiles
in the data gradient and an odd tile row (wino_dy_kernel) in the weight gradient; (33, 32, 16) a channel tail; (32, 32, 24) at
N = 3 is 108 tiles in rows of 6, so a wave of 64 tiles ends inside a tile row: the data gradient's input transform takes a tile's
outer columns from the neighbour lanes, and lanes 0 and 63 load them themselves.  N = 1 and 3.
"""
import hashlib
import json
import os

import pytest
import torch

from conftest import CHILDREN, child_result
from test_gpu_parity import L, dev, st   # noqa: F401  (fixtures: the library, the device)

pytestmark = pytest.mark.gpu

CHILD_DIGESTS = os.path.join(os.path.dirname(CHILDREN["rc"]), "pool_fold0_digests.json")   # beside the jobs' logs
CFG = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
       (512, 512), (512, 512), (512, 512))
TOL = 2e-5
SHAPES = [(32, 32, 8), (32, 160, 12), (64, 64, 14), (33, 32, 16), (32, 32, 24)]


def _image_pool():
    g = torch.Generator().manual_seed(4321)
    noise = torch.randn(3, 224, 224, generator=g)
    border = torch.randn(3, 224, 224, generator=g)
    border[:, :24, :] = 0.75; border[:, -24:, :] = 0.75; border[:, :, :24] = 0.75; border[:, :, -24:] = 0.75
    return {"noise": noise, "zero": torch.zeros(3, 224, 224), "const": torch.full((3, 224, 224), 0.5), "border": border}


BATCHES = {1: ("border",), 2: ("zero", "const"), 3: ("noise", "zero", "const")}


def _whole_backward(L, dev, n):
    """(sha256 of each of the 26 gradients, all finite?) of one forward + backward"""
    from umpr_amd.model import _ptr_array
    g = torch.Generator().manual_seed(99 + n)
    params = []
    for cin, cout in CFG:   # He initialisation keeps the activations' scale through the 13 layers
        params.append((torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev))
        params.append((torch.randn(cout, generator=g) * 0.01).to(dev))
    pool = _image_pool()
    images = torch.stack([pool[k] for k in BATCHES[n]]).to(dev)
    d_pool5 = torch.randn(n, 25088, generator=g).to(dev)
    grads = [torch.full_like(p, float("nan")) for p in params]
    keep_p, parr = _ptr_array(params + params[:6])
    keep_g, garr = _ptr_array(grads + grads[:6])
    acts = torch.empty(L.size("umpr_vgg16_act_bytes", n) // 4, device=dev)
    wf = torch.empty(L.size("umpr_vgg16_fwd_ws_bytes", n) // 4, device=dev)
    wb = torch.empty(L.size("umpr_vgg16_features_bwd_ws_bytes", n) // 4, device=dev)
    L.call("umpr_vgg16_features_fwd", images, parr, n, acts, wf, wf.numel() * 4, st())
    L.call("umpr_vgg16_features_bwd", images, parr, n, acts, d_pool5, garr, wb, wb.numel() * 4, st())
    torch.cuda.synchronize()
    return [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in grads], all(bool(torch.isfinite(t).all()) for t in grads)


@pytest.fixture(scope="module")
def whole(L, dev):
    out = {}
    for n in BATCHES:
        out[str(n)] = _whole_backward(L, dev, n)
        torch.cuda.empty_cache()
    if os.environ.get("UMPR_POOL_FOLD") == "0":   # the child job: leave the digests for the parent's comparison
        os.makedirs(os.path.dirname(CHILD_DIGESTS), exist_ok=True)
        with open(CHILD_DIGESTS, "w") as f:
            json.dump({k: v[0] for k, v in out.items()}, f)
    return out


@pytest.mark.parametrize("n", sorted(BATCHES))
def test_whole_backward_runs(whole, n):
    digests, finite = whole[str(n)]
    assert len(digests) == 26 and finite


def test_whole_backward_bitwise_equal_to_the_unfolded_kernels(whole):
    assert os.environ.get("UMPR_POOL_FOLD") is None, "run this comparison with UMPR_POOL_FOLD unset"
    rc, out = child_result("pool_fold0_check")
    assert rc == 0, out[-3000:]
    with open(CHILD_DIGESTS) as f:
        child = json.load(f)
    assert sorted(child) == sorted(whole)
    for key in sorted(whole):
        differ = [i for i, (a, b) in enumerate(zip(whole[key][0], child[key])) if a != b]
        print(f"n={key}: gradients that differ from UMPR_POOL_FOLD=0: {differ}")
        assert len(child[key]) == 26 and not differ, f"n={key}: gradients {differ} differ from the UMPR_POOL_FOLD=0 run"


def _layer_inputs(dev, N, Cin, Cout, H):
    g = torch.Generator().manual_seed(N * 1000 + Cin * 7 + Cout * 3 + H)
    # the layer's output on a grid of 0.5 after the ReLU: about half of the windows tie (many at zero), the rest have one maximum
    y = torch.relu(torch.round(torch.randn(N, Cout, H, H, generator=g) * 2.0) / 2.0)
    y[0, 0] = 0.0        # a plane of all-zero windows
    y[0, 1] = 0.5        # a plane of windows that tie at a positive value
    gp = torch.randn(N, Cout, H // 2, H // 2, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    x = torch.randn(N, Cin, H, H, generator=g)
    return y.to(dev), gp.to(dev), w.to(dev), x.to(dev)


def _debug(L, dev, t, N, Cin, Cout, H, f4, fold, want_dx, want_dw):
    y, gp, w, x = t
    nan = float("nan")
    unp = torch.full((N, Cout, H, H), nan, device=dev)
    dx = torch.full((N, Cin, H, H), nan, device=dev) if want_dx else None
    dw = torch.full((Cout, Cin, 3, 3), nan, device=dev) if want_dw else None
    db = torch.full((Cout,), nan, device=dev) if want_dw else None
    ws = torch.full((16 << 20,), nan, device=dev)
    L.call("umpr_debug_wino_pool_fold", y, gp, w, x, unp, dx, dw, db, N, Cin, Cout, H, H, f4, fold, ws, ws.numel() * 4, st())
    torch.cuda.synchronize()
    return dx, dw, db


@pytest.fixture(scope="module")
def reference(L, dev):
    """umpr_maxpool2_bwd_relu + umpr_conv3x3_bwd_data / umpr_conv3x3_bwd_weight per (shape, N), computed once"""
    out = {}
    for Cin, Cout, H in SHAPES:
        for N in (1, 3):
            y, gp, w, x = t = _layer_inputs(dev, N, Cin, Cout, H)
            unp = torch.empty_like(y)
            L.call("umpr_maxpool2_bwd_relu", y, gp, unp, N * Cout, H, H, st())
            wt = torch.empty(L.size("umpr_conv3x3_pack_bytes", N, Cin, Cout, H, H) // 4 + 1, device=dev)
            dx = torch.empty(N, Cin, H, H, device=dev)
            L.call("umpr_conv3x3_bwd_data", unp, w, None, dx, N, Cin, H, H, Cout, wt, wt.numel() * 4, st())
            ws = torch.empty(L.size("umpr_conv3x3_bwd_weight_ws_bytes", N, Cin, Cout, H, H) // 4 + 1, device=dev)
            dw, db = torch.empty(Cout, Cin, 3, 3, device=dev), torch.empty(Cout, device=dev)
            L.call("umpr_conv3x3_bwd_weight", unp, x, dw, db, N, Cin, H, H, Cout, ws, ws.numel() * 4, st())
            torch.cuda.synchronize()
            out[(Cin, Cout, H, N)] = (t, dx, dw, db)
    return out


def _close(name, got, ref):
    err = float((got - ref).abs().max())
    scale = float(ref.abs().max())
    print(f"{name}: max err {err:.3e}, largest reference magnitude {scale:.3e}, ratio {err / scale:.3e} (bound {TOL:.0e})")
    assert bool(torch.isfinite(got).all()) and err <= TOL * scale, (name, err, scale)


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("Cin,Cout,H", SHAPES)
def test_layer_data_gradient(L, dev, reference, Cin, Cout, H, N):
    t, ref_dx, _, _ = reference[(Cin, Cout, H, N)]
    folded = _debug(L, dev, t, N, Cin, Cout, H, 1, 1, True, False)[0]
    plain = _debug(L, dev, t, N, Cin, Cout, H, 1, 0, True, False)[0]
    assert torch.equal(folded.view(torch.int32), plain.view(torch.int32)), "the folded data gradient differs from the un-folded kernels"
    _close(f"dx {Cin}->{Cout} {H}x{H} N={N}", folded, ref_dx)


# a weight gradient on the 4x4 tile has no edge tiles (the plan never puts a 14x14 map there): 14x14 on the 2x2 tile only
WGRAD_CASES = [(Cin, Cout, H, f4) for Cin, Cout, H in SHAPES for f4 in (0, 1) if not (f4 and H % 4)]


@pytest.mark.parametrize("N", [1, 3])
@pytest.mark.parametrize("Cin,Cout,H,f4", WGRAD_CASES)
def test_layer_weight_gradient(L, dev, reference, Cin, Cout, H, f4, N):
    t, _, ref_dw, ref_db = reference[(Cin, Cout, H, N)]
    _, dw1, db1 = _debug(L, dev, t, N, Cin, Cout, H, f4, 1, False, True)
    _, dw0, db0 = _debug(L, dev, t, N, Cin, Cout, H, f4, 0, False, True)
    assert torch.equal(dw1.view(torch.int32), dw0.view(torch.int32)), "the folded weight gradient differs from the un-folded kernels"
    assert torch.equal(db1.view(torch.int32), db0.view(torch.int32)), "the folded bias gradient differs from the un-folded kernels"
    _close(f"dw {Cin}->{Cout} {H}x{H} N={N} f4={f4}", dw1, ref_dw)
    _close(f"db {Cin}->{Cout} {H}x{H} N={N} f4={f4}", db1, ref_db)
