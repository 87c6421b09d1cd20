"""The fp32 3x3 convolution entry points run what umpr_conv3x3_plan decides: checked on the GPU against the recorded dispatch
(tests/golden/conv_plan.json, see tests/test_conv_plan.py) through the library's own profiling registry.  After one call, the
Winograd GEMM family (4: forward / data gradient, 6: weight gradient) shows one launch exactly where the fixture says W2 or
W4, and the FLOPs that launch reports are those of the fixture's tile: 2 * planes * M * C * T with 36 planes over
ceil(H/4) * ceil(W/4) tiles (W4) or 16 planes over (H/2) * (W/2) tiles (W2).  Batch 1 throughout.  Outputs are compared with
torch at the bounds of test_gpu_parity.py::test_conv3x3 (5e-6 of max|y| on top where the pass is on the 4x4 tile)."""
import ctypes
import json
import os

import pytest
import torch
import torch.nn.functional as F

from conftest import ROOT
from test_gpu_parity import check, st

pytestmark = pytest.mark.gpu

FAMILY_WINO_GEMM, FAMILY_WINO_WGRAD_GEMM = 4, 6
# (Cin, Cout, H = W, passes, under umpr_set_conv_inference)
CASES = [(32, 32, 56, ("fwd", "dgrad", "wgrad"), False),
         (31, 64, 56, ("fwd", "dgrad"), False),
         (64, 128, 14, ("fwd", "wgrad"), False),     # forward: 4x4 tiles that hang over the border; weight gradient: 2x2 tile
         (3, 64, 16, ("fwd",), False),
         (64, 128, 112, ("fwd",), False),
         (64, 128, 112, ("fwd",), True)]


@pytest.fixture(scope="module")
def L():
    from umpr_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def rows():
    mode = os.environ.get("UMPR_WINO_F4", "2")   # read as test_conv3x3 reads it
    with open(os.path.join(ROOT, "tests", "golden", "conv_plan.json")) as fh:
        return {(r["cin"], r["cout"], r["hw"]): r for r in json.load(fh)["modes"][mode]}


def profiled(L, family, name, *args):
    """(launches, work) the family recorded during one call"""
    L.fn["umpr_profile_enable"](1)
    try:
        L.fn["umpr_profile_reset"]()
        L.call(name, *args)
        ms, work, n = ctypes.c_double(), ctypes.c_double(), ctypes.c_long()
        assert L.fn["umpr_profile_read"](family, ctypes.byref(ms), ctypes.byref(work), ctypes.byref(n)) == 0, L.last_error()
    finally:
        L.fn["umpr_profile_enable"](0)
    return n.value, work.value


def expect_gemm(what, cell, got, M, C, HW):
    launches, work = got
    if cell == "W4":
        want = (1, 2.0 * 36 * M * C * ((HW + 3) // 4) ** 2)
    elif cell == "W2":
        want = (1, 2.0 * 16 * M * C * (HW // 2) ** 2)
    else:
        want = (0, 0.0)
    assert (launches, work) == want, (what, cell, (launches, work), want)


@pytest.mark.parametrize("Cin,Cout,HW,passes,inference", CASES)
def test_entry_points_run_the_planned_algorithm(L, rows, Cin, Cout, HW, passes, inference):
    dev = torch.device("cuda:0")
    row = rows[(Cin, Cout, HW)]
    N = 1
    g = torch.Generator().manual_seed(N + Cin + Cout + HW)
    x = torch.randn(N, Cin, HW, HW, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5
    b = torch.randn(Cout, generator=g)
    x.requires_grad_(True); w.requires_grad_(True); b.requires_grad_(True)
    y_ref = F.relu(F.conv2d(x, w, b, padding=1))
    gy = torch.randn(y_ref.shape, generator=g)
    gz_ref = gy * (y_ref > 0)
    y_ref.backward(gy)
    xd, wd, bd, gz = x.detach().to(dev), w.detach().to(dev), b.detach().to(dev), gz_ref.to(dev)
    wt = torch.empty(L.size("umpr_conv3x3_pack_bytes", N, Cin, Cout, HW, HW) // 4, device=dev)
    tag = f"plan {Cin},{Cout},{HW}" + (" (inference)" if inference else "")
    if "fwd" in passes:
        cell = row["fwd_inf" if inference else "fwd"]
        y = torch.full(y_ref.shape, float("nan"), device=dev)
        L.call("umpr_set_conv_inference", 1 if inference else 0)
        try:
            got = profiled(L, FAMILY_WINO_GEMM, "umpr_conv3x3_fwd", xd, wd, bd, y, N, Cin, HW, HW, Cout, 1, wt, wt.numel() * 4, st())
        finally:
            L.call("umpr_set_conv_inference", 0)
        expect_gemm(tag + " fwd", cell, got, Cout, Cin, HW)
        check(tag + " fwd", y, y_ref, atol=2e-5, rtol=1e-5, rel_to_max=5e-6 if cell == "W4" else None)
    if "dgrad" in passes:
        cell = row["dgrad"]
        dx = torch.full(x.shape, float("nan"), device=dev)
        got = profiled(L, FAMILY_WINO_GEMM, "umpr_conv3x3_bwd_data", gz, wd, None, dx, N, Cin, HW, HW, Cout, wt, wt.numel() * 4, st())
        expect_gemm(tag + " dgrad", cell, got, Cin, Cout, HW)
        check(tag + " dgrad", dx, x.grad, atol=2e-5, rtol=1e-4, rel_to_max=5e-6 if cell == "W4" else None)
    if "wgrad" in passes:
        cell = row["wgrad"]
        dw = torch.full(w.shape, float("nan"), device=dev)
        db = torch.full(b.shape, float("nan"), device=dev)
        ws = torch.empty(L.size("umpr_conv3x3_bwd_weight_ws_bytes", N, Cin, Cout, HW, HW) // 4 + 64, device=dev)
        got = profiled(L, FAMILY_WINO_WGRAD_GEMM, "umpr_conv3x3_bwd_weight", gz, xd, dw, db, N, Cin, HW, HW, Cout, ws,
                       ws.numel() * 4, st())
        expect_gemm(tag + " wgrad", cell, got, Cout, Cin, HW)
        check(tag + " wgrad", dw, w.grad, atol=1e-4, rtol=1e-4, rel_to_max=1e-5)
        check(tag + " bgrad", db, b.grad, atol=1e-4, rtol=1e-4, rel_to_max=1e-5)
