"""Case table and float64 reference of the fp32 3x3 convolution entry points at the launcher's seams (test helper, not a test
module; CPU only).

umpr_conv3x3_fwd / _bwd_data / _bwd_weight run what umpr_conv3x3_plan (umpr_amd/csrc/conv3x3.hip) names.  A case is a shape
(N, Cin, Cout, H, W) plus the algorithm each pass is meant to land on with no UMPR_* switch set, in the codes of
tests/golden/conv_plan.json (G generic gather kernels, C first-layer kernels, D LDS-patch direct kernels, W2 / W4 Winograd tiles).
tests/test_conv_seams_cases.py asks the plan whether every row lands where it says and whether the table covers every kernel
family; tests/test_gpu_conv_seams.py runs the cases on the GPU.

Reference: F.conv2d(padding=1) in float64 with autograd; the yardstick of coattn_decisions.gate is the same expression in float32 on
the CPU.  Inputs are seeded from the shape: x = relu(randn), w = randn * sqrt(2 / (9 Cin)), b = 0.1 randn, gy = randn and
gz = gy * (z64 > 0) from the float64 pre-activation z64 - the gradient with respect to the pre-activation, which is what the
two backward entry points take, so no ReLU decision of a kernel enters the backward.
"""
import collections
import functools

import torch
import torch.nn.functional as F

CODES = {"G": 0, "C": 1, "D": 2, "W2": 3, "W4": 4}
PASSES = ("fwd", "dgrad", "wgrad")                  # pass codes 0, 1, 2 of umpr_debug_conv3x3_plan
Case = collections.namedtuple("Case", "shape fwd dgrad wgrad what")

CASES = (
    # generic kernels, tiny and non-square
    Case((1, 1, 1, 1, 1), "G", "G", "G", "every tap but the centre is padding; wgrad segment R=32, CW=1"),
    Case((2, 5, 7, 1, 9), "G", "G", "G", "H = 1; wgrad segment (3,9)"),
    Case((3, 7, 66, 5, 3), "G", "G", "G", "Cout = 66 on the <128,128> tile; 45 pixels in one partial pixel tile"),
    Case((1, 65, 3, 2, 67), "G", "G", "G", "K tail at Cin = 65; second pixel tile holds 6 pixels; wgrad segment (1,32) with a "
                                           "3-column tail at the (R+2)(CW+2) = 102 limit"),
    Case((2, 4, 130, 6, 10), "G", "G", "G", "two Cout tiles, the second holding 2 channels"),
    # direct weight-gradient templates off the VGG maps (forward and data gradient are generic there)
    Case((1, 8, 70, 7, 16), "G", "G", "D", "<2,16>, odd H"),
    Case((2, 66, 9, 10, 8), "G", "G", "D", "<4,8>, H % 4 = 2, two Cin tiles"),
    Case((1, 5, 64, 3, 14), "G", "G", "D", "<2,14>, odd H"),
    Case((2, 8, 70, 32, 32), "G", "G", "D", "64 segments: the default split count is >= 32 and the wide reduce kernel runs"),
    # first-layer kernels
    Case((3, 3, 70, 6, 32), "G", "G", "C", "wgrad C3 with a Cout tail and two Cout tiles; forward generic (Cout != 64)"),
    Case((1, 2, 64, 5, 16), "C", "G", "C", "forward C3 and wgrad C3 at Cin = 2, non-square, odd H"),
    Case((2, 1, 64, 3, 7), "C", "G", "G", "forward C3 at Cin = 1; wgrad generic with segment (4,7)"),
    # VGG maps with off-grid channels
    Case((2, 5, 70, 14, 14), "D", "W4", "D", "forward D; data gradient W4 with overhanging tiles; wgrad D <2,14>"),
    Case((1, 31, 33, 28, 28), "D", "W4", "D", "forward D; data gradient W4; wgrad D"),
    Case((3, 33, 65, 14, 14), "W4", "W4", "W2", "forward W4 edge; data gradient W4 edge; wgrad W2"),
    Case((1, 33, 65, 28, 28), "W4", "W4", "W4", "W4 on all three passes"),
    # (the table the cases were drawn up from had no data gradient on the direct kernel: fewer than 32 reduction channels)
    Case((2, 33, 5, 14, 14), "W4", "D", "D", "data gradient D: Cout = 5 is one packed stage of 4 channels and a tail of 1, 33 output "
                                             "rows on the 64-row tile"),
)
# what the table as a whole must reach
COVER = {"fwd": {"G", "C", "D", "W4"}, "dgrad": {"G", "D", "W4"}, "wgrad": {"G", "C", "D", "W2", "W4"}}
WGRAD_TEMPLATES = {(2, 16), (4, 8), (2, 14)}        # conv3x3_wgrad_v2_kernel<R, CW>
# the scratch fallbacks run on these two
FALLBACK_W4 = Case((1, 64, 64, 28, 28), "W4", "W4", "W4", "W4-planned on all passes: with less scratch, the direct kernels")
FALLBACK_D = CASES[5]


def case_id(case):
    return "x".join(str(v) for v in case.shape)


def segment(W):
    """(R, CW) of the direct weight gradient's pixel segment, from the comment of wgrad_segment in conv3x3.hip: R rows x CW columns
    with R * CW <= 32; two rows of 16 where W is a multiple of 16, else four of 8 where it is a multiple of 8, else two of 14 where
    it is a multiple of 14, else whole rows of a map narrower than 32, else one row of 32."""
    if W % 16 == 0:
        return 2, 16
    if W % 8 == 0:
        return 4, 8
    if W % 14 == 0:
        return 2, 14
    if W < 32:
        return 32 // W, W
    return 1, 32


def make_inputs(shape):
    N, Cin, Cout, H, W = shape
    g = torch.Generator().manual_seed(((((N * 131 + Cin) * 131 + Cout) * 131 + H) * 131 + W) % (2 ** 31))
    x = torch.relu(torch.randn(N, Cin, H, W, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5
    b = 0.1 * torch.randn(Cout, generator=g)
    gy = torch.randn(N, Cout, H, W, generator=g)
    return x, w, b, gy


def conv_and_grads(x, w, b, gz, dtype):
    """z = conv(x, w) + b and the gradients of <gz, z> in `dtype`: (z, dx, dw, db)"""
    xs, ws, bs = (t.detach().to(dtype).requires_grad_(True) for t in (x, w, b))
    z = F.conv2d(xs, ws, bs, padding=1)
    dx, dw, db = torch.autograd.grad(z, (xs, ws, bs), gz.to(dtype))
    return z.detach(), dx, dw, db


@functools.lru_cache(maxsize=None)
def reference(shape):
    """The inputs of a shape and both evaluations, computed once and shared: x, w, b, gz (float32, as the kernels get them) and
    z / y / dx / dw / db as pairs (float64 reference, float32 CPU yardstick).  Nobody writes into them."""
    x, w, b, gy = make_inputs(shape)
    z64 = F.conv2d(x.double(), w.double(), b.double(), padding=1)
    gz = gy * (z64 > 0)
    r64 = conv_and_grads(x, w, b, gz, torch.float64)
    r32 = conv_and_grads(x, w, b, gz, torch.float32)
    out = {"x": x, "w": w, "b": b, "gz": gz}
    for name, a, c in zip(("z", "dx", "dw", "db"), r64, r32):
        out[name] = (a, c)
    out["y"] = (torch.relu(r64[0]), torch.relu(r32[0]))
    return out
