"""Case table, references and gates of the bf16 3x3 convolution entry points at the launcher's seams (test helper, not a test
module; CPU only).

umpr_conv3x3_bf16_fwd / _bwd_data / _bwd_weight launch what umpr_conv_bf16_plan / umpr_wgrad_bf16_plan (umpr_amd/csrc/bf16_conv.hip)
say; umpr_debug_conv_bf16_plan reports it.  A case is a shape (N, Cin, Cout, HW) plus, per pass, the plan the row is there for, or
None where the entry point must refuse the shape.  tests/test_bf16_conv_seams_cases.py asks the plan query whether every row is
what it says and whether the table reaches every branch of the two launchers; tests/test_gpu_bf16_conv_seams.py runs the rows.

Two kinds of input, both seeded from the shape:
  "int"  x, w, gy integers in [-2, 2], bias an integer in [-8, 8].  Every product and every partial sum of every pass is an integer
         below 2^24 (forward 9 Cin 4 + 8 <= 11 528, data gradient 9 Cout 4 <= 41 472, weight gradient N HW^2 4 <= 401 408), so
         any fp32 summation order gives the same bits as float64 and the gate is EQUALITY: y == q(relu(e)), dx == q(e), dw and
         db equal to the integer.  |e| <= 256 is bf16-exact, so q is the identity on nearly every output.
  "rnd"  bf16-exact values: x = q(relu(randn)), w = q(randn sqrt(2 / (9 Cin))), gy = q(randn); bias = 0.1 randn in float32.  The
         reference e is the float64 convolution of those operands, the yardstick the same expression in float32 on the CPU, and
         m = K max|float32 - float64| over the tensor, K = 4 (coattn_decisions.K_START).  Forward and data gradient: every element
         must lie in [q(relu(e - m)), q(relu(e + m))] (no ReLU for dx) - rounding is monotone, so that is exactly "the bf16
         rounding of some value within m of e"; where the two ends coincide the element is held bit for bit.  The share of elements
         whose ends differ ("lax") must stay under LAX_CAP: a condition on the inputs, asserted on the CPU.  dw and db (fp32):
         coattn_decisions.gate with K = 4.
The backward passes take gy as the gradient with respect to the pre-activation, so no ReLU decision enters them.
"""
import collections
import functools

import torch
import torch.nn.functional as F
from torch.nn.grad import conv2d_input, conv2d_weight

import coattn_decisions as CD
import vgg_bf16_decisions as VB

PASSES = ("fwd", "dgrad", "wgrad")                  # pass codes 0, 1, 2 of umpr_debug_conv_bf16_plan
K = CD.K_START
LAX_CAP = 2e-2
# out[0..7] of umpr_debug_conv_bf16_plan; C: passes 0 / 1, G: pass 2 (include/umpr_hip.h)
C = collections.namedtuple("C", "BN nct ntp blocks interleaved chunks two_d pingpong")
G = collections.namedtuple("G", "big nseg ntiles splits segs_per_split last_segs blocks wide")
Case = collections.namedtuple("Case", "shape fwd dgrad wgrad what")

CASES = (
    Case((1, 64, 64, 14), C(64, 1, 1, 8, 0, 2, 0, 0), C(64, 1, 1, 8, 0, 2, 0, 0), G(0, 2, 1, 2, 1, 1, 8, 0),
         "one pixel tile, partly filled; splits clipped to nseg = 2, six idle splits"),
    Case((1, 32, 64, 14), C(64, 1, 1, 8, 0, 1, 0, 0), None, None, "forward on one chunk: nine steps, all ring prologue / epilogue"),
    Case((1, 64, 32, 14), None, C(64, 1, 1, 8, 0, 1, 0, 0), None, "data gradient on one chunk"),
    Case((2, 96, 192, 28), C(64, 3, 7, 24, 1, 3, 0, 0), None, None, "3 chunks, nct = 3 interleaved, ntp = 7 of a round of 8"),
    Case((2, 192, 96, 28), None, C(64, 3, 7, 24, 1, 3, 0, 0), None, "the same through the transposed pack"),
    Case((3, 192, 192, 56), C(64, 3, 39, 120, 1, 6, 0, 0), C(64, 3, 39, 120, 1, 6, 0, 0), G(0, 77, 9, 26, 3, 2, 288, 0),
         "nct = 3 interleaved over five rounds; 64x64 wgrad tile with 9 tiles, 26 splits of 3 (last 2), linear reduce, 6 idle"),
    Case((1, 64, 384, 112), C(128, 3, 56, 168, 1, 2, 1, 0), C(64, 1, 56, 56, 0, 12, 1, 0), G(1, 105, 3, 53, 2, 1, 168, 1),
         "BN 128 interleaved on the 2-D 16x16 tile; 12 chunks; 128x64 wgrad tile, 53 splits of 2 (last 1), wide reduce"),
    Case((2, 64, 768, 28), C(256, 3, 7, 24, 1, 2, 0, 1), C(64, 1, 7, 8, 0, 24, 0, 0), G(1, 14, 6, 14, 1, 1, 96, 0),
         "BN 256 interleaved under ping-pong; 24 chunks; 14 splits"),
    Case((2, 64, 768, 14), C(128, 6, 2, 48, 1, 2, 0, 1), C(64, 1, 2, 8, 0, 24, 0, 0), G(1, 4, 6, 4, 1, 1, 48, 0),
         "BN 128, nct = 6 interleaved under ping-pong"),
    Case((1, 64, 1152, 14), C(128, 9, 1, 72, 1, 2, 0, 1), C(64, 1, 1, 8, 0, 36, 0, 0), G(1, 2, 9, 2, 1, 1, 72, 0),
         "nct = 9 > 8; 36 chunks; 9 wgrad tiles on 2 splits"),
    Case((3, 320, 128, 14), C(128, 1, 3, 8, 0, 10, 0, 1), C(64, 5, 3, 40, 1, 4, 0, 0), G(1, 6, 5, 6, 1, 1, 40, 0),
         "10 chunks; data gradient nct = 5 interleaved; ncit = 5"),
    Case((2, 64, 192, 224), C(64, 3, 399, 1200, 1, 2, 1, 0), C(64, 1, 399, 400, 0, 6, 1, 0), G(0, 791, 3, 88, 9, 8, 264, 1),
         "8x32 tile interleaved, last band 3 rows, a band across the image seam; 88 splits of 9 (last 8), wide reduce"),
    Case((1, 128, 64, 224), C(64, 1, 203, 208, 0, 4, 1, 0), C(128, 1, 203, 208, 0, 2, 1, 0), G(0, 399, 2, 100, 4, 3, 208, 1),
         "64x64 wgrad tile with ncit = 2 on the 4x32 segment, 100 splits of 4 (last 3)"),
    # added after the plan query showed them unreached by the rows above
    Case((1, 64, 256, 28), C(256, 1, 4, 8, 0, 2, 0, 1), C(64, 1, 4, 8, 0, 8, 0, 0), G(1, 7, 2, 7, 1, 1, 16, 0),
         "BN 256 on the grouped grid rule (nct = 1)"),
    Case((1, 64, 256, 112), C(256, 1, 56, 56, 0, 2, 1, 1), C(64, 1, 56, 56, 0, 8, 1, 0), G(1, 105, 2, 105, 1, 1, 224, 1),
         "the 2-D tile under ping-pong (BN 256 on a 112 map)"),
)
SMALLEST = CASES[0]
INTERLEAVED = CASES[5]          # all three passes, forward and data gradient interleaved
RANDOM_ROWS = tuple(c for c in CASES if c.shape[3] in (14, 28, 56))      # the 224 and 112 rows run the integer inputs only
NCIT = {(3, 192, 192, 56): 3, (3, 320, 128, 14): 5, (1, 128, 64, 224): 2}   # out[9] of pass 2 where it is not 1


def case_id(case):
    return "x".join(str(v) for v in case.shape)


def runs(case):
    """the pass codes a row runs"""
    return [ps for ps in (0, 1, 2) if case[1 + ps] is not None]


def make_inputs(shape, kind):
    """x, w, b, gy as float32"""
    N, Cin, Cout, HW = shape
    g = torch.Generator().manual_seed((((N * 131 + Cin) * 131 + Cout) * 131 + HW + (7 if kind == "int" else 0)) % (2 ** 31))
    if kind == "int":
        ri = lambda lo, hi, *s: torch.randint(lo, hi + 1, s, generator=g).float()   # noqa: E731
        return ri(-2, 2, N, Cin, HW, HW), ri(-2, 2, Cout, Cin, 3, 3), ri(-8, 8, Cout), ri(-2, 2, N, Cout, HW, HW)
    assert kind == "rnd", kind
    q32 = lambda t: VB.q(t).float()   # noqa: E731
    x = q32(torch.relu(torch.randn(N, Cin, HW, HW, generator=g)))
    w = q32(torch.randn(Cout, Cin, 3, 3, generator=g) * (2.0 / (9 * Cin)) ** 0.5)
    b = 0.1 * torch.randn(Cout, generator=g)
    gy = q32(torch.randn(N, Cout, HW, HW, generator=g))
    return x, w, b, gy


def evaluate(x, w, b, gy, dtype, passes=(0, 1, 2)):
    """{e (pre-activation), dx, dw, db} of the passes asked for, computed in `dtype`; b may be None"""
    x, w, gy = x.to(dtype), w.to(dtype), gy.to(dtype)
    out = {}
    if 0 in passes:
        out["e"] = F.conv2d(x, w, None if b is None else b.to(dtype), padding=1)
    if 1 in passes:
        out["dx"] = conv2d_input(x.shape, w, gy, padding=1)
    if 2 in passes:
        out["dw"] = conv2d_weight(x, w.shape, gy, padding=1)
        out["db"] = gy.sum((0, 2, 3))
    return out


@functools.lru_cache(maxsize=None)
def reference(shape, kind, passes=(0, 1, 2)):
    """Inputs and evaluations of one row (passes: a tuple of pass codes), computed once and shared; nobody writes into them.
    "int": r32 is the reference and r64 is None (the CPU test shows that float64 gives the same); "rnd": r64 is the reference,
    r32 the yardstick."""
    x, w, b, gy = make_inputs(shape, kind)
    out = {"x": x, "w": w, "b": b, "gy": gy, "r32": evaluate(x, w, b, gy, torch.float32, passes)}
    out["r64"] = evaluate(x, w, b, gy, torch.float64, passes) if kind == "rnd" else None
    return out


def margin(ref, name):
    """m of a random-valued tensor: K x the float32 evaluation's largest distance from float64"""
    return K * float((ref["r32"][name].double() - ref["r64"][name]).abs().max())


def interval(e64, m, relu):
    lo, hi = e64 - m, e64 + m
    if relu:
        lo, hi = torch.relu(lo), torch.relu(hi)
    return VB.q(lo), VB.q(hi)


def interval_gate(got, e64, m, relu):
    """(elements outside [q(e - m), q(e + m)], share of elements whose two ends differ); a NaN is outside"""
    lo, hi = interval(e64, m, relu)
    inside = (got.double() >= lo) & (got.double() <= hi)
    return int((~inside).sum()), float((lo != hi).double().mean())


def equal_gate(got, want):
    """elements of `got` that are not the value `want` names (+0 and -0 are the same value; a NaN is none)"""
    return int((got.double() != want.double()).sum())


def flat_pixel(N, HW):
    """padded-flat pixel index P of (n, y, x) - the header comment of bf16_conv.hip - as LongTensor [N][HW][HW]"""
    n = torch.arange(N).view(N, 1, 1)
    y = torch.arange(HW).view(1, HW, 1)
    x = torch.arange(HW).view(1, 1, HW)
    return (n * (HW + 1) + y + 1) * (HW + 1) + x + 1


# ---- mutants of the CPU evaluation: what a subtly wrong kernel would compute (float32, on the same inputs) ---------------------
def mutant_pixel_dropped(ref, passes):
    """one input pixel read as zero: x in the forward and the weight gradient, gy in the data gradient (and db)"""
    x, gy = ref["x"].clone(), ref["gy"].clone()
    ix = tuple(int(v) for v in torch.nonzero(x)[x.count_nonzero() // 2])
    ig = tuple(int(v) for v in torch.nonzero(gy)[gy.count_nonzero() // 2])
    x[ix] = 0.0
    gy[ig] = 0.0
    out = evaluate(x, ref["w"], ref["b"], ref["gy"], torch.float32, [p for p in passes if p != 1])
    out.update(evaluate(ref["x"], ref["w"], ref["b"], gy, torch.float32, [p for p in passes if p == 1]))
    if 2 in passes:
        out["db"] = gy.sum((0, 2, 3))
    return out


def mutant_tap_skipped(ref, passes):
    w = ref["w"].clone()
    iw = tuple(int(v) for v in torch.nonzero(w)[w.count_nonzero() // 2])
    w[iw] = 0.0
    return evaluate(ref["x"], w, ref["b"], ref["gy"], torch.float32, [p for p in passes if p != 2])


def mutant_next_tiles_weights(ref, passes, bn=64):
    """output-channel tile 0 of the forward (data gradient: of Cin) computed with tile 1's weights"""
    out = {}
    if 0 in passes:
        w = ref["w"].clone()
        w[:bn] = ref["w"][bn:2 * bn]
        out.update(evaluate(ref["x"], w, ref["b"], ref["gy"], torch.float32, [0]))
    if 1 in passes:
        w = ref["w"].clone()
        w[:, :bn] = ref["w"][:, bn:2 * bn]
        out.update(evaluate(ref["x"], w, ref["b"], ref["gy"], torch.float32, [1]))
    return out


def mutant_last_segment_left_out(ref, nseg, seg_pixels=128):
    """the weight gradient without its last segment of 128 consecutive flat pixels (the 1-D segment of the 56 / 28 / 14 maps)"""
    N, _, HW, _ = ref["x"].shape
    keep = (flat_pixel(N, HW) < (nseg - 1) * seg_pixels).view(N, 1, HW, HW)
    assert 0 < int((~keep).sum()), "the last segment holds no real pixel"
    return evaluate(ref["x"], ref["w"], ref["b"], ref["gy"] * keep, torch.float32, [2])


def mutant_chunk_rounded(ref):
    """forward whose accumulator is rounded to bf16 once per 32-channel chunk"""
    x, w = ref["x"], ref["w"]
    acc = ref["b"].view(1, -1, 1, 1).expand(x.shape[0], -1, x.shape[2], x.shape[3]).clone()
    for c0 in range(0, x.shape[1], 32):
        acc = VB.q(acc + F.conv2d(x[:, c0:c0 + 32], w[:, c0:c0 + 32], None, padding=1)).float()
    return {"e": acc}
