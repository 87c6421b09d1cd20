"""umpr_conv3x3_bf16_fwd / _bwd_data / _bwd_weight at the launcher's seams: the rows of tests/bf16_conv_seams.py - the interleaved
grid rule under every tile, odd chunk counts, weight-gradient plans with short, clipped and idle splits, both reduces - and the
argument checks of the public wrappers.

Inputs go through umpr_bf16_from_nchw_f32 into 0xFF-filled tensors.  Every output and the scratch are 0xFF-filled (bf16 and fp32
NaN), exactly as long as umpr_bf16_tensor_bytes / umpr_conv3x3_bf16_ws_bytes report, between two 0xFF bands: a write past a buffer
shows in a band, a read of scratch the call never wrote shows as NaN.  Per row and pass: the gate of the input kind (equality on
the integer inputs; the interval / float32-distance gates on the random-valued ones, see the helper), every pad and guard element
of a bf16 output zero (the next layer and the weight gradient read them as zeros), a second call into the used buffers and a call
with 1 MiB more scratch bit-identical.  Every figure goes to bf16_conv_seams.log before anything is judged;
profiles/r22_a_bf16_conv_seams.txt holds those of the run that introduced the file.
"""
import copy
import os
import time

import pytest
import torch
from torch.nn.grad import conv2d_weight

import bf16_conv_seams as BS
import coattn_decisions as CD
import vgg_bf16_decisions as VB
from test_gpu_bf16 import LOG as BF16_LOG
from test_gpu_bf16 import L, dev, poison_lds, st, to_cb8   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(BF16_LOG), "bf16_conv_seams.log")
BAND = 16384                      # bytes in front of and behind every banded buffer (the buffer keeps its alignment)
MIB = 1 << 20
NAMES = ("umpr_conv3x3_bf16_fwd", "umpr_conv3x3_bf16_bwd_data", "umpr_conv3x3_bf16_bwd_weight")


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")
    print(msg)


class Banded:
    """`nbytes` of 0xFF-filled device memory between two 0xFF bands"""

    def __init__(self, dev, nbytes):
        self.n = nbytes
        self.all = torch.full((nbytes + 2 * BAND,), 0xFF, dtype=torch.uint8, device=dev)
        self.t = self.all[BAND:BAND + nbytes]

    def bands_ok(self):
        return bool((self.all[:BAND] == 0xFF).all()) and bool((self.all[BAND + self.n:] == 0xFF).all())

    def untouched(self):
        return bool((self.all == 0xFF).all())


_ON_DEV = {}


def on_dev(L, dev, shape, kind):
    """the row's operands as the entry points take them: x and gy in CB8-PF through the converter, w and b in fp32"""
    if (shape, kind) not in _ON_DEV:
        x, w, b, gy = BS.make_inputs(shape, kind)
        _ON_DEV[(shape, kind)] = {"x": to_cb8(L, x, dev), "gy": to_cb8(L, gy, dev), "w": w.to(dev), "b": b.to(dev)}
    return _ON_DEV[(shape, kind)]


@pytest.fixture(scope="module", autouse=True)
def _wall_time_and_release():
    t0 = time.time()
    yield
    log(f"wall time of tests/test_gpu_bf16_conv_seams.py: {time.time() - t0:.1f} s")
    _ON_DEV.clear()
    torch.cuda.empty_cache()


class Call:
    """One entry-point call on fresh banded 0xFF buffers.  scratch_bytes None: exactly what umpr_conv3x3_bf16_ws_bytes reports.
    `over` replaces arguments by name (None = NULL).  After run(): .raw bytes / floats on the CPU, .dec the decoded bf16 outputs,
    .pads the non-zero pad and guard elements, .problems what containment found."""

    def __init__(self, L, dev, ps, shape, ops, scratch_bytes=None, relu=1, mask=None, **over):
        N, Cin, Cout, HW = shape
        self.L, self.ps, self.shape, self.over = L, ps, shape, over
        if scratch_bytes is None:
            scratch_bytes = L.size("umpr_conv3x3_bf16_ws_bytes", N, Cin, Cout, HW, HW)
        self.scratch = Banded(dev, scratch_bytes)
        tb = lambda C: L.size("umpr_bf16_tensor_bytes", N, C, HW, HW)   # noqa: E731
        sizes = {0: (("y", tb(Cout)),), 1: (("dx", tb(Cin)),), 2: (("dw", 4 * Cout * Cin * 9), ("db", 4 * Cout))}[ps]
        self.bufs = {name: Banded(dev, n) for name, n in sizes}
        geo = dict(N=N, Cin=Cin, H=HW, W=HW, Cout=Cout)
        tail = dict(ws=self.scratch.t, ws_bytes=scratch_bytes, stream=st())
        if ps == 0:
            self.named = dict(x=ops["x"], w=ops["w"], bias=ops["b"], y=self.bufs["y"].t, **geo, relu=relu, **tail)
        elif ps == 1:
            self.named = dict(dy=ops["gy"], w=ops["w"], mask_src=mask, dx=self.bufs["dx"].t, **geo, **tail)
        else:
            self.named = dict(dy=ops["gy"], x=ops["x"], dw=self.bufs["dw"].t, db=self.bufs["db"].t, **geo, **tail)
        assert set(over) <= set(self.named), over
        self.named.update(over)
        self.raw, self.dec, self.pads, self.problems = {}, {}, {}, []

    def everything(self):
        return list(self.bufs.items()) + [("scratch", self.scratch)]

    def run(self):
        N, Cin, Cout, HW = self.shape
        self.L.call(NAMES[self.ps], *self.named.values())
        torch.cuda.synchronize()
        self.problems = [f"band of {name} written" for name, b in self.everything() if not b.bands_ok()]
        for name, b in self.bufs.items():
            if self.named.get(name, 0) is None:                          # an optional output left out
                if not b.untouched():
                    self.problems.append(f"{name} was not passed and is written")
                continue
            if self.ps < 2:
                C = Cout if self.ps == 0 else Cin
                self.raw[name] = b.t.cpu()
                self.dec[name] = VB.decode(b.t, N, C, HW, HW)
                self.pads[name] = VB.nonzero_outside(b.t, N, C, HW, HW)
                if self.pads[name]:
                    self.problems.append(f"{name}: {self.pads[name]} non-zero pad / guard elements")
            else:
                self.raw[name] = b.t.view(torch.float32).cpu()
                self.dec[name] = self.raw[name].view((Cout, Cin, 3, 3) if name == "dw" else (Cout,))
            if not bool(torch.isfinite(self.dec[name]).all()):
                self.problems.append(f"{name} is not finite")
        return self

    def refused(self, message):
        """the call must come back with `message` and must not have written anything: outputs, scratch and bands still 0xFF"""
        from umpr_amd._lib import UmprHipError
        with pytest.raises(UmprHipError, match=message):
            self.L.call(NAMES[self.ps], *self.named.values())
        torch.cuda.synchronize()
        for name, b in self.everything():
            assert b.untouched(), f"the refused call wrote {name}"


def same_bits(a, b):
    return all(torch.equal(a.raw[n].view(torch.uint8), b.raw[n].view(torch.uint8)) for n in a.raw) and set(a.raw) == set(b.raw)


def judge(tag, kind, ref, dec, relu=True):
    """the decoded outputs of one call against the row's reference; returns what is outside, logs every figure first"""
    bad = []
    for name, got in dec.items():
        rname = "e" if name == "y" else name
        if kind == "int":
            want = ref["r32"][rname]
            want = VB.q(torch.relu(want) if name == "y" and relu else want) if name in ("y", "dx") else want
            n = BS.equal_gate(got, want)
            log(f"{tag} {name}: {n} of {got.numel()} differ from the integer reference (max |ref| {float(want.abs().max()):g})")
            if n:
                bad.append((tag, name, n))
        elif name in ("y", "dx"):
            m = BS.margin(ref, rname)
            n, lax = BS.interval_gate(got, ref["r64"][rname], m, name == "y" and relu)
            log(f"{tag} {name}: {n} of {got.numel()} outside, m = {m:.3e}, lax share {lax:.3e}")
            if n or lax > BS.LAX_CAP:
                bad.append((tag, name, n, lax))
        else:
            ok, rows = CD.gate([got], [ref["r64"][name]], [ref["r32"][name]], names=[name], K=BS.K, log=log, tag=tag)
            if not ok:
                bad.append((tag, name, rows[0]["d_max"], rows[0]["r_max"], rows[0]["ratio"]))
    return bad


def run_row(L, dev, case, kind):
    ref = BS.reference(case.shape, kind, tuple(BS.runs(case)))
    ops = on_dev(L, dev, case.shape, kind)
    bad = []
    for ps in BS.runs(case):
        tag = f"{BS.case_id(case)} {kind} {BS.PASSES[ps]}"
        first = Call(L, dev, ps, case.shape, ops).run()
        bad += [(tag, p) for p in first.problems]
        bad += judge(tag, kind, ref, first.dec)
        again = _reused(first).run()
        larger = Call(L, dev, ps, case.shape, ops, scratch_bytes=first.scratch.n + MIB).run()
        bad += [(tag, "second call", p) for p in again.problems] + [(tag, "larger scratch", p) for p in larger.problems]
        if not same_bits(first, again):
            bad.append((tag, "a second call into the used buffers gives other bits"))
        if not same_bits(first, larger):
            bad.append((tag, "the result depends on the size of the scratch"))
    return bad


def _reused(call):
    """the same call on the same (now used) buffers, its results kept apart from the first call's"""
    again = copy.copy(call)
    again.raw, again.dec, again.pads, again.problems = {}, {}, {}, []
    return again


# ------------------------------------------------------------------------------------------------------- a. integer inputs
@pytest.mark.parametrize("case", BS.CASES, ids=BS.case_id)
def test_integer_inputs_are_reproduced_exactly(L, dev, case):
    bad = run_row(L, dev, case, "int")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- b. random-valued inputs
@pytest.mark.parametrize("case", BS.RANDOM_ROWS, ids=BS.case_id)
def test_random_inputs_within_the_float32_distance(L, dev, case):
    bad = run_row(L, dev, case, "rnd")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- c. chained
def test_forward_output_feeds_the_next_weight_gradient_as_it_stands(L, dev):
    """The forward's own output tensor - pads, guards and all - is `x` of the next layer's weight gradient, without passing through
    the converter.  Integer inputs on the smallest row: y <= 9 * 64 * 4 + 8 = 2312 stays an integer under bf16 rounding and
    196 * 2312 * 2 < 2^24, so the weight gradient is exact again."""
    case = BS.SMALLEST
    N, Cin, Cout, HW = case.shape
    assert Cin == Cout
    ref = BS.reference(case.shape, "int", tuple(BS.runs(case)))
    ops = on_dev(L, dev, case.shape, "int")
    fwd = Call(L, dev, 0, case.shape, ops).run()
    y = VB.q(torch.relu(ref["r32"]["e"])).float()
    want32, want64 = (conv2d_weight(y.to(t), ref["w"].shape, ref["gy"].to(t), padding=1) for t in (torch.float32, torch.float64))
    assert torch.equal(want32.double(), want64) and float(want64.abs().max()) < 2.0 ** 24 and bool((y == y.round()).all())
    wg = Call(L, dev, 2, case.shape, dict(ops, x=fwd.bufs["y"].t)).run()
    n = BS.equal_gate(wg.dec["dw"], want32)
    log(f"chained {BS.case_id(case)}: forward problems {fwd.problems}, wgrad problems {wg.problems}, dw differs at {n}")
    assert not fwd.problems and not wg.problems and BS.equal_gate(fwd.dec["y"], y) == 0 and n == 0
    assert BS.equal_gate(wg.dec["db"], ref["r32"]["db"]) == 0


# ------------------------------------------------------------------------------------------------------- d. optional arguments
@pytest.mark.parametrize("case", [BS.SMALLEST, BS.INTERLEAVED], ids=BS.case_id)
def test_without_relu_bias_and_bias_gradient(L, dev, case):
    """relu = 0 and bias = NULL: the signed convolution alone; db = NULL: the same dw, and the db buffer is not touched."""
    ref = BS.reference(case.shape, "int", tuple(BS.runs(case)))
    ops = on_dev(L, dev, case.shape, "int")
    plain = BS.evaluate(ref["x"], ref["w"], None, ref["gy"], torch.float32, (0,))
    fwd = Call(L, dev, 0, case.shape, ops, relu=0, bias=None).run()
    assert bool((fwd.dec["y"] < 0).any()), "no negative output: the ReLU is still on"
    bad = [p for p in fwd.problems] + judge(f"{BS.case_id(case)} relu0 nobias", "int", {"r32": plain}, fwd.dec, relu=False)
    wg = Call(L, dev, 2, case.shape, ops, db=None).run()
    bad += [p for p in wg.problems] + judge(f"{BS.case_id(case)} nodb", "int", ref, wg.dec)
    assert "db" not in wg.dec and "dw" in wg.dec
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- e. mask semantics
SPECIALS = (0x0000, 0x8000 - (1 << 16), 0x0001, 0x8001 - (1 << 16), 0x0080)   # +0, -0, smallest subnormals (+, -), smallest normal
KEEPS = (False, False, True, False, True)


@pytest.mark.parametrize("case", [BS.SMALLEST, BS.CASES[10]], ids=BS.case_id)
def test_mask_is_greater_than_zero_as_ieee_defines_it(L, dev, case):
    """mask_src > 0 is false at +0, -0 and the negative subnormal and true at the positive subnormal and the smallest normal - the
    comparison the header states for the fp32 entry point, nothing flushed: the masked dx holds the unmasked call's bits where it is
    true and +0 elsewhere.  On the smallest row and on a data gradient under the interleaved rule."""
    N, Cin, Cout, HW = case.shape
    ops = on_dev(L, dev, case.shape, "rnd")
    plain = Call(L, dev, 1, case.shape, ops).run()
    g = torch.Generator().manual_seed(N * Cin * HW)
    bits = VB.q(torch.randn(N, Cin, HW, HW, generator=g)).float().view(torch.int32) >> 16     # bf16 bits of a normal draw
    reps = 40
    live = torch.nonzero(plain.dec["dx"].flatten()).flatten()
    where = live[torch.randperm(len(live), generator=g)[:reps * len(SPECIALS)]]
    bits.view(-1)[where] = torch.tensor(SPECIALS, dtype=torch.int32).repeat(reps)
    keep = bits > 0                                            # sign clear and not zero: > 0 for everything that is no NaN
    assert torch.equal(keep.view(-1)[where], torch.tensor(KEEPS).repeat(reps))
    mask_f32 = (bits << 16).view(torch.float32)
    ps = VB.plane_stride(L.size("umpr_bf16_tensor_bytes", N, Cin, HW, HW), Cin)
    mask = VB.encode(mask_f32, ps).to(dev)
    masked = Call(L, dev, 1, case.shape, ops, mask=mask).run()
    assert not plain.problems and not masked.problems, (plain.problems, masked.problems)
    want = torch.where(keep, plain.dec["dx"].float(), torch.zeros(()))
    wrong = torch.nonzero(want.view(torch.int32) != masked.dec["dx"].float().view(torch.int32))
    log(f"mask {BS.case_id(case)}: {int(keep.sum())} of {keep.numel()} kept, {len(wrong)} wrong")
    assert len(wrong) == 0, [(tuple(int(v) for v in i), hex(int(bits[tuple(i)]) & 0xFFFF), float(plain.dec["dx"][tuple(i)]),
                              float(masked.dec["dx"][tuple(i)])) for i in wrong[:8]]


# ------------------------------------------------------------------------------------------------------- f. refusals
REQUIRED = {0: ("x", "w", "y", "ws"), 1: ("dy", "w", "dx", "ws"), 2: ("dy", "x", "dw", "ws")}


def test_what_the_entry_points_refuse(L, dev):
    """Every refusal is a host check in the wrapper or in the plan function the launcher starts with (api.hip,
    umpr_conv_bf16_plan / umpr_wgrad_bf16_plan), taken before the first launch: non-zero, the cause named, no byte written."""
    # the passes a row marks refused
    for case in BS.CASES:
        ops = on_dev(L, dev, case.shape, "int")
        for ps in (0, 1, 2):
            if ps not in BS.runs(case):
                Call(L, dev, ps, case.shape, ops).refused("must be multiples of")
    case = BS.SMALLEST
    N, Cin, Cout, HW = case.shape
    ops = on_dev(L, dev, case.shape, "int")
    for ps in (0, 1, 2):
        least = Cin * Cout * 18 + 1024 if ps < 2 else case.wgrad.splits * (9 * Cout * Cin + Cout) * 4 + 1024
        Call(L, dev, ps, case.shape, ops, scratch_bytes=least - 1).refused("scratch too small" if ps < 2 else "workspace too small")
        assert not Call(L, dev, ps, case.shape, ops, scratch_bytes=least).run().problems      # ... and that least is enough
        for name in REQUIRED[ps]:
            Call(L, dev, ps, case.shape, ops, **{name: None}).refused(f"{name} is NULL")
        Call(L, dev, ps, case.shape, ops, N=0).refused("must be positive")
        Call(L, dev, ps, case.shape, ops, Cin=0).refused("must be positive")
        Call(L, dev, ps, (N, Cin, Cout, 16), ops).refused("not a VGG16 map size")
    # the two pools
    from umpr_amd._lib import UmprHipError
    x, y, gx = ops["x"], Banded(dev, L.size("umpr_bf16_tensor_bytes", N, Cin, HW // 2, HW // 2)), Banded(dev, ops["x"].numel())
    for args, message in (((None, y.t, N, Cin, HW, HW), "x is NULL"), ((x, None, N, Cin, HW, HW), "y is NULL"),
                          ((x, y.t, 0, Cin, HW, HW), "must be positive"), ((x, y.t, N, Cin, 0, HW), "must be positive")):
        with pytest.raises(UmprHipError, match=message):
            L.call("umpr_maxpool2_bf16_fwd", *args, st())
    for args, message in (((None, y.t, gx.t, N, Cin, HW, HW), "x is NULL"), ((x, None, gx.t, N, Cin, HW, HW), "dy is NULL"),
                          ((x, y.t, None, N, Cin, HW, HW), "dx is NULL"), ((x, y.t, gx.t, 0, Cin, HW, HW), "must be positive")):
        with pytest.raises(UmprHipError, match=message):
            L.call("umpr_maxpool2_bf16_bwd_relu", *args, st())
    torch.cuda.synchronize()
    assert y.untouched() and gx.untouched()
