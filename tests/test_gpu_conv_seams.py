"""umpr_conv3x3_fwd / _bwd_data / _bwd_weight at the launcher's seams: the cases of tests/conv_seams.py (generic kernels on tiny and
non-square maps, the direct weight-gradient templates with a last segment that is not full, the first-layer kernels below three
channels, VGG maps with channel counts off every tile) and the three scratch-size fallbacks of umpr_conv3x3_run / umpr_conv3x3_wgrad.

Every output and every scratch buffer is NaN-filled, exactly as long as the size entry point says, and sits between two NaN guard
bands (Guarded of test_gpu_workspace_layouts.py): a write past a buffer shows in a band, a read of scratch the call never wrote
shows as NaN.  Results must not depend on the scratch being larger (bit-identical with 1 MiB more).  Accuracy: cells on the generic,
first-layer and direct kernels and the F(2x2,3x3) weight gradient are held to K x the distance the float32 CPU convolution has from
the float64 one (coattn_decisions.gate: K = 4, floor 2^-22); cells on the F(4x4,3x3) tile cannot meet a direct-sum yardstick and
keep the bounds test_gpu_parity.py::test_conv3x3 states for them, their ratios are logged only.  Every row goes to conv_seams.log
before anything is judged; profiles/r20_a_conv_seams.txt holds the worst ratio per cell of the run that set K.
"""
import ctypes
import os

import pytest
import torch

import coattn_decisions as CD
import conv_seams as CS
from test_gpu_conv_plan import FAMILY_WINO_GEMM, FAMILY_WINO_WGRAD_GEMM, profiled
from test_gpu_parity import LOG as PARITY_LOG
from test_gpu_parity import L, check, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)
from test_gpu_workspace_layouts import MIB, NAN_BITS, Guarded

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "conv_seams.log")
# gate factors above K_START by "<pass> <cell>", each no more than a measured worst ratio (profiles/r20_a_conv_seams.txt).
K_OF = {}
LETTER = {v: k for k, v in CS.CODES.items()}
DEFAULT_SWITCHES = not any(k.startswith("UMPR_") and k != "UMPR_TEST_CHILD" for k in os.environ)


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def plan(L, ps, shape):
    """(letter, ws_bytes) umpr_conv3x3_plan gives pass `ps` (0 forward, 1 data gradient, 2 weight gradient) in this process"""
    ws = ctypes.c_size_t()
    algo = L.fn["umpr_debug_conv3x3_plan"](ps, *shape, 0, ctypes.byref(ws), None)
    return LETTER[algo], ws.value


def untouched(t):
    return bool((t.view(torch.int32) == NAN_BITS).all())


_ON_DEV = {}


def on_dev(dev, shape):
    if shape not in _ON_DEV:
        ref = CS.reference(shape)
        _ON_DEV[shape] = {k: ref[k].to(dev) for k in ("x", "w", "b", "gz")}
    return _ON_DEV[shape]


class Call:
    """One entry-point call on fresh guarded NaN buffers.  scratch_bytes None: exactly what the size entry point reports;
    "null": no scratch at all.  After run(): .out = the outputs on the CPU, .problems = what containment found."""

    def __init__(self, L, dev, ps, shape, scratch_bytes=None, relu=1, mask=None):
        N, Cin, Cout, H, W = shape
        self.L, self.ps, self.shape, self.relu, self.mask = L, ps, shape, relu, mask
        self.d = on_dev(dev, shape)
        size = "umpr_conv3x3_bwd_weight_ws_bytes" if ps == 2 else "umpr_conv3x3_pack_bytes"
        if scratch_bytes is None:
            scratch_bytes = L.size(size, *shape)
        self.scratch = None if scratch_bytes == "null" else Guarded(dev, scratch_bytes)
        outs = {0: (("y", N * Cout * H * W),), 1: (("dx", N * Cin * H * W),), 2: (("dw", Cout * Cin * 9), ("db", Cout))}[ps]
        self.bufs = {name: Guarded(dev, 4 * n) for name, n in outs}
        self.out, self.problems = {}, []

    def args(self):
        N, Cin, Cout, H, W = self.shape
        d, sc = self.d, self.scratch
        tail = (sc.t if sc else None, sc.n * 4 if sc else 0, st())
        if self.ps == 0:
            return ("umpr_conv3x3_fwd", d["x"], d["w"], d["b"], self.bufs["y"].t, N, Cin, H, W, Cout, self.relu) + tail
        if self.ps == 1:
            return ("umpr_conv3x3_bwd_data", d["gz"], d["w"], self.mask, self.bufs["dx"].t, N, Cin, H, W, Cout) + tail
        return ("umpr_conv3x3_bwd_weight", d["gz"], d["x"], self.bufs["dw"].t, self.bufs["db"].t, N, Cin, H, W, Cout) + tail

    def collect(self):
        torch.cuda.synchronize()
        named = list(self.bufs.items()) + ([("scratch", self.scratch)] if self.scratch else [])
        self.problems = [f"guard band of {name} written" for name, b in named if not b.guards_ok()]
        self.problems += [f"{name} is not finite" for name, b in self.bufs.items() if not bool(torch.isfinite(b.t).all())]
        self.out = {name: b.t.cpu() for name, b in self.bufs.items()}
        return self

    def run(self):
        self.L.call(*self.args())
        return self.collect()

    def release(self):
        """drop the device buffers; .out and .problems stay"""
        self.scratch_bytes = self.scratch.n * 4 if self.scratch else 0
        self.bufs = self.scratch = self.d = self.mask = None
        return self

    def run_profiled(self, family):
        """as run(); returns the launches the library's profiling registry saw in `family`"""
        name, *rest = self.args()
        launches, _ = profiled(self.L, family, name, *rest)
        self.collect()
        return launches

    def refused(self, message):
        """the call must come back with `message` and must not have written anything: outputs, scratch and bands still NaN"""
        from umpr_amd._lib import UmprHipError
        with pytest.raises(UmprHipError, match=message):
            self.L.call(*self.args())
        torch.cuda.synchronize()
        for name, b in list(self.bufs.items()) + ([("scratch", self.scratch)] if self.scratch else []):
            assert untouched(b.all), f"the refused call wrote {name}"


def shaped(shape, name, t):
    N, Cin, Cout, H, W = shape
    return t.view({"y": (N, Cout, H, W), "z": (N, Cout, H, W), "dx": (N, Cin, H, W), "dw": (Cout, Cin, 3, 3), "db": (Cout,)}[name])


W4_BOUNDS = {"y": dict(atol=2e-5, rtol=1e-5, rel_to_max=5e-6), "dx": dict(atol=2e-5, rtol=1e-4, rel_to_max=5e-6),
             "dw": dict(atol=1e-4, rtol=1e-4, rel_to_max=1e-5), "db": dict(atol=1e-4, rtol=1e-4, rel_to_max=1e-5)}


def judge(tag, ps, cell, shape, out, ref_name=None):
    """Every tensor of `out` against the float64 reference: gated where the cell is a direct sum, at test_conv3x3's bounds (ratio
    logged only) on the 4x4 tile.  Returns the rows that are outside."""
    ref = CS.reference(shape)
    bad = []
    for name, got in out.items():
        r64, r32 = ref[ref_name or name]
        got = shaped(shape, name, got)
        key = f"{CS.PASSES[ps]} {cell}"
        ok, rows = CD.gate([got], [r64], [r32], names=[name], K=K_OF.get(key, CD.K_START), log=log,
                           tag=f"{tag} [{key}{'' if cell != 'W4' else ', not gated'}]")
        if cell == "W4":
            check(f"{tag} {name}", got, r64, **W4_BOUNDS[name])
        elif not ok:
            bad.append((tag, name, rows[0]["d_max"], rows[0]["r_max"], rows[0]["ratio"]))
    return bad


_RUNS = {}


@pytest.fixture(scope="module", autouse=True)
def _release_buffers():
    """the module keeps nothing on the device behind it: the cached inputs go, and the allocator hands its free blocks back"""
    yield
    _ON_DEV.clear()
    _RUNS.clear()
    torch.cuda.empty_cache()


def case_runs(L, dev, case):
    """per pass: (cell, the call at the exact scratch size, the same call with 1 MiB more)"""
    if case.shape not in _RUNS:
        runs = []
        for ps in (0, 1, 2):
            cell, _ = plan(L, ps, case.shape)
            exact = Call(L, dev, ps, case.shape).run().release()
            larger = Call(L, dev, ps, case.shape, scratch_bytes=exact.scratch_bytes + MIB).run().release()
            runs.append((cell, exact, larger))
        _RUNS[case.shape] = runs
    return _RUNS[case.shape]


# ------------------------------------------------------------------------------------------------------- a. containment
@pytest.mark.parametrize("case", CS.CASES, ids=CS.case_id)
def test_containment_at_exact_sizes(L, dev, case):
    bad = []
    for ps, (cell, exact, larger) in enumerate(case_runs(L, dev, case)):
        if DEFAULT_SWITCHES:
            assert cell == case[1 + ps], (case.shape, CS.PASSES[ps], cell)
        for size, c in (("exact", exact), ("larger", larger)):
            print(f"{CS.case_id(case)} {CS.PASSES[ps]} {cell} {size}: problems {c.problems}")
            bad += [(CS.PASSES[ps], size, p) for p in c.problems]
        for name in exact.out:
            if not torch.equal(exact.out[name].view(torch.int32), larger.out[name].view(torch.int32)):
                bad.append((CS.PASSES[ps], f"{name} depends on the size of the scratch"))
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- b. accuracy
@pytest.mark.parametrize("case", CS.CASES, ids=CS.case_id)
def test_accuracy_against_float64(L, dev, case):
    bad = []
    for ps, (cell, exact, _) in enumerate(case_runs(L, dev, case)):
        bad += judge(f"seam {CS.case_id(case)}", ps, cell, case.shape, exact.out)
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- c. relu = 0
@pytest.mark.parametrize("case", [CS.CASES[2], CS.CASES[10], CS.CASES[12]], ids=CS.case_id)
def test_forward_without_relu(L, dev, case):
    """One forward on the generic, one on the first-layer and one on the direct kernel: the signed pre-activation."""
    cell, _ = plan(L, 0, case.shape)
    if DEFAULT_SWITCHES:
        assert cell == case.fwd and cell in "GCD"
    c = Call(L, dev, 0, case.shape, relu=0).run()
    assert not c.problems, c.problems
    assert bool((c.out["y"] < 0).any()), "no negative output: the ReLU is still on"
    bad = judge(f"relu0 {CS.case_id(case)}", 0, cell, case.shape, c.out, ref_name="z")
    assert not bad, bad


# ------------------------------------------------------------------------------------------------------- d. mask semantics
SPECIALS = (0x00000000, 0x80000000 - (1 << 32), 0x00800000, 0x00000001, 0x007FFFFF, 0x80000001 - (1 << 32), 0x807FFFFF - (1 << 32))
KEEPS = (False, False, True, True, True, False, False)   # +0, -0, smallest normal, smallest and largest denormal, the negative denormals


@pytest.mark.parametrize("case", [CS.CASES[2], CS.CASES[16]], ids=CS.case_id)
def test_mask_is_greater_than_zero_as_ieee_defines_it(L, dev, case):
    """mask_src > 0 is false at +0 and -0 and at negative denormals and true at positive denormals and the smallest normal (no flush
    to zero in the comparison): the masked dx holds the unmasked call's bits where it is true and +0 elsewhere, on the generic and
    on the direct kernel."""
    cell, _ = plan(L, 1, case.shape)
    if DEFAULT_SWITCHES:
        assert cell == case.dgrad and cell in "GD"
    N, Cin, Cout, H, W = case.shape
    numel = N * Cin * H * W
    g = torch.Generator().manual_seed(numel)
    mask = torch.randn(numel, generator=g)
    reps = max(1, min(40, numel // (4 * len(SPECIALS))))
    where = torch.randperm(numel, generator=g)[:reps * len(SPECIALS)]
    bits = mask.view(torch.int32)
    bits[where] = torch.tensor(SPECIALS, dtype=torch.int32).repeat(reps)
    keep = bits > 0                                               # sign clear and not zero: > 0 for everything that is no NaN
    assert torch.equal(keep[where], torch.tensor(KEEPS).repeat(reps))
    plain = Call(L, dev, 1, case.shape).run()
    masked = Call(L, dev, 1, case.shape, mask=mask.to(dev)).run()
    assert not plain.problems and not masked.problems, (plain.problems, masked.problems)
    want = torch.where(keep, plain.out["dx"], torch.zeros(()))
    assert bool((plain.out["dx"][where] != 0).all()), "a planted position where dx is zero decides nothing"
    wrong = torch.nonzero(want.view(torch.int32) != masked.out["dx"].view(torch.int32)).flatten()
    print(f"{CS.case_id(case)} {cell}: {int(keep.sum())} of {numel} kept, {len(wrong)} wrong")
    assert len(wrong) == 0, [(int(i), hex(int(bits[i]) & 0xFFFFFFFF), float(plain.out["dx"][i]), float(masked.out["dx"][i]))
                             for i in wrong[:8]]


# ------------------------------------------------------------------------------------------------------- e. scratch fallbacks
def test_forward_and_data_gradient_fall_back_to_the_direct_kernel(L, dev):
    """A W4-planned layer handed scratch for the packed weights only - what the plan reserves for the same channels on a 224 map,
    which it never sizes for Winograd - runs the direct kernel in both passes; four bytes fewer are refused."""
    shape = CS.FALLBACK_W4.shape
    N, Cin, Cout, H, W = shape
    bad = []
    for ps in (0, 1):
        cell, planned_bytes = plan(L, ps, shape)
        _, packed = plan(L, ps, (N, Cin, Cout, 224, 224))
        assert packed == Cout * ((Cin + 3) // 4) * 36 * 4 and packed < planned_bytes
        if DEFAULT_SWITCHES:   # with the planned scratch the same call is the one Winograd GEMM: the zero below is the fallback's
            assert cell == "W4"
            full = Call(L, dev, ps, shape)
            assert full.run_profiled(FAMILY_WINO_GEMM) == 1 and not full.problems, full.problems
        small = Call(L, dev, ps, shape, scratch_bytes=packed)
        launches = small.run_profiled(FAMILY_WINO_GEMM)
        print(f"{CS.PASSES[ps]}: {packed} of {planned_bytes} bytes, {launches} Winograd GEMM launches, problems {small.problems}")
        assert launches == 0 and not small.problems, (launches, small.problems)
        bad += judge(f"fallback {CS.case_id(CS.FALLBACK_W4)} packed-only", ps, "D", shape, small.out)
        Call(L, dev, ps, shape, scratch_bytes=packed - 4).refused("weight scratch too small")
    assert not bad, bad


@pytest.mark.parametrize("case", [CS.FALLBACK_W4, CS.FALLBACK_D], ids=CS.case_id)
def test_weight_gradient_with_one_to_three_slabs(L, dev, case):
    """k * per_split bytes, per_split = (9 Cout Cin + Cout) * 4 (one [9][Cout][Cin] slab and its [Cout] bias row): the direct kernel
    with k splits, the bias rows carved behind the k slabs; less than one slab is refused."""
    N, Cin, Cout, H, W = case.shape
    per_split = (9 * Cout * Cin + Cout) * 4
    cell, planned_bytes = plan(L, 2, case.shape)
    if DEFAULT_SWITCHES:
        assert cell == case.wgrad
    assert 3 * per_split < planned_bytes
    bad = []
    for k in (1, 2, 3):
        c = Call(L, dev, 2, case.shape, scratch_bytes=k * per_split)
        launches = c.run_profiled(FAMILY_WINO_WGRAD_GEMM)
        print(f"{k} slabs: {launches} Winograd weight-gradient launches, problems {c.problems}")
        assert launches == 0 and not c.problems, (k, launches, c.problems)
        bad += judge(f"fallback {CS.case_id(case)} {k} slabs", 2, "D", case.shape, c.out)
    Call(L, dev, 2, case.shape, scratch_bytes=per_split - 4).refused("workspace too small")
    assert not bad, bad


@pytest.mark.parametrize("case", [CS.CASES[12], CS.FALLBACK_W4], ids=CS.case_id)
def test_forward_without_scratch_runs_the_generic_kernel(L, dev, case):
    """wpack = NULL, 0: a D-planned and a W4-planned forward run the generic gather kernel (the only one that needs no scratch); the
    data gradient needs the flipped weights and is refused."""
    c = Call(L, dev, 0, case.shape, scratch_bytes="null")
    launches = c.run_profiled(FAMILY_WINO_GEMM)
    assert launches == 0 and not c.problems, (launches, c.problems)
    bad = judge(f"fallback {CS.case_id(case)} no scratch", 0, "G", case.shape, c.out)
    Call(L, dev, 1, case.shape, scratch_bytes="null").refused("needs the weight scratch")
    assert not bad, bad
