"""The case table of tests/conv_seams.py against umpr_conv3x3_plan, without a GPU: every case lands on the algorithm its row names
with no UMPR_* switch set, the table covers every kernel family and every template of the direct weight gradient, and the float64
reference's gradients agree with finite differences.  The plan is asked as tests/test_conv_plan.py asks it: in a child process
whose environment carries no UMPR_* variable (the switches are read once per process)."""
import json
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import conv_seams as CS
from test_conv_plan import built_library

CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
plan = lib.umpr_debug_conv3x3_plan
plan.restype, plan.argtypes = ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_size_t)] * 2
out = []
for n, ci, co, h, w in json.loads(sys.argv[2]):
    out.append([plan(ps, n, ci, co, h, w, 0, None, None) for ps in (0, 1, 2)])
print(json.dumps(out))
"""
ALL = CS.CASES + (CS.FALLBACK_W4,)


@pytest.fixture(scope="module")
def planned():
    """{shape: (forward, data gradient, weight gradient)} in the fixture's letters"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("UMPR_")}
    out = subprocess.run([sys.executable, "-c", CHILD, built_library(), json.dumps([c.shape for c in ALL])], env=env, check=True,
                         stdout=subprocess.PIPE, text=True, timeout=120).stdout
    letter = {v: k for k, v in CS.CODES.items()}
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "conv_plan.json")) as fh:
        assert json.load(fh)["codes"] == CS.CODES
    return {c.shape: tuple(letter[a] for a in row) for c, row in zip(ALL, json.loads(out.strip().splitlines()[-1]))}


@pytest.mark.parametrize("case", ALL, ids=CS.case_id)
def test_case_lands_on_the_algorithm_its_row_names(planned, case):
    assert planned[case.shape] == (case.fwd, case.dgrad, case.wgrad), (case.shape, case.what)


def test_table_covers_every_kernel_family(planned):
    assert len({c.shape for c in ALL}) == len(ALL)
    for i, ps in enumerate(CS.PASSES):
        got = {planned[c.shape][i] for c in CS.CASES}
        assert got >= CS.COVER[ps], (ps, sorted(CS.COVER[ps] - got))
    templates = [CS.segment(c.shape[4]) for c in CS.CASES if planned[c.shape][2] == "D"]
    assert set(templates) == CS.WGRAD_TEMPLATES, templates          # a direct weight gradient is one of the three, each is there
    for rc in CS.WGRAD_TEMPLATES:                                  # ... and at least once with a last segment that is not full
        assert any(CS.segment(c.shape[4]) == rc and c.shape[3] % rc[0] for c in CS.CASES if planned[c.shape][2] == "D"), rc
    # the first-layer weight gradient needs the (2,16) segment; the generic one is reached with one-row, whole-map and 32-wide segments
    assert all(CS.segment(c.shape[4]) == (2, 16) and c.shape[1] <= 3 for c in CS.CASES if planned[c.shape][2] == "C")
    generic = {CS.segment(c.shape[4]) for c in CS.CASES if planned[c.shape][2] == "G"}
    assert {(32, 1), (3, 9), (1, 32), (4, 7)} <= generic, generic
    # the wide reduce kernel: at least 32 segments, hence at least 32 splits by default
    n, _, _, h, w = CS.CASES[8].shape
    r, cw = CS.segment(w)
    assert planned[CS.CASES[8].shape][2] == "D" and n * -(-h // r) * -(-w // cw) >= 32
    assert planned[CS.FALLBACK_D.shape][2] == "D" and planned[CS.FALLBACK_W4.shape] == ("W4", "W4", "W4")


def test_gate_rejects_one_dropped_contribution():
    """What the GPU tests' gate (K_START x the float32 CPU distance, floor 2^-22) makes of a float32 result that is right but for one
    input pixel read as zero, or one weight tap skipped: every tensor that pixel or tap enters is outside, by orders of magnitude."""
    import coattn_decisions as CD
    shape = CS.CASES[2].shape
    ref = CS.reference(shape)
    x, w = ref["x"].clone(), ref["w"].clone()
    x[1, 3, 2, 1] = 0.0
    assert float(ref["x"][1, 3, 2, 1]) > 0
    z, _, dw, _ = CS.conv_and_grads(x, ref["w"], ref["b"], ref["gz"], torch.float32)
    w[65, 6, 2, 2] = 0.0
    _, dx, _, _ = CS.conv_and_grads(ref["x"], w, ref["b"], ref["gz"], torch.float32)
    names = ("y", "dw", "dx")
    ok, rows = CD.gate([torch.relu(z), dw, dx], [ref[n][0] for n in names], [ref[n][1] for n in names], names=names, K=CD.K_START)
    assert not ok and all(r["ratio"] > 100 * CD.K_START for r in rows), rows
    ok, rows = CD.gate([ref[n][1] for n in names], [ref[n][0] for n in names], [ref[n][1] for n in names], names=names, K=CD.K_START)
    assert ok and all(r["ratio"] <= 1.0 for r in rows), rows


@pytest.mark.parametrize("case", CS.CASES[:2], ids=CS.case_id)
def test_reference_gradients_against_finite_differences(case):
    """<gz, z> is linear in each of x, w and b, so a central difference in float64 is the derivative up to rounding: every element of
    the three gradients of the smallest case (and of the next one, which has more than one of everything)."""
    ref = CS.reference(case.shape)
    x, w, b, gz = (ref[k].double() for k in ("x", "w", "b", "gz"))
    loss = lambda x_, w_, b_: float((F.conv2d(x_, w_, b_, padding=1) * gz).sum())
    h = 2.0 ** -10
    for name, i in (("dx", 0), ("dw", 1), ("db", 2)):
        args = [x, w, b]
        got = ref[name][0]
        fd = torch.empty_like(got).flatten()
        for e in range(fd.numel()):
            hi, lo = args[i].clone().flatten(), args[i].clone().flatten()
            hi[e] += h
            lo[e] -= h
            up = loss(*(args[:i] + [hi.view_as(args[i])] + args[i + 1:]))
            down = loss(*(args[:i] + [lo.view_as(args[i])] + args[i + 1:]))
            fd[e] = (up - down) / (2 * h)
        scale = max(float(got.abs().max()), 1e-30)
        assert float((fd.view_as(got) - got).abs().max()) <= 1e-9 * scale + 1e-10, (name, case.shape)
        # the float32 yardstick is the same function: within float32 rounding of the reference
        assert float((ref[name][1].double() - got).abs().max()) <= 1e-5 * scale + 1e-7, (name, case.shape)
    assert torch.equal(ref["gz"] != 0, (ref["z"][0] > 0) & (CS.make_inputs(case.shape)[3] != 0))
    assert ref["x"].dtype == torch.float32 and float(ref["x"].min()) >= 0.0
