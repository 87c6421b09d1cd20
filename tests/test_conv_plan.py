"""umpr_conv3x3_plan (csrc/conv3x3.hip) is the one place that decides which kernels a pass of an fp32 3x3 convolution runs.
Its answers are pinned, without a GPU, to tests/golden/conv_plan.json: the decisions of the dispatch conditions as they stood
before the plan function existed, for the 13 VGG16 layers and the shapes of test_conv3x3, under UMPR_WINO_F4 = 2, 1 and 0.

The switches are read once per process, so each mode is evaluated in one child process whose environment carries no other
UMPR_* variable.  The child calls umpr_debug_conv3x3_plan (pure host arithmetic) for every row and pass; compared are the
algorithm and whether the layer keeps its transformed input (v_bytes != 0).  The scratch a pass reserves must never exceed what
the matching public size entry point returns for the same shape.  Every expectation comes from the fixture."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "umpr_amd", "libumpr_hip.so")
FIXTURE = os.path.join(ROOT, "tests", "golden", "conv_plan.json")
# (fixture column, pass code, inference flag) in the order the child answers
PASSES = (("fwd", 0, 0), ("fwd_inf", 0, 1), ("dgrad", 1, 0), ("wgrad", 2, 0))

CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
N, shapes, passes = json.loads(sys.argv[2])
plan = lib.umpr_debug_conv3x3_plan
plan.restype, plan.argtypes = ctypes.c_int, [ctypes.c_int] * 7 + [ctypes.POINTER(ctypes.c_size_t)] * 2
size = {}
for name in ("umpr_conv3x3_pack_bytes", "umpr_conv3x3_bwd_weight_ws_bytes"):
    size[name] = getattr(lib, name)
    size[name].restype, size[name].argtypes = ctypes.c_size_t, [ctypes.c_int] * 5
out = []
for ci, co, hw in shapes:
    row = {"pack": size["umpr_conv3x3_pack_bytes"](N, ci, co, hw, hw),
           "wgrad_ws": size["umpr_conv3x3_bwd_weight_ws_bytes"](N, ci, co, hw, hw), "plans": []}
    for ps, inf in passes:
        ws, v = ctypes.c_size_t(), ctypes.c_size_t()
        algo = plan(ps, N, ci, co, hw, hw, inf, ctypes.byref(ws), ctypes.byref(v))
        row["plans"].append([algo, ws.value, v.value])
    out.append(row)
print(json.dumps(out))
"""


def built_library():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return LIB


@pytest.fixture(scope="module")
def fixture():
    with open(FIXTURE) as fh:
        return json.load(fh)


@pytest.mark.parametrize("mode", ["2", "1", "0"])
def test_plan_matches_the_recorded_dispatch(fixture, mode):
    rows = fixture["modes"][mode]
    assert len(rows) == 34
    env = {k: v for k, v in os.environ.items() if not k.startswith("UMPR_")}
    env["UMPR_WINO_F4"] = mode
    spec = [fixture["N"], [[r["cin"], r["cout"], r["hw"]] for r in rows], [[ps, inf] for _, ps, inf in PASSES]]
    out = subprocess.run([sys.executable, "-c", CHILD, built_library(), json.dumps(spec)], env=env, check=True,
                         stdout=subprocess.PIPE, text=True, timeout=120).stdout
    got = json.loads(out.strip().splitlines()[-1])
    assert len(got) == len(rows)
    wrong = []
    for r, g in zip(rows, got):
        shape = (r["cin"], r["cout"], r["hw"])
        for (col, ps, inf), (algo, ws, v) in zip(PASSES, g["plans"]):
            if algo != fixture["codes"][r[col]]:
                wrong.append((shape, col, "algorithm", algo, r[col]))
            # the training forward and the weight gradient share the slot; no other pass names one
            keeps = bool(r["v"]) and col in ("fwd", "wgrad")
            if (v != 0) != keeps:
                wrong.append((shape, col, "v_bytes", v, r["v"]))
            limit = g["wgrad_ws"] if col == "wgrad" else g["pack"]
            if ws > limit:
                wrong.append((shape, col, "ws_bytes above the public size", ws, limit))
        if g["plans"][0][2] != g["plans"][3][2]:
            wrong.append((shape, "forward and weight gradient disagree on the slot's size", g["plans"][0][2], g["plans"][3][2]))
    assert not wrong, wrong
