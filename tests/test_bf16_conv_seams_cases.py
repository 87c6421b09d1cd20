"""The case table of tests/bf16_conv_seams.py against umpr_debug_conv_bf16_plan, without a GPU: every row's plan is what the row
names and the refusals are where the rows say; the table reaches every branch of the two launchers; the float32 CPU convolution is
the float64 one bit for bit on the integer inputs; on the random-valued rows the float32 CPU result passes the gates with the lax
share under its cap; and mutants of the CPU evaluation - what a subtly wrong kernel would compute - do not.  The plan is asked in a
child process, as tests/test_conv_seams_cases.py asks its own."""
import json
import subprocess
import sys

import pytest
import torch

import bf16_conv_seams as BS
import coattn_decisions as CD
import vgg_bf16_decisions as VB
from test_conv_plan import built_library

CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
plan = lib.umpr_debug_conv_bf16_plan
plan.restype, plan.argtypes = ctypes.c_int, [ctypes.c_int] * 6 + [ctypes.POINTER(ctypes.c_long)]
size = lib.umpr_conv3x3_bf16_ws_bytes
size.restype, size.argtypes = ctypes.c_size_t, [ctypes.c_int] * 5
lib.umpr_last_error.restype = ctypes.c_char_p
out = []
for n, ci, co, hw in json.loads(sys.argv[2]):
    row = {"ws": size(n, ci, co, hw, hw), "plans": []}
    for ps in (0, 1, 2):
        v = (ctypes.c_long * 10)(*([-7] * 10))
        rc = plan(ps, n, ci, co, hw, hw, v)
        row["plans"].append([rc, list(v), lib.umpr_last_error().decode() if rc else ""])
    out.append(row)
print(json.dumps(out))
"""
EXTRA = ((1, 64, 64, 16), (1, 64, 64, 15), (1, 48, 80, 14), (2, 100, 100, 28))     # refused by every pass


@pytest.fixture(scope="module")
def planned():
    shapes = [c.shape for c in BS.CASES] + list(EXTRA)
    out = subprocess.run([sys.executable, "-c", CHILD, built_library(), json.dumps(shapes)], check=True, stdout=subprocess.PIPE,
                         text=True, timeout=120).stdout
    return dict(zip(shapes, json.loads(out.strip().splitlines()[-1])))


def scratch_rule(ps, shape, splits=None):
    """the header's rule: packed weights for the forward and the data gradient, slabs and bias rows for the weight gradient"""
    _, Cin, Cout, _ = shape
    return Cin * Cout * 18 + 1024 if ps < 2 else splits * (9 * Cout * Cin + Cout) * 4 + 1024


@pytest.mark.parametrize("case", BS.CASES, ids=BS.case_id)
def test_row_is_planned_as_it_says(planned, case):
    got = planned[case.shape]
    need = 0
    for ps in (0, 1, 2):
        rc, v, err = got["plans"][ps]
        want = case[1 + ps]
        if want is None:
            assert rc < 0 and "must be multiples of" in err and v == [-7] * 10, (case.shape, BS.PASSES[ps], rc, v, err)
            continue
        assert rc == 0 and tuple(v[:8]) == tuple(want), (case.shape, BS.PASSES[ps], rc, v, want, case.what)
        assert v[8] == scratch_rule(ps, case.shape, want.splits if ps == 2 else None), (case.shape, BS.PASSES[ps], v[8])
        assert v[9] == (BS.NCIT.get(case.shape, 1) if ps == 2 else 0), (case.shape, v[9])
        need = max(need, v[8])
        if ps == 2:                                           # the row's own figures hang together
            assert want.last_segs == want.nseg - (want.splits - 1) * want.segs_per_split and 0 < want.last_segs <= want.segs_per_split
            assert want.blocks == -(-want.splits // 8) * 8 * want.ntiles and want.wide == (want.splits >= 32)
        else:
            assert want.blocks >= want.nct * want.ntp and want.chunks * 32 == (case.shape[2] if ps else case.shape[1])
    assert got["ws"] == -(-need // 1024) * 1024, (case.shape, got["ws"], need)      # what the passes that run need, no more


def test_shapes_off_the_kernels_are_refused_by_name(planned):
    for shape in EXTRA:
        for ps in (0, 1, 2):
            rc, v, err = planned[shape]["plans"][ps]
            word = "not a VGG16 map size" if shape[1] % 64 == 0 and shape[2] % 64 == 0 else "must be multiples of"
            assert rc < 0 and word in err and v == [-7] * 10, (shape, ps, rc, err)
        assert planned[shape]["ws"] >= shape[1] * shape[2] * 18 + 1024          # the size query itself survives them


def test_table_reaches_every_branch_of_the_launchers():
    assert len({c.shape for c in BS.CASES}) == len(BS.CASES)
    conv = [p for c in BS.CASES for p in (c.fwd, c.dgrad) if p is not None]
    rules = {(p.BN, p.interleaved) for p in conv}
    assert rules == {(bn, r) for bn in (64, 128, 256) for r in (0, 1)}, rules        # both grid rules under each BN
    assert {(p.two_d, p.pingpong) for p in conv} == {(0, 0), (0, 1), (1, 0), (1, 1)}
    assert all(p.pingpong == (p.BN != 64 and (p.BN == 256 or not p.two_d)) for p in conv)
    chunks = {p.chunks for p in conv}
    assert {1, 2, 3} <= chunks and max(chunks) > 3, chunks
    assert any(p.nct > 8 for p in conv) and any(p.interleaved and p.nct < 8 for p in conv)
    assert any(p.interleaved and p.ntp % 8 for p in conv), "no interleaved launch with a partly filled last round"
    assert any(p.interleaved and p.ntp > 8 for p in conv), "no interleaved launch with more than one round"
    # per pass: the forward and the data gradient each see the interleaved rule (the transposed pack feeds the second)
    assert any(c.fwd and c.fwd.interleaved for c in BS.CASES) and any(c.dgrad and c.dgrad.interleaved for c in BS.CASES)
    wg = [c.wgrad for c in BS.CASES if c.wgrad is not None]
    assert any(g.big and g.ntiles > 1 for g in wg) and any(not g.big and g.ntiles > 1 for g in wg)
    assert {g.wide for g in wg} == {0, 1}
    assert any(g.last_segs < g.segs_per_split for g in wg), "no short last split"
    assert any(g.splits == g.nseg and g.splits % 8 for g in wg), "no splits clipped to the segment count"
    assert any(g.blocks > g.splits * g.ntiles for g in wg), "no idle workgroups behind the last split"
    assert any(g.segs_per_split > 2 for g in wg) and any(g.segs_per_split == 1 for g in wg)
    assert 3 in BS.NCIT.values()
    # every map size; 2-D segments (224 / 112) on both wgrad tiles
    assert {c.shape[3] for c in BS.CASES} == {14, 28, 56, 112, 224}
    assert {(c.shape[3], c.wgrad.big) for c in BS.CASES if c.wgrad and c.shape[3] >= 112} >= {(224, 0), (112, 1)}
    assert all(c.shape[3] in (14, 28, 56) for c in BS.RANDOM_ROWS) and BS.SMALLEST in BS.RANDOM_ROWS and BS.INTERLEAVED in BS.RANDOM_ROWS
    assert BS.INTERLEAVED.fwd.interleaved and BS.INTERLEAVED.dgrad.interleaved and BS.INTERLEAVED.wgrad is not None


@pytest.mark.parametrize("case", BS.CASES, ids=BS.case_id)
def test_float32_is_float64_on_the_integer_inputs(case):
    """Every partial sum is an integer below 2^24: the float32 CPU convolution the GPU test compares with is the float64 one, bit
    for bit, and the outputs are overwhelmingly bf16-exact as they stand."""
    passes = tuple(BS.runs(case))
    ref = BS.reference(case.shape, "int", passes)
    for t in (ref["x"], ref["w"], ref["gy"]):
        assert float(t.abs().max()) == 2.0 and bool((t == t.round()).all()) and bool((t == 0).any())
    assert float(ref["b"].abs().max()) <= 8.0 and bool((ref["b"] == ref["b"].round()).all())
    r64 = BS.evaluate(ref["x"], ref["w"], ref["b"], ref["gy"], torch.float64, passes)
    for name, v in ref["r32"].items():
        assert torch.equal(v.double(), r64[name]), (case.shape, name)
        assert float(v.abs().max()) < 2.0 ** 24
        if name in ("e", "dx"):
            exact = float((VB.q(v) == v.double()).double().mean())
            assert exact >= 0.9, (case.shape, name, exact)
            if name == "e":
                assert bool((v < 0).any()) and bool((v > 0).any())


@pytest.mark.parametrize("case", BS.RANDOM_ROWS, ids=BS.case_id)
def test_float32_passes_the_gates_of_the_random_rows(case):
    """The yardstick itself is inside its own gates, and the interval gate is tight on all but LAX_CAP of the elements."""
    passes = tuple(BS.runs(case))
    ref = BS.reference(case.shape, "rnd", passes)
    for t in (ref["x"], ref["w"], ref["gy"]):
        assert torch.equal(VB.q(t), t.double()), "operands are not bf16-exact"
    assert float(ref["x"].min()) == 0.0
    for name, relu in (("e", True), ("dx", False)):
        if name not in ref["r32"]:
            continue
        m = BS.margin(ref, name)
        got = VB.q(torch.relu(ref["r32"][name]) if relu else ref["r32"][name])
        outside, lax = BS.interval_gate(got, ref["r64"][name], m, relu)
        print(f"{BS.case_id(case)} {name}: m = {m:.3e}, float32 outside {outside}, lax share {lax:.3e}")
        assert outside == 0 and lax <= BS.LAX_CAP, (case.shape, name, outside, lax)
        assert 0 < m < 2.0 ** -12 * float(ref["r64"][name].abs().max())
    if "dw" in ref["r32"]:
        names = ("dw", "db")
        ok, rows = CD.gate([ref["r32"][n] for n in names], [ref["r64"][n] for n in names], [ref["r32"][n] for n in names],
                           names=names, K=BS.K)
        assert ok and all(r["ratio"] <= 1.0 for r in rows), rows


def _outside(ref, kind, got):
    """{tensor: elements (forward, data gradient) or gate ratio (weight, bias gradient) by which `got` fails the row's gate; 0 = passes}"""
    out = {}
    for name, v in got.items():
        if kind == "int":
            want = ref["r32"][name]
            if name in ("e", "dx"):
                out[name] = BS.equal_gate(VB.q(torch.relu(v) if name == "e" else v), VB.q(torch.relu(want) if name == "e" else want))
            else:
                out[name] = BS.equal_gate(v, want)
        elif name in ("e", "dx"):
            relu = name == "e"
            out[name] = BS.interval_gate(VB.q(torch.relu(v) if relu else v), ref["r64"][name], BS.margin(ref, name), relu)[0]
        else:
            ok, rows = CD.gate([v], [ref["r64"][name]], [ref["r32"][name]], names=[name], K=BS.K)
            out[name] = 0 if ok else rows[0]["ratio"]
    return out


@pytest.mark.parametrize("kind", ["int", "rnd"])
@pytest.mark.parametrize("case", [BS.SMALLEST, BS.INTERLEAVED], ids=BS.case_id)
def test_mutants_of_the_cpu_evaluation_fail_the_gates(case, kind):
    """One input pixel dropped, one tap skipped, one output-channel tile fed the next tile's weights (where there is a next tile), the
    last pixel segment left out of the weight gradient, accumulation rounded to bf16 once per 32-channel chunk: each is outside the
    gate of every tensor it enters.  (The chunk-rounded forward is a mutant for the random-valued inputs only: the integer partial
    sums are bf16-exact, which is why those rows run both kinds.)"""
    ref = BS.reference(case.shape, kind, (0, 1, 2))
    clean = _outside(ref, kind, ref["r32"])
    assert not any(clean.values()), clean
    mutants = {"pixel dropped": BS.mutant_pixel_dropped(ref, (0, 1, 2)), "tap skipped": BS.mutant_tap_skipped(ref, (0, 1, 2)),
               "last segment left out": BS.mutant_last_segment_left_out(ref, case.wgrad.nseg)}
    if case.fwd.nct > 1:
        mutants["next tile's weights"] = BS.mutant_next_tiles_weights(ref, (0, 1), case.fwd.BN)
    if kind == "rnd":
        mutants["chunk rounded"] = BS.mutant_chunk_rounded(ref)
    for what, got in mutants.items():
        bad = _outside(ref, kind, got)
        print(f"{BS.case_id(case)} {kind} {what}: {bad}")
        assert got and all(v > 0 for v in bad.values()), (case.shape, kind, what, bad)
    if kind == "int":
        chunked = _outside(ref, kind, BS.mutant_chunk_rounded(ref))
        print(f"{BS.case_id(case)} int chunk rounded: {chunked}")
