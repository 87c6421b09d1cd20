"""Host-side contracts of libumpr_hip.so that hold without a GPU: the workspace-size entry points return what they returned
before the A/B kernel variants were retired, and no retired environment switch is left in the built library.

The four size functions are pure host arithmetic (no HIP call).  Several of the switches they consult are read once, when the
library loads or at the first call, so they are evaluated in ONE child process whose environment carries no UMPR_* variable;
every test below reads that child's answer.  The expected numbers were recorded from the build of the commit before the
retirement, never from the code under test.

Since every workspace got one layout function that its size entry point and its user share, EVERY size_t entry point of the
header that takes only integers is pinned the same way (CASES below), to tests/golden/cabi_sizes.json: recorded from the
build of the commit before that restructuring, once with no UMPR_* variable and once under each of three settings the layouts
consult: UMPR_WINO_F4=0 and =1, which change sizes, and UMPR_EMB_GATHER=0, which changes the GRU's carving but must not change
its size (the size always takes E rounded up to 4)."""
import json
import os
import subprocess
import sys

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIB = os.path.join(ROOT, "umpr_amd", "libumpr_hip.so")

GRU_N = (1, 16, 17, 64, 65)          # both sides of the 16-sequence tile and of the retired 64-sequence one
GRU_L = 5
# (Cin, Cout, H = W) of the 13 VGG16 conv layers
VGG = ((3, 64, 224), (64, 64, 224), (64, 128, 112), (128, 128, 112), (128, 256, 56), (256, 256, 56), (256, 256, 56),
       (256, 512, 28), (512, 512, 28), (512, 512, 28), (512, 512, 14), (512, 512, 14), (512, 512, 14))

EXPECTED = {
    "umpr_embed_gru_bidir_ws_bytes": {      # by E, over GRU_N
        "50": [10413584, 10544384, 10654480, 11267072, 11377168],
        "300": [59558256, 59763456, 59878512, 60724224, 60839280],
    },
    "umpr_conv3x3_pack_bytes": {            # by batch, over VGG
        "1": [9216, 147456, 39846144, 53477632, 24117504, 33554688, 33554688, 33030912, 56623872, 56623872, 56623872,
              56623872, 56623872],
        "3": [9216, 147456, 116916480, 156238080, 61866240, 83886336, 83886336, 47187200, 75498752, 75498752, 56623872,
              56623872, 56623872],
    },
    "umpr_conv3x3_bwd_weight_ws_bytes": {
        "1": [3670016, 75628544, 28318976, 40115456, 18878720, 28315904, 28315904, 33034496, 56627456, 56627456, 25170176,
              25170176, 25170176],
        "3": [3670016, 75628544, 77876480, 110906624, 44837120, 66070784, 66070784, 47194368, 75505920, 75505920, 33562880,
              33562880, 33562880],
    },
    # the bf16 entry points take the 12 layers with Cin >= 64 (conv1_1 has kernels of its own: umpr_conv1_bf16_*)
    "umpr_conv3x3_bf16_ws_bytes": {
        "1": [None, 29543424, 31021056, 61986816, 30698496, 61369344, 61369344, 33045504, 66075648, 66075648, 18879488,
              18879488, 18879488],
        "3": [None, 35009536, 44610560, 59625472, 46047232, 61369344, 61369344, 47207424, 66075648, 66075648, 56636416,
              56636416, 56636416],
    },
}

RETIRED_SWITCHES = ("UMPR_GRU_V1", "UMPR_MERGE_DX", "UMPR_B16_M16", "UMPR_B16_ABL", "UMPR_B16_D", "UMPR_B16_CFG",
                    "UMPR_B16_T64", "UMPR_B16_T3", "UMPR_B16_PP", "UMPR_WINO_DMA", "UMPR_WINO_CHUNK_MB")

CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
gru_n, gru_l, vgg = json.loads(sys.argv[2])
out = {}
f = lib.umpr_embed_gru_bidir_ws_bytes
f.restype, f.argtypes = ctypes.c_size_t, [ctypes.c_int] * 3
out["umpr_embed_gru_bidir_ws_bytes"] = {str(E): [f(N, gru_l, E) for N in gru_n] for E in (50, 300)}
for name in ("umpr_conv3x3_pack_bytes", "umpr_conv3x3_bwd_weight_ws_bytes", "umpr_conv3x3_bf16_ws_bytes"):
    g = getattr(lib, name)
    g.restype, g.argtypes = ctypes.c_size_t, [ctypes.c_int] * 5
    bf16 = name == "umpr_conv3x3_bf16_ws_bytes"
    out[name] = {str(N): [None if bf16 and ci < 64 else g(N, ci, co, h, h) for ci, co, h in vgg] for N in (1, 3)}
print(json.dumps(out))
"""


def built_library():
    if not os.path.exists(LIB):
        import __graft_entry__ as g
        g.build()
    return LIB


@pytest.fixture(scope="module")
def sizes():
    env = {k: v for k, v in os.environ.items() if not k.startswith("UMPR_")}
    out = subprocess.run([sys.executable, "-c", CHILD, built_library(), json.dumps([GRU_N, GRU_L, VGG])], env=env,
                         check=True, stdout=subprocess.PIPE, text=True, timeout=120).stdout
    return json.loads(out.strip().splitlines()[-1])


@pytest.mark.parametrize("name", sorted(EXPECTED))
def test_workspace_sizes_are_what_they_were(sizes, name):
    assert sizes[name] == EXPECTED[name], name


# ---- every integer-only size_t entry point -----------------------------------------------------------------------------------
BS = (1, 3, 4, 5)
SL_PAIRS = ((1, 1), (7, 9), (8, 8), (5, 13), (10, 20))         # S * L = 1, 63, 64, 65, 200: both sides of the 64-wide score tile
SNET = ((3, 1, 5), (1, 4, 5), (5, 1, 5), (2, 2, 1), (4, 2, 7))  # B * S = 3, 4, 5 (four sentences per workgroup), 4, 8
R_SHAPES = ((5, 3, 17), (4, 4, 16), (1, 1, 257))               # B * S * L = 255, 256, 257: the C-Net's cdiv(R, 256)
ES = (49, 50, 300)                                             # 49: not a multiple of 4
N_IMG = (1, 2, 3, 64)
CTRL = tuple((B, s_ui, l_ui, S, L) for B in BS for (s_ui, l_ui), (S, L) in (((1, 1), (7, 9)), ((10, 20), (5, 13)), ((8, 8), (8, 8))))
CASES = {
    "umpr_embed_gru_bidir_ws_bytes": [(N, GRU_L, E) for E in ES for N in GRU_N],
    "umpr_coattention_fwd_ws_bytes": [(B, S * L) for B in BS for S, L in SL_PAIRS],
    "umpr_coattention_bwd_ws_bytes": [(B, S * L) for B in BS for S, L in SL_PAIRS],
    "umpr_snet_bwd_ws_bytes": list(SNET),
    "umpr_review_merge_bwd_ws_bytes": [(B,) for B in BS],
    "umpr_cnet_head_fwd_ws_bytes": [(B, 2, 5, KS) for B in BS for KS in (1, 2, 4)],
    "umpr_cnet_head_bwd_ws_bytes": [r + (KC, KS, V) for r in R_SHAPES for KC in (4, 100) for KS in (1, 2, 4) for V in (1, 4)],
    "umpr_control_gate_bwd_ws_bytes": [(B,) for B in BS],
    "umpr_review_net_arena_bytes": [(B, S, L) for B in BS for S, L in SL_PAIRS],
    "umpr_review_net_ws_bytes": [(B, S, L, E) for B in BS for S, L in SL_PAIRS for E in ES],
    "umpr_control_net_arena_bytes": [c + (KC, V) for c in CTRL for KC in (4, 100) for V in (1, 4)],
    "umpr_control_net_ws_bytes": [c + (E, KC, KS, V) for c in CTRL for E in ES for KC in (4, 100) for KS in (1, 2, 4)
                                  for V in (1, 4)],
    "umpr_conv3x3_pack_bytes": [(N, ci, co, h, h) for N in (1, 3) for ci, co, h in VGG],
    "umpr_conv3x3_bwd_weight_ws_bytes": [(N, ci, co, h, h) for N in (1, 3) for ci, co, h in VGG],
    "umpr_conv3x3_bf16_ws_bytes": [(N, ci, co, h, h) for N in (1, 3) for ci, co, h in VGG[1:]],
    "umpr_bf16_tensor_bytes": [(N, c, h, h) for N in (1, 3) for c in (8, 64) for h in (7, 14, 224)],
    "umpr_photo_store_slot_bytes": [(224, 224), (32, 33), (512, 512), (7, 5)],
}
for _name in ("umpr_vgg16_act_bytes", "umpr_vgg16_fwd_ws_bytes", "umpr_vgg16_ws_bytes", "umpr_vgg16_pool5_offset",
              "umpr_vgg16_classifier_bwd_ws_bytes", "umpr_vgg16_features_bwd_ws_bytes", "umpr_vgg16_cls_arena_bytes",
              "umpr_vgg16_bf16_act_bytes", "umpr_vgg16_bf16_fwd_ws_bytes", "umpr_vgg16_bf16_bwd_ws_bytes"):
    CASES[_name] = [(n,) for n in N_IMG]
CASES["umpr_grad_norm_ws_bytes"] = [()]
CASES = {k: list(dict.fromkeys(v)) for k, v in CASES.items()}   # (VGG16 repeats layer shapes)
CONFIGS = {"default": {}, "emb_gather_0": {"UMPR_EMB_GATHER": "0"}, "wino_f4_0": {"UMPR_WINO_F4": "0"},
           "wino_f4_1": {"UMPR_WINO_F4": "1"}}
GOLDEN = os.path.join(ROOT, "tests", "golden", "cabi_sizes.json")

ALL_CHILD = r"""
import ctypes, json, sys
lib = ctypes.CDLL(sys.argv[1])
out = {}
for name, calls in json.load(open(sys.argv[2])).items():
    f = getattr(lib, name)
    f.restype = ctypes.c_size_t
    out[name] = {}
    for args in calls:
        f.argtypes = [ctypes.c_int] * len(args)
        out[name][",".join(map(str, args))] = f(*args)
print(json.dumps(out))
"""


def all_sizes(lib, extra_env, tmp_dir):
    """{entry point: {"a,b,...": bytes}} for CASES, from one child process without UMPR_* variables other than extra_env"""
    env = {k: v for k, v in os.environ.items() if not k.startswith("UMPR_")}
    env.update(extra_env)
    spec = os.path.join(str(tmp_dir), "cases.json")
    with open(spec, "w") as fh:
        json.dump(CASES, fh)
    out = subprocess.run([sys.executable, "-c", ALL_CHILD, lib, spec], env=env, check=True, stdout=subprocess.PIPE,
                         text=True, timeout=120).stdout
    return json.loads(out.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def golden():
    with open(GOLDEN) as fh:
        return json.load(fh)


@pytest.mark.parametrize("config", sorted(CONFIGS))
def test_every_size_entry_point_returns_what_the_parent_build_returned(golden, config, tmp_path):
    got = all_sizes(built_library(), CONFIGS[config], tmp_path)
    want = golden[config]
    assert sorted(got) == sorted(want) == sorted(CASES)
    for name in sorted(CASES):
        assert list(got[name]) == [",".join(map(str, a)) for a in CASES[name]] == list(want[name]), name
        wrong = {k: (got[name][k], want[name][k]) for k in want[name] if got[name][k] != want[name][k]}
        assert not wrong, (config, name, wrong)


def test_no_retired_switch_is_in_the_built_library():
    """A retired name must not survive as a NUL-terminated string: a stale variable in a shell can then select nothing."""
    blob = open(built_library(), "rb").read()
    present = sorted(n for n in RETIRED_SWITCHES if n.encode() + b"\x00" in blob)
    assert not present, present
