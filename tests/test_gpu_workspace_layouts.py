"""The VGG feature entry points through the C ABI at exactly the workspace size they report, and the bf16 GEMM scope.

No other test calls umpr_vgg16_features_fwd/_bwd or their bf16 twins directly: the module reaches them with a pooled workspace that
may be larger than required.  Here the workspace is exactly `*_ws_bytes(n)` long, NaN-filled, with NaN guard bands in front of and
behind it and the activation arena; the 26 gradients must be finite, the guard bands untouched, and the gradients bit-identical
  * to the same call with a workspace one MiB larger than required (no kernel's result depends on the space it is given), and
  * between UMPR_WGRAD_STREAM unset (weight gradients on the library's side stream) and =0 (a straight line on the caller's
    stream).  The switch is read when the library loads, so the =0 run is a job of tools/run_gpu_children.py: the same test in a
    child process, which leaves its digests in the launcher's output directory for the comparison here.
"""
import hashlib
import json
import os

import pytest
import torch

from conftest import CHILDREN, child_result
from test_gpu_parity import L, dev   # noqa: F401  (fixtures: the library, the device)

pytestmark = pytest.mark.gpu

CHILD_DIGESTS = os.path.join(os.path.dirname(CHILDREN["rc"]), "vgg_features_digests_stream0.json")   # beside the jobs' logs
GUARD = 4096                      # floats in front of and behind every guarded buffer (16 KiB: the buffer keeps its alignment)
NAN_BITS = 0x7FC00000
MIB = 1 << 20
CFG = ((3, 64), (64, 64), (64, 128), (128, 128), (128, 256), (256, 256), (256, 256), (256, 512), (512, 512), (512, 512),
       (512, 512), (512, 512), (512, 512))
PATHS = {"fp32": ("umpr_vgg16_features_fwd", "umpr_vgg16_features_bwd", "umpr_vgg16_act_bytes", "umpr_vgg16_fwd_ws_bytes",
                  "umpr_vgg16_features_bwd_ws_bytes"),
         "bf16": ("umpr_vgg16_bf16_features_fwd", "umpr_vgg16_bf16_features_bwd", "umpr_vgg16_bf16_act_bytes",
                  "umpr_vgg16_bf16_fwd_ws_bytes", "umpr_vgg16_bf16_bwd_ws_bytes")}
CASES = [(path, n) for path in PATHS for n in (1, 3)]


class Guarded:
    """`nbytes` of NaN-filled device memory between two NaN guard bands"""

    def __init__(self, dev, nbytes):
        assert nbytes % 4 == 0
        self.n = nbytes // 4
        self.all = torch.full((self.n + 2 * GUARD,), float("nan"), device=dev)
        self.t = self.all[GUARD:GUARD + self.n]

    def guards_ok(self):
        bits = self.all.view(torch.int32)
        return bool((bits[:GUARD] == NAN_BITS).all()) and bool((bits[GUARD + self.n:] == NAN_BITS).all())


def _inputs(dev, n):
    g = torch.Generator().manual_seed(1234 + n)
    params = []
    for cin, cout in CFG:   # He initialisation keeps the activations' scale through the 13 layers
        params.append((torch.randn(cout, cin, 3, 3, generator=g) * (2.0 / (9 * cin)) ** 0.5).to(dev))
        params.append((torch.randn(cout, generator=g) * 0.01).to(dev))
    images = torch.randn(n, 3, 224, 224, generator=g).to(dev)
    d_pool5 = torch.randn(n, 25088, generator=g).to(dev)
    return params, images, d_pool5


def _run(L, dev, path, n, extra_bytes):
    """forward + backward on fresh guarded buffers; (problems, [sha256 of each of the 26 gradients])"""
    from umpr_amd.model import _ptr_array
    from umpr_amd._lib import stream_ptr
    fwd, bwd, act_bytes, fwd_ws_bytes, bwd_ws_bytes = PATHS[path]
    params, images, d_pool5 = _inputs(dev, n)
    grads = [torch.full_like(p, float("nan")) for p in params]
    keep_p, parr = _ptr_array(params + params[:6])
    keep_g, garr = _ptr_array(grads + grads[:6])
    acts = Guarded(dev, L.size(act_bytes, n))
    wf = Guarded(dev, L.size(fwd_ws_bytes, n) + extra_bytes)
    wb = Guarded(dev, L.size(bwd_ws_bytes, n) + extra_bytes)
    s = stream_ptr()
    if path == "fp32":
        L.call(fwd, images, parr, n, acts.t, wf.t, wf.n * 4, s)
    else:
        pool5 = Guarded(dev, n * 25088 * 4)
        L.call(fwd, images, parr, n, acts.t, pool5.t, wf.t, wf.n * 4, s)
    L.call(bwd, images, parr, n, acts.t, d_pool5, garr, wb.t, wb.n * 4, s)
    torch.cuda.synchronize()
    bad = [f"guard band of the {name} written" for name, b in (("activation arena", acts), ("forward workspace", wf),
                                                               ("backward workspace", wb)) if not b.guards_ok()]
    bad += [f"gradient {i} is not finite" for i, t in enumerate(grads) if not bool(torch.isfinite(t).all())]
    return bad, [hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest() for t in grads]


@pytest.fixture(scope="module")
def runs(L, dev):
    out = {}
    for path, n in CASES:
        out[f"{path}-{n}"] = {"exact": _run(L, dev, path, n, 0), "larger": _run(L, dev, path, n, MIB)}
        torch.cuda.empty_cache()
    if os.environ.get("UMPR_WGRAD_STREAM") == "0":   # the child job: leave the digests for the parent's comparison
        os.makedirs(os.path.dirname(CHILD_DIGESTS), exist_ok=True)
        with open(CHILD_DIGESTS, "w") as f:
            json.dump({k: v["exact"][1] for k, v in out.items()}, f)
    return out


@pytest.mark.parametrize("path,n", CASES)
def test_vgg_features_at_exact_workspace_size(runs, path, n):
    r = runs[f"{path}-{n}"]
    for size in ("exact", "larger"):
        print(f"{path} n={n} {size}: problems {r[size][0]}")
        assert not r[size][0], (size, r[size][0])
    differ = [i for i, (a, b) in enumerate(zip(r["exact"][1], r["larger"][1])) if a != b]
    assert len(r["exact"][1]) == 26 and not differ, f"gradients {differ} depend on the size of the workspace"


def test_vgg_feature_gradients_do_not_depend_on_the_wgrad_stream(runs):
    assert os.environ.get("UMPR_WGRAD_STREAM") is None, "run this comparison with UMPR_WGRAD_STREAM unset"
    rc, out = child_result("wgrad_stream0_check")
    assert rc == 0, out[-3000:]
    with open(CHILD_DIGESTS) as f:
        child = json.load(f)
    assert sorted(child) == sorted(runs)
    for key in sorted(runs):
        differ = [i for i, (a, b) in enumerate(zip(runs[key]["exact"][1], child[key])) if a != b]
        assert len(child[key]) == 26 and not differ, f"{key}: gradients {differ} differ between the two stream settings"


def test_bf16_gemm_scope_restores_the_callers_setting(L, dev):
    """A fused text call with b16_gemm=1 made while the host thread had set umpr_set_gemm_bf16(1) leaves the setting at 1: the
    next generic GEMM still rounds its operands to bf16.  A = all 1 + 2^-10 (rounds to 1 in bf16), B = ones, K = 32: exactly 32."""
    from umpr_amd.model import _ptr_array
    from umpr_amd._lib import stream_ptr
    B, S, Ln, E, vocab = 1, 1, 2, 4, 8
    g = torch.Generator().manual_seed(7)
    shapes = [(192, E), (192, 64), (192,), (192,), (192, E), (192, 64), (192,), (192,), (128, 128), (64, 128), (64,), (64, 128),
              (64,), (128, 256), (128, 256)]
    params = [(torch.randn(*s, generator=g) * 0.1).to(dev) for s in shapes]
    keep, parr = _ptr_array(params)
    emb = torch.randn(vocab, E, generator=g).to(dev)
    ids = torch.randint(0, vocab, (2 * B * S, Ln), generator=g).to(dev)
    lengths = torch.full((2 * B * S,), Ln, dtype=torch.int32, device=dev)
    order = torch.arange(2 * B * S, dtype=torch.int32, device=dev)
    arena = torch.empty(L.size("umpr_review_net_arena_bytes", B, S, Ln), dtype=torch.uint8, device=dev)
    ws_bytes = L.size("umpr_review_net_ws_bytes", B, S, Ln, E)
    ws = torch.empty(ws_bytes // 4 + 1, device=dev)
    out = torch.empty(B, 128, device=dev)
    A = torch.full((16, 32), 1.0 + 2.0 ** -10, device=dev)
    Bm = torch.ones(32, 16, device=dev)
    C = torch.zeros(16, 16, device=dev)
    L.fn["umpr_set_gemm_bf16"](1)
    try:
        rc = L.fn["umpr_review_net_fwd"](ids.data_ptr(), emb.data_ptr(), E, parr, lengths.data_ptr(), order.data_ptr(), B, S, Ln, 1, 0,
                                         0, arena.data_ptr(), out.data_ptr(), ws.data_ptr(), ws_bytes, stream_ptr())
        assert rc == 0, L.last_error()
        rc = L.fn["umpr_gemm_f32"](A.data_ptr(), 32, 0, Bm.data_ptr(), 16, 0, C.data_ptr(), 16, 16, 16, 32, None, 0, 0, 0, 1.0,
                                   None, 0, stream_ptr())
        assert rc == 0, L.last_error()
        torch.cuda.synchronize()
    finally:
        L.fn["umpr_set_gemm_bf16"](0)
    assert bool(torch.isfinite(out).all())
    print("C[0][0] =", float(C[0, 0]), "min", float(C.min()), "max", float(C.max()))
    assert bool((C == 32.0).all()), (float(C.min()), float(C.max()))
