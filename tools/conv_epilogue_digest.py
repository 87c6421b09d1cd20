"""usage: python tools/conv_epilogue_digest.py OUT.json
sha256 of what the direct fp32 conv kernels write for the shapes of tests/test_gpu_direct_conv_epilogue.py: forward (raw, +bias,
+bias+ReLU), data gradient and masked data gradient, on seeded inputs.  Run it on two builds of libumpr_hip.so and compare the
files: equal digests = byte-identical outputs (how a change to the kernels' prologue / epilogue is held against its parent)."""
import hashlib
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from umpr_amd._lib import lib  # noqa: E402

SHAPES = [(1, 8, 40, 224), (2, 8, 16, 112), (3, 8, 130, 28), (5, 12, 130, 28), (7, 6, 64, 14), (6, 8, 128, 112),
          (1, 40, 8, 224), (2, 16, 8, 112), (3, 130, 8, 28), (5, 130, 12, 28), (7, 64, 6, 14), (6, 128, 8, 112),
          (1, 64, 64, 224), (1, 64, 128, 112)]


def digest(t):
    torch.cuda.synchronize()
    return hashlib.sha256(t.cpu().numpy().tobytes()).hexdigest()


def main(out_path):
    L = lib()
    dev = torch.device("cuda:0")
    st = torch.cuda.current_stream().cuda_stream
    out = {}
    for N, Cin, Cout, HW in SHAPES:
        g = torch.Generator().manual_seed(1000 + N + Cin + Cout + HW)
        x = torch.randn(N, Cin, HW, HW, generator=g).to(dev)
        w = (torch.randn(Cout, Cin, 3, 3, generator=g) / (Cin * 9) ** 0.5).to(dev)
        b = torch.randn(Cout, generator=g).to(dev)
        gy = torch.randn(N, Cout, HW, HW, generator=g).to(dev)
        m = torch.randn(N, Cin, HW, HW, generator=g).to(dev)
        wt = torch.empty(L.size("umpr_conv3x3_pack_bytes", N, Cin, Cout, HW, HW) // 4, device=dev)
        key = f"{N},{Cin},{Cout},{HW}"
        plan = [L.fn["umpr_debug_conv3x3_plan"](ps, N, Cin, Cout, HW, HW, 0, None, None) for ps in (0, 1)]
        out[key + " plan fwd/dgrad"] = plan
        for name, bias, relu in (("fwd raw", None, 0), ("fwd bias", b, 0), ("fwd bias relu", b, 1)):
            y = torch.full((N, Cout, HW, HW), float("nan"), device=dev)
            L.call("umpr_conv3x3_fwd", x, w, bias, y, N, Cin, HW, HW, Cout, relu, wt, wt.numel() * 4, st)
            out[f"{key} {name}"] = digest(y)
        for name, mask in (("dgrad", None), ("dgrad mask", m)):
            dx = torch.full((N, Cin, HW, HW), float("nan"), device=dev)
            L.call("umpr_conv3x3_bwd_data", gy, w, mask, dx, N, Cin, HW, HW, Cout, wt, wt.numel() * 4, st)
            out[f"{key} {name}"] = digest(dx)
    with open(out_path, "w") as fh:
        json.dump(out, fh, indent=1, sort_keys=True)
    print(f"{len(out)} entries -> {out_path}")


if __name__ == "__main__":
    main(sys.argv[1])
