"""The epilogue of the direct fp32 conv kernels (csrc/conv3x3.hip: igemm_epilogue, behind conv3x3_igemm_v2_kernel), bit for bit.

test_gpu_parity.py::test_conv3x3 holds these kernels to 2e-5 + 1e-5 |y| against the CPU convolution.  Here the part after
the main loop is pinned exactly, through the public entry points, against the kernel's own raw accumulator output:

    fwd(bias=None, relu=0)  = raw
    fwd(bias=b,    relu=0) == raw + b[co]            one fp32 add
    fwd(bias=b,    relu=1) == max(raw + b[co], 0)
    bwd_data(mask=m)       == where(m > 0, bwd_data(mask=None), 0)

compared as 32-bit patterns (the references are single IEEE operations, computed on the CPU).  The epilogue loads the bias and
the mask in batches ahead of their use, with clamped addresses for channels past Cout and pixels past the end, so every output
lies between two sentinel bands of 256 floats (one tile row) that must come back untouched, is pre-filled with NaN that must
all be overwritten, and the mask sits at the very end of its allocation.

Shapes (N, Cin, Cout, HW): the smallest that reach each instance <BM,BN,W> and each guard; umpr_debug_conv3x3_plan must
answer 2 (direct) for the pass a case runs.  The data gradient swaps the channel roles (its output channels are Cin, and 32
or more reduction channels on a 28 / 14 map go to Winograd), so it has mirrored shapes of its own.
  forward        (1,8,40,224)   <64,256,224>, Cout tail (40 of 64 rows)
                 (2,8,16,112)   <64,128,112>, Cout < 64, tiles straddle the two images
                 (3,8,130,28)   <128,128,28>, two channel tiles with a 2-row tail, 2352 pixels = 18.4 tiles
                 (5,12,130,28)  the same with 3 reduction stages and 30.6 pixel tiles
                 (7,6,64,14)    <64,128,14>, full channel tile, 1372 pixels = 10.7 tiles
                 (6,8,128,112)  588 pixel tiles: <128,128,112> on 512 of them, then the <128,64,112> tail kernel on 76
  data gradient  (1,40,8,224)   <64,256,224> with 40 output channels from 2 reduction stages
                 (1,8,40,224) (2,16,8,112) (6,8,128,112): 8 output channels, <64,256,224> / <64,128,112>
                 (3,130,8,28) (5,130,12,28) (7,64,6,14) (6,128,8,112): the forward's instances with the roles swapped
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

BAND = 256          # sentinel floats in front of and behind every output: one row of the widest pixel tile
DIRECT = 2          # ConvAlgo CONV_DIRECT

FWD_SHAPES = [(1, 8, 40, 224), (2, 8, 16, 112), (3, 8, 130, 28), (5, 12, 130, 28), (7, 6, 64, 14), (6, 8, 128, 112)]
DGRAD_SHAPES = [(1, 40, 8, 224), (1, 8, 40, 224), (2, 16, 8, 112), (6, 8, 128, 112), (3, 130, 8, 28), (5, 130, 12, 28),
                (7, 64, 6, 14), (6, 128, 8, 112)]


@pytest.fixture(scope="module")
def L():
    from umpr_amd._lib import lib
    return lib()


@pytest.fixture(scope="module")
def dev():
    assert torch.cuda.is_available()
    return torch.device("cuda:0")


def st():
    return torch.cuda.current_stream().cuda_stream


@pytest.fixture(autouse=True)
def poison_lds(L, dev):
    """NaN in LDS before every test: a patch slot the staging never wrote would show up in the output."""
    sink = torch.zeros(1, dtype=torch.int32, device=dev)
    L.call("umpr_debug_poison_lds", sink, st())
    yield


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Banded:
    """A NaN-filled output tensor between two sentinel bands."""
    SENTINEL = 0x7FC0BEEF   # a quiet NaN with a payload

    def __init__(self, shape, dev):
        n = 1
        for d in shape:
            n *= d
        self.buf = torch.full((n + 2 * BAND,), self.SENTINEL, dtype=torch.int32, device=dev).view(torch.float32)
        self.out = self.buf[BAND:BAND + n].view(shape)
        self.out.fill_(float("nan"))

    def result(self, name):
        torch.cuda.synchronize()
        b = self.buf.view(torch.int32)
        front, back = b[:BAND].cpu(), b[-BAND:].cpu()
        assert bool((front == self.SENTINEL).all()), f"{name}: wrote in front of the output"
        assert bool((back == self.SENTINEL).all()), f"{name}: wrote behind the output"
        out = self.out.cpu()
        assert not torch.isnan(out).any(), f"{name}: {int(torch.isnan(out).sum())} outputs never written (or NaN)"
        return out


def at_the_end(t, dev):
    """A device copy of t whose last element is the last element of its allocation."""
    buf = torch.empty(t.numel() + 64, dtype=t.dtype, device=dev)
    view = buf[64:].view(t.shape)
    view.copy_(t)
    return view


def same_bits(name, got, ref):
    bad = bits(got) != bits(ref)
    assert not bool(bad.any()), f"{name}: {int(bad.sum())}/{bad.numel()} outputs differ in their bits, first at " \
                                f"{[int(i) for i in bad.nonzero()[0]]}"


def inputs(N, C, Co, HW, seed):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(N, C, HW, HW, generator=g)
    w = torch.randn(Co, C, 3, 3, generator=g) / (C * 9) ** 0.5
    return g, x, w


@pytest.mark.parametrize("N,Cin,Cout,HW", FWD_SHAPES)
def test_forward_epilogue_is_one_add_and_one_max(L, dev, N, Cin, Cout, HW):
    assert L.fn["umpr_debug_conv3x3_plan"](0, N, Cin, Cout, HW, HW, 0, None, None) == DIRECT
    g, x, w = inputs(N, Cin, Cout, HW, 11 * N + Cin + Cout + HW)
    b = torch.randn(Cout, generator=g)
    xd, wd, bd = x.to(dev), w.to(dev), at_the_end(b, dev)
    wt = torch.empty(L.size("umpr_conv3x3_pack_bytes", N, Cin, Cout, HW, HW) // 4, device=dev)
    got = {}
    for name, bias, relu in (("raw", None, 0), ("bias", bd, 0), ("bias+relu", bd, 1), ("relu", None, 1)):
        y = Banded((N, Cout, HW, HW), dev)
        L.call("umpr_conv3x3_fwd", xd, wd, bias, y.out, N, Cin, HW, HW, Cout, relu, wt, wt.numel() * 4, st())
        got[name] = y.result(f"fwd {name} {N},{Cin},{Cout},{HW}")
    raw = got["raw"]
    assert float(raw.abs().max()) > 0.1            # a real convolution, not zeros
    plus = raw + b[None, :, None, None]
    same_bits("bias", got["bias"], plus)
    same_bits("bias+relu", got["bias+relu"], torch.clamp_min(plus, 0.0))
    same_bits("relu", got["relu"], torch.clamp_min(raw, 0.0))


@pytest.mark.parametrize("N,Cin,Cout,HW", DGRAD_SHAPES)
def test_data_gradient_mask_is_one_select(L, dev, N, Cin, Cout, HW):
    assert L.fn["umpr_debug_conv3x3_plan"](1, N, Cin, Cout, HW, HW, 0, None, None) == DIRECT
    g, gy, wt_ = inputs(N, Cout, Cin, HW, 13 * N + Cin + Cout + HW)
    w = wt_.transpose(0, 1).contiguous()           # the parameter [Cout][Cin][3][3]
    m = torch.randn(N, Cin, HW, HW, generator=g)
    m[torch.rand(m.shape, generator=g) < 0.25] = 0.0                      # exact zeros (both signs) mask like negatives
    m[torch.rand(m.shape, generator=g) < 0.05] = -0.0
    gyd, wd, md = gy.to(dev), w.to(dev), at_the_end(m, dev)
    wt = torch.empty(L.size("umpr_conv3x3_pack_bytes", N, Cin, Cout, HW, HW) // 4, device=dev)
    got = {}
    for name, mask in (("raw", None), ("masked", md)):
        dx = Banded((N, Cin, HW, HW), dev)
        L.call("umpr_conv3x3_bwd_data", gyd, wd, mask, dx.out, N, Cin, HW, HW, Cout, wt, wt.numel() * 4, st())
        got[name] = dx.result(f"dgrad {name} {N},{Cin},{Cout},{HW}")
    raw = got["raw"]
    assert float(raw.abs().max()) > 0.1
    assert 0.3 < float((m > 0).float().mean()) < 0.5
    same_bits("masked", got["masked"], torch.where(m > 0, raw, torch.zeros_like(raw)))
