"""umpr_gemm_f32 - the kernel every GEMM-shaped piece runs on - at the edges tests/test_gpu_parity.py::test_gemm never varies: padded
and odd row pitches, operands one float past an aligned base, a C with ldc > N, K = 0 and every stage / chain-fold edge of K, the
whole epilogue (act x bias_mode x accumulate x alpha, unsplit and through splitk_reduce_kernel), split-K workspaces of every size
down to none, all four tiles, the unsplit 128 x 128 tile, and the one- to four-stage products of the bf16 mode's two-stage pipeline.

The reference is the float64 product with the epilogue in float64 (of the bf16-rounded operands under umpr_set_gemm_bf16(1)); a
result is held to K x the distance the float32 CPU product + epilogue has from it (coattn_decisions.gate: K = 4, floor 2^-22).
Operand padding is NaN (a read of it would show), C is NaN where the call must write (or holds the addend under accumulate) and
carries a sentinel bit pattern in its gap columns and in a band behind its last row that must come back bit-identical; workspaces
are NaN-filled with a guard band behind ws_bytes.  Every row is logged to gemm_edges.log before anything is judged.
"""
import os

import pytest
import torch

import classifier_reference as CR
from test_gpu_parity import LOG as PARITY_LOG
from test_gpu_parity import L, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "gemm_edges.log")
GUARD = 4096                       # floats behind C's last row and behind ws_bytes
SENTINEL = 0x7FC12345              # a NaN with a payload: gap columns and the band behind C, compared as bits
LAYOUTS = [(0, 0), (0, 1), (1, 0), (1, 1)]
# gate factors above K_START: ceil(1.25 x worst measured ratio), see profiles/r06_a_classifier_gemm_gates.txt.  Empty: none needed.
K_OF = {}
ACTS = {0: lambda v: v, 1: torch.relu, 2: torch.tanh, 3: torch.sigmoid}


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


def _operand(dev, g, rows, rowlen, pad, off):
    """(the logical matrix on the CPU, its device image: NaN-filled, row pitch rowlen + pad, based `off` floats past the allocation)"""
    m = torch.randn(rows, rowlen, generator=g)
    ld = max(rowlen + pad, 1)
    flat = torch.full((off + max(rows, 1) * ld + 4,), float("nan"), device=dev)
    if rows * rowlen:
        flat[off:off + rows * ld].view(rows, ld)[:, :rowlen] = m.to(dev)
    return m, flat, flat[off:], ld


class _Rows:
    def __init__(self):
        self.rows, self.fails = [], []

    def judge(self):
        bad = [(r["name"], r["d_max"], r["r_max"], r["ratio"]) for r in self.rows if not r["ok"]]
        assert not self.fails and not bad, (self.fails, bad)


def _gemm(L, dev, R, M, N, K, ta, tb, *, pad_a=0, pad_b=0, pad_c=0, off=0, bias_mode=1, act=0, acc=0, alpha=1.0, ws_bytes=None,
          b16=False, exact=False):
    """One call and its verdict into R.  ws_bytes None: no workspace (never split); else a NaN-filled workspace of exactly that size."""
    tag = (f"{'b16' if b16 else 'f32'} M{M} N{N} K{K} ta{ta} tb{tb} pad{pad_a}/{pad_b}/{pad_c} off{off} bias{bias_mode} act{act} "
           f"acc{acc} alpha{alpha:g} ws{'-' if ws_bytes is None else ws_bytes}")
    g = torch.Generator().manual_seed(M * 7 + N * 3 + K + 11 * ta + 13 * tb)
    A, _, Ad, lda = _operand(dev, g, K if ta else M, M if ta else K, pad_a, off)
    B, _, Bd, ldb = _operand(dev, g, N if tb else K, K if tb else N, pad_b, off)
    assert (Ad.data_ptr() % 16 == 0) == (off == 0) and (Bd.data_ptr() % 16 == 0) == (off == 0)
    bias = torch.randn(M if bias_mode == 2 else N, generator=g)
    C0 = torch.randn(M, N, generator=g)
    ldc = N + pad_c
    cbits = torch.full((M * ldc + GUARD,), SENTINEL, dtype=torch.int32, device=dev)
    Cd = cbits.view(torch.float32)
    Cv = Cd[:M * ldc].view(M, ldc)
    Cv[:, :N] = C0.to(dev) if acc else float("nan")
    wsd = None
    if ws_bytes is not None:
        wsd = torch.full((ws_bytes + 4 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)      # 0xFFFFFFFF is a NaN
    bd = bias.to(dev) if bias_mode else None
    L.call("umpr_set_gemm_bf16", int(b16))
    try:
        L.call("umpr_gemm_f32", Ad, lda, ta, Bd, ldb, tb, Cd, ldc, M, N, K, bd, bias_mode, act, acc,
               alpha, wsd, ws_bytes or 0, st())
    finally:
        L.call("umpr_set_gemm_bf16", 0)
    torch.cuda.synchronize()
    got = Cv[:, :N].cpu()
    if not (bool((cbits[:M * ldc].view(M, ldc)[:, N:] == SENTINEL).all()) and bool((cbits[M * ldc:] == SENTINEL).all())):
        R.fails.append(f"{tag}: a gap column of C or the band behind it was written")
    if wsd is not None and not bool((wsd[ws_bytes:] == 0xFF).all()):
        R.fails.append(f"{tag}: written behind ws_bytes")
    if bool(torch.isnan(got).any()):
        R.fails.append(f"{tag}: NaN in C")
    rnd = CR.bf16_round if b16 else (lambda t: t)
    opA, opB = rnd(A.t() if ta else A), rnd(B.t() if tb else B)

    def epilogue(prod, dt):
        v = alpha * prod
        if bias_mode:
            v = v + (bias.to(dt)[:, None] if bias_mode == 2 else bias.to(dt))
        if acc:
            v = v + C0.to(dt)
        return ACTS[act](v)

    ref = epilogue(opA.double() @ opB.double(), torch.float64)
    ref32 = epilogue(opA.float() @ opB.float(), torch.float32)
    name = "gemm bf16" if b16 else "gemm f32"
    R.rows += CR.gate([got], [ref], [ref32], names=[name], K=K_OF.get(name, CR.K_START), log=log, tag=tag)[1]
    if exact and not torch.equal(got, ref32):
        R.fails.append(f"{tag}: not exactly act(bias + (accumulate ? C : 0))")


# ------------------------------------------------------------------------------------------------------- 1. strides and alignment
@pytest.mark.parametrize("b16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_strides_and_alignment(L, dev, ta, tb, b16):
    """M, N = 65 / 129 at K = 50 (no extent a multiple of 4: the scalar loads whatever the pitch) and 68 / 132 at K = 52 (every
    extent a multiple of 4: the float4 loads wherever pitch and base allow them): row pitches of the row length + 4 and + 1, both
    operands one float past an aligned allocation (the float4 path must switch itself off), and ldc = N + 3 with a sentinel in the
    gap columns and behind the last row - unsplit, and split (K + 512, with a workspace)."""
    R = _Rows()
    for M, N, K in ((65, 129, 50), (129, 65, 50), (68, 132, 52), (132, 68, 52)):
        kw = dict(ta=ta, tb=tb, b16=b16)
        _gemm(L, dev, R, M, N, K, pad_a=4, pad_b=4, **kw)
        _gemm(L, dev, R, M, N, K, pad_a=1, pad_b=1, **kw)
        _gemm(L, dev, R, M, N, K, pad_a=4, pad_b=0, pad_c=3, **kw)
        _gemm(L, dev, R, M, N, K + 512, pad_a=0, pad_b=4, pad_c=3, ws_bytes=8 * M * N * 4, **kw)
        if K % 4 == 0:
            _gemm(L, dev, R, M, N, K, off=1, **kw)
            _gemm(L, dev, R, M, N, K, off=1, pad_a=4, pad_b=4, pad_c=3, **kw)
    R.judge()


# ------------------------------------------------------------------------------------------------------- 2. K edges
K_EDGES = (0, 1, 15, 16, 17, 31, 32, 33, 127, 128, 129, 2047, 2048, 2049)


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_k_edges_f32(L, dev, ta, tb):
    """M = 70, N = 40 at every stage edge (BK = 16), the chain fold (KFLUSH * BK = 128) and many folds, without a workspace and -
    from K = 2047 on - split over one.  K = 0 gives exactly act(bias + (accumulate ? C : 0))."""
    R = _Rows()
    for K in K_EDGES:
        _gemm(L, dev, R, 70, 40, K, ta, tb, act=1, exact=K == 0)
        _gemm(L, dev, R, 70, 40, K, ta, tb, act=1, acc=1, bias_mode=2, alpha=-0.5, exact=K == 0)
        _gemm(L, dev, R, 70, 40, K, ta, tb, act=2, acc=1, bias_mode=0, alpha=-0.5)
        if K >= 2047:
            _gemm(L, dev, R, 70, 40, K, ta, tb, act=1, ws_bytes=16 * 70 * 40 * 4)
    R.judge()


@pytest.mark.parametrize("ta,tb", LAYOUTS)
def test_k_edges_bf16_pipeline(L, dev, ta, tb):
    """bf16 mode: K = 1 .. 49 gives nt = 1, 2, 3, 4 stages of the two-stage pipeline (separate code for each of the first three),
    with ragged M and N on one and on several tiles; K = 0 as in fp32."""
    R = _Rows()
    for K in (0, 1, 16, 17, 32, 33, 48, 49):
        for M, N in ((70, 40), (33, 130)):
            _gemm(L, dev, R, M, N, K, ta, tb, b16=True, exact=K == 0)
        _gemm(L, dev, R, 70, 40, K, ta, tb, b16=True, act=1, acc=1, bias_mode=2, alpha=-0.5, exact=K == 0)
    R.judge()


# ------------------------------------------------------------------------------------------------------- 3. epilogue
@pytest.mark.parametrize("b16", [False, True], ids=["f32", "bf16"])
@pytest.mark.parametrize("act", [0, 1, 2, 3], ids=["none", "relu", "tanh", "sigmoid"])
def test_epilogue(L, dev, act, b16):
    """act x bias_mode 0..2 x accumulate x alpha in {1, -0.5}: in the kernel's own epilogue (K = 40) and in splitk_reduce_kernel
    (K = 1000 with a workspace: bias[m], accumulate and the activation behind the slab sum)."""
    R = _Rows()
    for bias_mode in (0, 1, 2):
        for acc in (0, 1):
            for alpha in (1.0, -0.5):
                kw = dict(ta=0, tb=1, bias_mode=bias_mode, act=act, acc=acc, alpha=alpha, b16=b16)
                _gemm(L, dev, R, 70, 40, 40, **kw)
                _gemm(L, dev, R, 70, 40, 1000, ws_bytes=8 * 70 * 40 * 4, **kw)
    R.judge()


# ------------------------------------------------------------------------------------------------------- 4. split-K workspace
@pytest.mark.parametrize("b16", [False, True], ids=["f32", "bf16"])
def test_splitk_workspace_sizes(L, dev, b16):
    """K = 1000, M = 130, N = 70 (auto split 7): an ample workspace, exactly two slabs, one byte less (one slab: unsplit), less than
    one slab (unsplit), and a workspace given at K = 511 (no split below 512).  The gate holds whatever the split; nothing is
    written behind ws_bytes."""
    M, N, K = 130, 70, 1000
    per = M * N * 4
    R = _Rows()
    for ws_bytes in (64 * per, 7 * per, 2 * per, 2 * per - 1, per - 4, 16):
        for ta, tb in ((1, 1), (0, 1)):
            _gemm(L, dev, R, M, N, K, ta, tb, bias_mode=2, act=2, ws_bytes=ws_bytes, b16=b16)
    _gemm(L, dev, R, M, N, 511, 1, 1, ws_bytes=64 * per, b16=b16)
    R.judge()


# ------------------------------------------------------------------------------------------------------- 5. tiles
@pytest.mark.parametrize("b16", [False, True], ids=["f32", "bf16"])
def test_tiles_with_split(L, dev, b16):
    """64 x 64, 128 x 64, 64 x 128 and 128 x 128 tiles (a deep-K product that will split keeps its 128-wide tiles), ragged, K = 600
    over a workspace, all four layouts."""
    R = _Rows()
    for M, N in ((60, 50), (130, 50), (60, 130), (130, 131)):
        for ta, tb in LAYOUTS:
            _gemm(L, dev, R, M, N, 600, ta, tb, ws_bytes=8 * M * N * 4, b16=b16)
    R.judge()


@pytest.mark.parametrize("b16", [False, True], ids=["f32", "bf16"])
def test_unsplit_128x128_tile(L, dev, b16):
    """M = 3067, N = 2041, K = 20: 24 x 16 = 384 tiles, the smallest grid that keeps both tile halvings off (UMPR_GEMM_SMALL_GRID);
    ragged in both directions, two stages, all four layouts."""
    R = _Rows()
    for ta, tb in LAYOUTS:
        _gemm(L, dev, R, 3067, 2041, 20, ta, tb, act=1, pad_c=3 if ta == tb else 0, b16=b16)
    R.judge()
