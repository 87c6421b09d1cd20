"""The moving average of the weights on the GPU (umpr_ema_update / umpr_arena_swap in csrc/optim.hip, FusedAdam(ema_decay=),
swapped_ema, load_checkpoint(weights="ema")): the update kernel against CPU torch.lerp bit for bit (tests/test_ema_cpu.py shows
that this yardstick is the single-rounded FMA form on the very same inputs), the swap bit for bit, the optimiser's plumbing against
an average carried on the host and a twin optimiser without one - plain, clipped, skipped, accumulated - the swap around an
evaluation, the full model with the early classifier update, the oracle driven with AveragedModel (fixture ema_umpr_r, written by
tests/golden/make_ema_golden.py), a checkpoint and a resume, and that a run without the option is the run it was."""
import ctypes

import numpy as np
import pytest
import torch

from conftest import load_golden
from test_ema_cpu import DECAYS, INF_AT, NAN_AT, SWEEP, ema_pool, lerp_chain

pytestmark = pytest.mark.gpu

# both kernels: 2048 workgroups of 256 threads; one pass of the grid covers that many float4s where the two bases sit alike inside
# a 16-byte line, that many floats where they do not; four passes per iteration of the unrolled loop
BLOCKS, THREADS = 2048, 256
assert SWEEP == BLOCKS * THREADS * 4
GUARD = 64
SIZES = [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024, 1025, BLOCKS * THREADS + 3, SWEEP + 5, 4 * SWEEP + 9]
OFFSETS = ((0, 0), (1, 1), (0, 1), (1, 0))


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


def _cfg(**kw):
    from umpr_amd.config import Config
    cfg = Config(argv=[])
    for k, v in kw.items():
        setattr(cfg, k, v)
    return cfg


def _bits(x):
    return np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)


# ------------------------------------------------------------------------------------------------ the kernels
@pytest.fixture(scope="module")
def pool():
    return ema_pool()


@pytest.fixture(scope="module")
def chains(pool):
    """{decay: [ema after update 1, 2, 3]} over the whole pool, CPU torch.lerp, computed once; elementwise, so a prefix of the
    result is the result of the prefix"""
    return {d: lerp_chain(pool, d) for d in DECAYS}


@pytest.fixture(scope="module")
def swap_pools(pool):
    """two different vectors for the exchange, NaNs of distinct payloads (quiet and signalling, both signs), both zeros and both
    infinities among them"""
    a, b = pool[0].copy(), pool[1].copy()
    a.view(np.uint32)[[0, 4, 255, 1024]] = [0x7FC00001, 0xFFC12345, 0x7F800001, 0xFFFFFFFF]
    b.view(np.uint32)[[0, 3, 256, 1023]] = [0x7FC0BEEF, 0xFF800002, 0x7FFFFFFF, 0xFFC00000]
    a[1], b[1], a[2], b[2] = np.inf, -np.inf, 0.0, -0.0
    assert not np.array_equal(_bits(a), _bits(b))
    return a, b


class _Buf:
    """n floats behind `off` floats of padding, between two NaN guard bands of 64 floats (the padding is guard as well)"""

    def __init__(self, vals, off, dev):
        n = len(vals)
        self.host = np.full(GUARD + off + n + GUARD, np.nan, np.float32)
        self.lo, self.hi = GUARD + off, GUARD + off + n
        self.host[self.lo:self.hi] = vals
        self.dev = torch.from_numpy(self.host.copy()).to(dev)
        self.n, self.ptr = n, self.dev.data_ptr() + 4 * self.lo      # (an empty view would report a null pointer)
        assert self.dev.data_ptr() % 256 == 0 and self.ptr % 16 == 4 * (off % 4)

    def check(self, want, what):
        got = self.dev.cpu().numpy()
        assert _bits(got[:self.lo]).tobytes() == _bits(self.host[:self.lo]).tobytes(), what + ": guard in front"
        assert _bits(got[self.hi:]).tobytes() == _bits(self.host[self.hi:]).tobytes(), what + ": guard behind"
        bad = np.flatnonzero(_bits(got[self.lo:self.hi]) != _bits(want))
        assert bad.size == 0, (what, bad[:5], got[self.lo:self.hi][bad[:5]], np.asarray(want)[bad[:5]])


def _table(bufs):
    return (ctypes.c_void_p * max(len(bufs), 1))(*[b.ptr for b in bufs])


def _update(L, emas, params, decay, first, counts=None):
    cn = (ctypes.c_long * max(len(emas), 1))(*(counts if counts is not None else [e.n for e in emas]))
    pe, pp = _table(emas), _table(params)
    L.call("umpr_ema_update", ctypes.addressof(pe), ctypes.addressof(pp), ctypes.addressof(cn), len(emas), decay, first, st())


def _swap(L, xs, ys, counts=None):
    cn = (ctypes.c_long * max(len(xs), 1))(*(counts if counts is not None else [x.n for x in xs]))
    px, py = _table(xs), _table(ys)
    L.call("umpr_arena_swap", ctypes.addressof(px), ctypes.addressof(py), ctypes.addressof(cn), len(xs), st())


@pytest.mark.parametrize("decay", DECAYS)
@pytest.mark.parametrize("n", SIZES)
def test_update_kernel_equals_cpu_lerp_bit_for_bit(L, dev, pool, chains, n, decay):
    """first = 1 onto a NaN-filled average, then first = 0 twice with other parameters: the average is torch.lerp's, bit for
    bit and with no element exempt, the parameters and every guard band are untouched - with both bases on 16-byte boundaries,
    both one float behind one (the float4 path with a head and a tail), and one of them only (element by element)"""
    want = [c[:n] for c in chains[decay]]
    if n > 19:
        assert np.isnan(want[2][NAN_AT]) and np.isinf(want[2][INF_AT]) and want[2][7] == 0 and want[2][13] == 0
    for off_e, off_p in OFFSETS:
        what = f"n={n} decay={decay} ema+{off_e} p+{off_p}"
        ema = _Buf(np.full(n, np.nan, np.float32), off_e, dev)
        ps = [_Buf(pool[j][:n], off_p, dev) for j in range(3)]
        for j in range(3):
            _update(L, [ema], [ps[j]], decay, int(j == 0))
            ema.check(want[j], f"{what} after update {j + 1}")
        for j in range(3):
            ps[j].check(pool[j][:n], f"{what} parameters {j + 1}")


@pytest.mark.parametrize("n", SIZES)
def test_swap_kernel_exchanges_and_restores_bit_for_bit(L, dev, swap_pools, n):
    a0, b0 = swap_pools[0][:n], swap_pools[1][:n]
    for off_a, off_b in OFFSETS:
        what = f"n={n} a+{off_a} b+{off_b}"
        a, b = _Buf(a0, off_a, dev), _Buf(b0, off_b, dev)
        _swap(L, [a], [b])
        a.check(b0, what + ": a after the swap")
        b.check(a0, what + ": b after the swap")
        _swap(L, [a], [b])
        a.check(a0, what + ": a after the second swap")
        b.check(b0, what + ": b after the second swap")


def test_three_arenas_with_an_empty_one_in_the_middle(L, dev, pool, chains, swap_pools):
    sizes, offs, lo = (1025, 0, 257), (0, 0, 1), (0, 5000, 9000)
    decay = DECAYS[0]
    emas = [_Buf(np.full(n, np.nan, np.float32), o, dev) for n, o in zip(sizes, offs)]
    ps = [[_Buf(pool[j][s:s + n], o, dev) for n, o, s in zip(sizes, offs, lo)] for j in range(3)]
    for j in range(3):
        _update(L, emas, ps[j], decay, int(j == 0))
    for k, (n, s) in enumerate(zip(sizes, lo)):
        emas[k].check(chains[decay][2][s:s + n], f"arena {k}")
        for j in range(3):
            ps[j][k].check(pool[j][s:s + n], f"arena {k} parameters {j + 1}")
    # a table of nothing, and a table whose counts are all zero, are successful no-ops
    _update(L, [], [], decay, 1)
    _update(L, emas, ps[0], decay, 1, counts=[0, 0, 0])
    emas[0].check(chains[decay][2][:1025], "after the no-ops")
    # the swap over the same layout
    xs = [_Buf(swap_pools[0][s:s + n], o, dev) for n, o, s in zip(sizes, offs, lo)]
    ys = [_Buf(swap_pools[1][s:s + n], o, dev) for n, o, s in zip(sizes, offs, lo)]
    _swap(L, xs, ys)
    _swap(L, [], [])
    _swap(L, xs, ys, counts=[0, 0, 0])
    for k, (n, s) in enumerate(zip(sizes, lo)):
        xs[k].check(swap_pools[1][s:s + n], f"swap: a of arena {k}")
        ys[k].check(swap_pools[0][s:s + n], f"swap: b of arena {k}")


def test_refusals_leave_everything_untouched(L, dev, pool):
    from umpr_amd._lib import UmprHipError
    ema, p = _Buf(np.full(100, np.nan, np.float32), 0, dev), _Buf(pool[0][:100], 0, dev)
    pe, pp = (ctypes.c_void_p * 1)(ema.ptr), (ctypes.c_void_p * 1)(p.ptr)
    odd = (ctypes.c_void_p * 1)(p.ptr + 2)
    null, cn, neg = (ctypes.c_void_p * 1)(None), (ctypes.c_long * 1)(100), (ctypes.c_long * 1)(-1)
    A = ctypes.addressof
    tables = (((None, A(pp), A(cn), 1), "null arena table"), ((A(pe), None, A(cn), 1), "null arena table"),
              ((A(pe), A(pp), None, 1), "null arena table"), ((A(null), A(pp), A(cn), 1), "bad pointer / count"),
              ((A(pe), A(null), A(cn), 1), "bad pointer / count"), ((A(pe), A(pp), A(cn), 9), "arenas outside 0..8"),
              ((A(pe), A(pp), A(cn), -1), "arenas outside 0..8"), ((A(pe), A(pp), A(neg), 1), "bad pointer / count"),
              ((A(pe), A(odd), A(cn), 1), "not aligned to a float"), ((A(odd), A(pp), A(cn), 1), "not aligned to a float"))
    for args, text in tables:
        for first in (0, 1):
            with pytest.raises(UmprHipError, match="ema_update: .*" + text):
                L.call("umpr_ema_update", *args, 0.9, first, st())
        with pytest.raises(UmprHipError, match="arena_swap: .*" + text):
            L.call("umpr_arena_swap", *args, st())
    for decay in (0.5, 1.0, 0.0, -0.1, 1.5, float("nan")):
        for first in (0, 1):
            with pytest.raises(UmprHipError, match="ema_update: decay .* outside the open interval"):
                L.call("umpr_ema_update", A(pe), A(pp), A(cn), 1, decay, first, st())
    # the swap of a range with one that overlaps it: itself, and one that starts inside it
    inside, part = (ctypes.c_void_p * 1)(p.ptr + 4 * 40), (ctypes.c_long * 1)(60)
    for a, b in ((pp, pp), (pp, inside), (inside, pp)):
        with pytest.raises(UmprHipError, match="arena_swap: arena 0: the two ranges overlap"):
            L.call("umpr_arena_swap", A(a), A(b), A(part), 1, st())
    ema.check(np.full(100, np.nan, np.float32), "average after the refusals")
    p.check(pool[0][:100], "parameters after the refusals")


# ------------------------------------------------------------------------------------------------ the optimiser on UMPR-R
def _umpr_r(dev):
    from umpr_amd.model import UMPR
    from umpr_amd.synthetic import make_param_state
    P = make_param_state(31, 50, 1000, 1, True, m_scale=0.05)
    model = UMPR(_cfg(review_net_only=True), P["embedding.weight"].numpy())
    model.load_state_dict(P)
    return model.to(dev)


def _fresh_r(dev, **kw):
    from umpr_amd.optim import FusedAdam
    model = _umpr_r(dev)
    return model, FusedAdam(model, 1e-3, 1e-3, **kw)


def _snap(opt):
    return [t.clone() for g in opt.groups for t in (g.p, g.m, g.v)]


def _same(a, b):
    return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))


def _eq(x, y):
    """bit for bit (torch.equal calls NaN unequal to itself and -0 equal to +0)"""
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


def _params(model):
    return {n: p.detach().cpu().clone() for n, p in model.named_parameters() if p.requires_grad}


class _HostAverage:
    """the expected average, carried on the host with torch.lerp from a copy of the parameters after the first step"""

    def __init__(self, decay):
        self.w, self.ema = 1.0 - decay, None

    def update(self, params):
        self.ema = ({n: p.clone() for n, p in params.items()} if self.ema is None
                    else {n: torch.lerp(self.ema[n], params[n], self.w) for n in params})

    def check(self, opt, what):
        got = opt.ema_tensors()
        assert sorted(got) == sorted(self.ema)
        for n, t in got.items():
            assert t.shape == self.ema[n].shape and _eq(t.cpu(), self.ema[n]), (what, n)


@pytest.fixture(scope="module")
def micro():
    from umpr_amd.synthetic import make_batch
    return [make_batch(700 + j, 4, 1000, review_net_only=True) for j in range(8)]


def _norms_without_clipping(dev, micro):
    from umpr_amd.train import train_step
    model, opt = _fresh_r(dev, max_grad_norm=1e9)
    norms = []
    for b in micro[:4]:
        train_step(model, opt, b)
        norms.append(opt.clip_stats()["norm"])
    return norms


@pytest.mark.parametrize("clip", [False, True])
def test_umpr_r_average_equals_the_host_lerp_and_leaves_the_steps_alone(dev, micro, clip):
    """four steps at decay 0.9: after every one ema_tensors() is the host-carried torch.lerp, bit for bit, and parameters and
    moments are those of a twin without the average.  clip: the same with max_grad_norm between the second and third largest
    of the four gradient norms, so that two steps clip - and then a fifth step whose gradient carries an inf: it is skipped,
    the parameters keep every bit, and the average still moves one lerp towards them"""
    from umpr_amd.streams import wait_for_gradients
    from umpr_amd.train import train_step
    kw = {}
    if clip:
        norms = sorted(_norms_without_clipping(dev, micro))
        kw["max_grad_norm"] = 0.5 * (norms[1] + norms[2])
        print("gradient norms", norms, "max_grad_norm", kw["max_grad_norm"])
    model, opt = _fresh_r(dev, ema_decay=0.9, **kw)
    twin_model, twin = _fresh_r(dev, **kw)
    assert not opt.ema_ready and opt._ema is None
    want = _HostAverage(0.9)
    seen = []
    for s in range(4):
        train_step(model, opt, micro[s])
        train_step(twin_model, twin, micro[s])
        assert opt.ema_ready
        now = _params(model)
        seen.append(now)
        want.update(now)
        want.check(opt, f"step {s + 1}")
        assert _same(_snap(opt), _snap(twin)), s
    assert not any(_eq(seen[0][n], seen[3][n]) for n in seen[0])            # the steps moved every tensor ...
    assert not any(_eq(want.ema[n], seen[3][n]) for n in seen[0])           # ... and the average is not the last iterate
    assert twin._ema is None and not twin.ema_ready
    if not clip:
        return
    stats = opt.clip_stats()
    assert stats["clipped"] == 2 and stats["skipped"] == 0 and stats["seen"] == 4, stats
    for m, o in ((model, opt), (twin_model, twin)):
        m.train()
        _, loss = m(*micro[4])
        o.zero_grad()
        loss.backward()
        wait_for_gradients(dev)
        o.groups[0].g[12345] = float("inf")
        o.step()
    assert opt.clip_stats()["skipped"] == 1 and opt.step_count == 5
    now = _params(model)
    assert all(_eq(now[n], seen[3][n]) for n in now)                        # skipped: nothing moved
    before = {n: t.clone() for n, t in want.ema.items()}
    want.update(now)
    want.check(opt, "the skipped step")
    assert not any(_eq(before[n], want.ema[n]) for n in before)             # the average did
    assert _same(_snap(opt), _snap(twin))


def test_umpr_r_average_counts_optimiser_steps_under_accumulation(dev, micro):
    """groups of two micro-batches: one update of the average per optimiser step, none between the micro-batches"""
    from umpr_amd.train import train_step
    model, opt = _fresh_r(dev, ema_decay=0.9)
    twin_model, twin = _fresh_r(dev)
    want = _HostAverage(0.9)
    for s in range(4):
        for m, o in ((model, opt), (twin_model, twin)):
            train_step(m, o, micro[2 * s], update=False)
            if m is model and s > 0:
                want.check(opt, f"inside group {s + 1}")                    # the micro-batch alone moved nothing
            train_step(m, o, micro[2 * s + 1], update=True)
        assert opt.step_count == s + 1 and opt.pending == 0
        want.update(_params(model))
        want.check(opt, f"group {s + 1}")
        assert _same(_snap(opt), _snap(twin)), s


# ------------------------------------------------------------------------------------------------ the swap around an evaluation
def test_swapped_ema_puts_the_average_under_the_model_and_takes_it_back(dev, micro):
    from umpr_amd.train import evaluate_mse, train_step
    model, opt = _fresh_r(dev, ema_decay=0.9)
    with pytest.raises(RuntimeError, match="the first step"):
        with opt.swapped_ema():
            raise AssertionError("entered")
    want = _HostAverage(0.9)
    for s in range(3):
        train_step(model, opt, micro[s])
        want.update(_params(model))
    raw = _params(model)
    before = _snap(opt) + [a.clone() for a in opt._ema.arenas]
    versions = [p._version for p in model.parameters()]
    # a second model that simply holds the averaged weights
    other = _umpr_r(dev)
    with torch.no_grad():
        for n, p in other.named_parameters():
            if n in want.ema:
                p.copy_(want.ema[n])
    valid = micro[5:7]
    mse_other, mse_raw = evaluate_mse(other, valid), evaluate_mse(model, valid)
    with opt.swapped_ema() as inside:
        assert inside is opt
        now = _params(model)
        assert all(_eq(now[n], want.ema[n]) for n in now)                   # the parameters are the average ...
        for n, t in opt.ema_tensors().items():
            assert _eq(t.cpu(), raw[n]), n                                  # ... and the EMA arenas hold the raw weights
        mse_ema = evaluate_mse(model, valid)
        for call in (opt.step, opt.accumulate, opt.arm_early, opt.state_dict):
            with pytest.raises(RuntimeError, match="swapped_ema"):
                call()
        with pytest.raises(RuntimeError, match="already inside"):
            with opt.swapped_ema():
                raise AssertionError("entered")
    print(f"valid mse: raw {mse_raw!r} averaged {mse_ema!r} second model {mse_other!r}")
    assert mse_ema == mse_other and mse_ema != mse_raw
    assert _same(before, _snap(opt) + list(opt._ema.arenas))
    assert versions == [p._version for p in model.parameters()] and opt.step_count == 3
    # an exception raised inside the context still swaps back
    with pytest.raises(KeyError, match="inside"):
        with opt.swapped_ema():
            assert _eq(_params(model)[sorted(raw)[0]], want.ema[sorted(raw)[0]])
            raise KeyError("inside")
    assert _same(before, _snap(opt) + list(opt._ema.arenas)) and not opt._swapped
    train_step(model, opt, micro[3])                                        # and the run goes on
    want.update(_params(model))
    want.check(opt, "the step behind the swaps")


# ------------------------------------------------------------------------------------------------ the full model
@pytest.fixture(scope="module")
def full_state():
    from umpr_amd.synthetic import make_batch, make_param_state
    return make_param_state(121, 50, 500, 1, False, m_scale=0.05), [make_batch(130, 2, 500, 1), make_batch(131, 2, 500, 1)]


@pytest.mark.parametrize("variant", ["fp32", "fp32_freeze_conv", "bf16"])
def test_full_model_average_behind_the_early_classifier_update(dev, full_state, variant):
    """V = 1, two train_steps of two samples with the early classifier update armed (it ran: asserted): after step 1 the average
    equals the parameters over every element of the arenas - an update that did not wait for the side stream's Adam on the
    classifier slice would have copied stale weights - and after step 2 it equals the host lerp"""
    from umpr_amd import optim
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    from umpr_amd.train import train_step
    assert optim._EARLY_ADAM != "0"
    P, batches = full_state
    cfg = _cfg(views=["unknown"], dtype="bf16" if variant == "bf16" else "fp32", freeze_conv=variant == "fp32_freeze_conv")
    model = UMPR(cfg, P["embedding.weight"].numpy())
    model.load_state_dict(P)
    model = model.to(dev)
    torch.manual_seed(5)
    opt = FusedAdam(model, 1e-3, 1e-3, ema_decay=0.9)
    assert opt.early_bucket() is not None
    seen, step = [], opt.step
    opt.step = lambda *a, **kw: (seen.append(opt._early_done is not None), step(*a, **kw))[1]
    start = [g.p.cpu() for g in opt.groups]
    train_step(model, opt, batches[0])
    first = [g.p.cpu() for g in opt.groups]
    for g, a, p0, p1 in zip(opt.groups, opt._ema.arenas, start, first):
        assert a.shape == g.p.shape and _eq(a.cpu(), p1)
        assert g.numel == 0 or not _eq(p0, p1)
    _, lo, hi, _ = opt.early_bucket()
    assert not torch.equal(start[0][lo:hi], first[0][lo:hi])                # the classifier slice moved
    train_step(model, opt, batches[1])
    assert seen == [True, True]                                             # both steps found the slice updated early
    for g, a, p1 in zip(opt.groups, opt._ema.arenas, first):
        assert _eq(a.cpu(), torch.lerp(p1, g.p.cpu(), 1.0 - 0.9))
    assert all(torch.isfinite(a).all() for a in opt._ema.arenas)
    assert sorted(opt.ema_tensors()) == sorted(n for n, p in model.named_parameters() if p.requires_grad)


# ------------------------------------------------------------------------------------------------ against the oracle
def _worst_ratio(got, g, prefix):
    """max over the compared elements of |x - oracle| / (2e-5 + 1e-4 |oracle|): the project's trajectory tolerance"""
    worst = {}
    for k, x in got.items():
        ref = torch.from_numpy(g[prefix + k])
        mask = torch.from_numpy(np.unpackbits(g["mask/" + k])[:ref.numel()].astype(bool)).view(ref.shape)
        assert mask.any(), k
        d = (x.detach().cpu() - ref).abs() / (2e-5 + 1e-4 * ref.abs())
        worst[k] = float(d[mask].max())
    return worst


def test_average_vs_oracle(dev):
    """Four steps at lr 1e-3, l2 1e-3, decay 0.9 against the oracle driven with torch.optim.Adam and AveragedModel(multi_avg_fn=
    get_ema_multi_avg_fn(0.9)).update_parameters behind every step.  The average is a convex combination of iterates that each
    meet the trajectory tolerance 2e-5 + 1e-4 |x|, so it is held to the same one."""
    from umpr_amd.synthetic import make_batch
    from umpr_amd.train import train_step
    g = load_golden("ema_umpr_r")
    g.update(load_golden("ema_umpr_r_params"))
    assert float(g["decay"]) == 0.9 and float(g["lr"]) == 1e-3 and float(g["l2"]) == 1e-3
    # each of the wrong implementations the oracle ran ends far outside the tolerance: passing means none of them is at work
    for mutant in ("init", "before", "weight", "none"):
        print("separation", mutant, float(g["separation/" + mutant]))
        assert float(g["separation/" + mutant]) > 10, mutant
    model, opt = _fresh_r(dev, ema_decay=float(g["decay"]))
    for s in range(4):
        train_step(model, opt, make_batch(500 + 2 * s, 4, 1000, review_net_only=True))
    params = {k: p for k, p in model.named_parameters() if p.requires_grad}
    assert sorted("ema/" + k for k in params) == sorted(k for k in g if k.startswith("ema/"))
    worst_p = _worst_ratio(params, g, "param/")
    print("parameters, error / tolerance:", {k: round(v, 3) for k, v in worst_p.items()})
    worst = _worst_ratio(opt.ema_tensors(), g, "ema/")
    print("average, error / tolerance:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst_p.values()) <= 1.0, worst_p
    assert max(worst.values()) <= 1.0, worst


# ------------------------------------------------------------------------------------------------ checkpoint and resume
def test_checkpoint_carries_the_average_and_a_resume_is_exact(dev, micro, tmp_path):
    from umpr_amd.checkpoint import load_checkpoint, save_checkpoint
    from umpr_amd.train import train_step
    path = str(tmp_path / "ema.pt")
    model, opt = _fresh_r(dev, ema_decay=0.9)
    for s in range(4):
        train_step(model, opt, micro[s])
        if s == 1:
            save_checkpoint(path, model, opt, batch_counter=2)
            at_two = ({n: t.cpu().clone() for n, t in opt.ema_tensors().items()}, _params(model))
    ck = torch.load(path, weights_only=True)
    assert sorted(ck["optimizer"]) == ["base_lr", "ema", "ema_decay", "lr", "m", "step", "v"] and ck["optimizer"]["ema_decay"] == 0.9
    for n, t in at_two[1].items():
        assert _eq(ck["model"][n], t), n                                    # "model" keeps the raw weights
    # resumed in a fresh model
    res_model, res = _fresh_r(dev, ema_decay=0.9)
    assert load_checkpoint(path, res_model, res, map_location=dev)["batch_counter"] == 2
    assert res.ema_ready and res.step_count == 2
    for s in (2, 3):
        train_step(res_model, res, micro[s])
    assert _same(_snap(opt) + list(opt._ema.arenas), _snap(res) + list(res._ema.arenas))
    # weights="ema" into a fresh model: the average of the checkpoint, bit for bit, in place of the raw weights
    fresh = _umpr_r(dev)
    load_checkpoint(path, fresh, map_location=dev, weights="ema")
    for n, p in fresh.named_parameters():
        if n in at_two[0]:
            assert _eq(p.detach().cpu(), at_two[0][n]) and not _eq(p.detach().cpu(), at_two[1][n]), n
    # and the two settings refuse each other's checkpoints before anything is loaded
    _, off = _fresh_r(dev)
    with pytest.raises(ValueError, match="--ema_decay"):
        load_checkpoint(path, fresh, off, map_location=dev)
    assert off.step_count == 0


# ------------------------------------------------------------------------------------------------ off is off
def test_without_the_option_the_trajectory_and_the_allocations_are_the_old_ones(dev):
    """ema_decay = 0, given or not: the Adam trajectory fixture (adam_umpr_r) at its own tolerances - the golden-checked path of
    test_gpu_grad_accum.py - over its three steps and bit-equality with an optimiser built without the argument over four;
    no EMA arena is ever allocated"""
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_batch
    from umpr_amd.train import train_step
    g = load_golden("adam_umpr_r")
    model = _umpr_r(dev)
    opt = FusedAdam(model, float(g["lr"]), float(g["l2"]), lr_decay=0.99, ema_decay=0.0)
    twin_model = _umpr_r(dev)
    twin = FusedAdam(twin_model, float(g["lr"]), float(g["l2"]), lr_decay=0.99)
    for step in range(4):
        batch = make_batch(500 + step, 4, 1000, review_net_only=True)
        _, loss = train_step(model, opt, batch)
        train_step(twin_model, twin, batch)
        if step < 3:
            assert abs(loss.item() - g["losses"][step]) < 1e-4
        assert opt._ema is None and not opt.ema_ready and opt.ema_bytes() == 0
        with pytest.raises(RuntimeError, match="the moving average is off"):
            opt.ema_tensors()
        if step == 0:
            opt.epoch_end()
            twin.epoch_end()
        if step == 2:
            for k, p in model.named_parameters():
                if "param/" + k in g:
                    ref = torch.from_numpy(np.asarray(g["param/" + k]))
                    assert torch.allclose(p.detach().cpu(), ref, atol=2e-5, rtol=1e-4), k
        assert _same(_snap(opt), _snap(twin))
    assert sorted(opt.state_dict()) == ["base_lr", "lr", "m", "step", "v"]
