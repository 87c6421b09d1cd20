"""Per-module learning rates, decoupled decay and warm-up on the GPU (umpr_adam_step_groups in csrc/optim.hip, FusedAdam(lr_scales=,
wd_scales=, decoupled_decay=, warmup_steps=)): the segmented kernel against the plain forms bit for bit at multipliers 1, its host-
against its device-scalar form, against the float64 restatement (tests/adam_groups_reference.py) at the project's gate, a skipped
step; then the optimiser on UMPR-R against the oracle with one torch param group per parameter (fixture param_groups_umpr_r,
written by tests/golden/make_param_groups_golden.py), as a captured graph against eager, and on the full model against twins that
were simply built with the scaled learning rate and decay."""
import ctypes
import math

import numpy as np
import pytest
import torch

from adam_groups_reference import adam_groups_step
from conftest import load_golden

pytestmark = pytest.mark.gpu

GUARD, GUARD_VALUE = 64, -7.5
PASS = 8192 * 256           # elements one pass of the capped grid covers: from here on a thread takes a second element
# (n, the segment ends in front of n): one segment; a boundary at a wave's edge inside a block; two, with a ragged last segment; one
# at a block's edge; the most a launch takes; three around the start of the grid's second pass, with a ragged tail
CASES = {"one": (64, []), "wave_edge": (128, [64]), "ragged": (193, [64, 128]), "block_edge": (515, [256]),
         "sixteen": (16 * 64, [64 * k for k in range(1, 16)]),
         "second_pass": (PASS + 64 * 5 + 77, [PASS - 64, PASS, PASS + 64])}
OFFSETS = [0, 1]            # floats: the optimiser passes slices of its arenas, so 16-byte alignment is not the kernel's to assume
LR, WD, SCALE = 1e-3, 1e-2, 0.5


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


def _eq(x, y):
    """bit for bit"""
    return x.shape == y.shape and torch.equal(x.contiguous().view(torch.int32), y.contiguous().view(torch.int32))


class _Guarded:
    """`values` on the device, `off` floats behind a 256-byte boundary of a larger buffer with guard elements on both sides."""

    def __init__(self, values, off, dev):
        n = values.numel()
        self.buf = torch.full((GUARD + off + n + GUARD,), GUARD_VALUE, dtype=torch.float32, device=dev)
        self.t = self.buf[GUARD + off:GUARD + off + n]
        self.t.copy_(values)
        assert self.t.data_ptr() % 16 == 4 * off
        self.lo, self.hi = GUARD + off, GUARD + off + n

    def guards_untouched(self):
        return bool((self.buf[:self.lo] == GUARD_VALUE).all()) and bool((self.buf[self.hi:] == GUARD_VALUE).all())


@pytest.fixture(scope="module")
def start():
    """p, g, m, v of the largest case, made once; every case takes prefixes"""
    n = max(n for n, _ in CASES.values())
    g = torch.Generator().manual_seed(9)
    return [torch.randn(n, generator=g), torch.randn(n, generator=g) * 0.1, torch.randn(n, generator=g) * 0.01,
            torch.rand(n, generator=g) * 1e-3]


def _hyper(step, dev, decoupled=False, lr=LR, wd=WD, scale=SCALE):
    return torch.tensor([scale, lr / (1 - 0.9 ** step), 1 / math.sqrt(1 - 0.999 ** step), lr * wd if decoupled else wd],
                        dtype=torch.float32, device=dev)


def _state(coef, finite, dev):
    return torch.tensor([coef, 1.0, finite, 1.0, 0, 0, 0, 0], dtype=torch.float32, device=dev)


def _groups(L, bufs, n, step, ends, lr_mult, wd_mult, decoupled=False, hyper=None, state=None):
    k = len(ends)
    e, a, w = (ctypes.c_long * k)(*ends), (ctypes.c_float * k)(*lr_mult), (ctypes.c_float * k)(*wd_mult)
    L.call("umpr_adam_step_groups", *bufs, n, LR, 0.9, 0.999, 1e-8, WD, step, SCALE, hyper, state, ctypes.addressof(e),
           ctypes.addressof(a), ctypes.addressof(w), k, int(decoupled), st())


def _mults(k):
    """distinct per segment, none of them 1, a zero decay among them"""
    return [0.25 + 0.375 * j for j in range(k)], [0.0 if j % 5 == 1 else 3.0 - 0.15 * j for j in range(k)]


# ------------------------------------------------------------------------------------------------ the kernel
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("case", list(CASES))
def test_segmented_kernel_with_multipliers_one_equals_the_plain_kernels(L, dev, start, case, off):
    """coupled, every multiplier exactly 1: the four forms of the segmented launch (host / device scalars, without / with a clip
    coefficient of 1) leave p, m and v bit-identical to umpr_adam_step over three steps"""
    n, inner = CASES[case]
    ends, ones = inner + [n], [1.0] * (len(inner) + 1)
    sets = [[_Guarded(t[:n], off, dev) for t in start] for _ in range(5)]
    plain, host, devf, host_clip, dev_clip = [[b.t for b in s] for s in sets]
    state = _state(1.0, 1.0, dev)
    for step in (1, 2, 3):
        L.call("umpr_adam_step", *plain, n, LR, 0.9, 0.999, 1e-8, WD, step, SCALE, st())
        _groups(L, host, n, step, ends, ones, ones)
        _groups(L, devf, n, step, ends, ones, ones, hyper=_hyper(step, dev))
        _groups(L, host_clip, n, step, ends, ones, ones, state=state)
        _groups(L, dev_clip, n, step, ends, ones, ones, hyper=_hyper(step, dev), state=state)
    assert float((plain[0] - start[0][:n].to(dev)).abs().max()) > 1e-3      # the steps moved the parameters
    for k, name in ((0, "p"), (2, "m"), (3, "v")):
        for what, other in (("host", host), ("dev", devf), ("host_clip", host_clip), ("dev_clip", dev_clip)):
            assert _eq(plain[k], other[k]), (name, what)
    assert all(b.guards_untouched() for s in sets for b in s)


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("case", list(CASES))
def test_host_scalar_form_equals_device_scalar_form(L, dev, start, case, off, decoupled):
    """with distinct multipliers per segment, coupled and decoupled, without and with a clip coefficient of 0.37: the scalars by
    value and from device memory give the same bits over three steps"""
    n, inner = CASES[case]
    ends = inner + [n]
    lr_mult, wd_mult = _mults(len(ends))
    sets = [[_Guarded(t[:n], off, dev) for t in start] for _ in range(4)]
    host, devf, host_clip, dev_clip = [[b.t for b in s] for s in sets]
    state = _state(0.37, 1.0, dev)
    for step in (1, 2, 3):
        _groups(L, host, n, step, ends, lr_mult, wd_mult, decoupled)
        _groups(L, devf, n, step, ends, lr_mult, wd_mult, decoupled, hyper=_hyper(step, dev, decoupled))
        _groups(L, host_clip, n, step, ends, lr_mult, wd_mult, decoupled, state=state)
        _groups(L, dev_clip, n, step, ends, lr_mult, wd_mult, decoupled, hyper=_hyper(step, dev, decoupled), state=state)
    for k, name in ((0, "p"), (2, "m"), (3, "v")):
        assert _eq(host[k], devf[k]) and _eq(host_clip[k], dev_clip[k]), name
        assert not _eq(host[k], host_clip[k]), name
    assert all(b.guards_untouched() for s in sets for b in s)


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("case", list(CASES))
def test_segmented_kernel_vs_float64(L, dev, start, case, off, decoupled):
    """three steps with distinct multipliers per segment against the float64 restatement: each of p, m and v within K = 4 x the
    distance the float32 CPU evaluation of the same statements has from float64 (coattn_decisions.gate, the project's gate).  An
    element that took its neighbour's multipliers is off by a quarter of a step or a tenth of the decay term: hundreds of times
    that."""
    import coattn_decisions as C
    n, inner = CASES[case]
    ends = inner + [n]
    lr_mult, wd_mult = _mults(len(ends))
    a, w, prev = np.empty(n), np.empty(n), 0
    for end, a_, w_ in zip(ends, lr_mult, wd_mult):
        a[prev:end], w[prev:end], prev = np.float32(a_), np.float32(w_), end
    bufs = [_Guarded(t[:n], off, dev) for t in start]
    got = [b.t for b in bufs]
    ref = [t[:n].double().numpy() for t in start]
    ref32 = [t[:n].numpy() for t in start]
    for step in (1, 2, 3):
        _groups(L, got, n, step, ends, lr_mult, wd_mult, decoupled)
        kw = dict(decoupled=decoupled, grad_scale=SCALE)
        ref[0], ref[2], ref[3] = adam_groups_step(*ref, step, LR, WD, a, w, dtype=np.float64, **kw)
        ref32[0], ref32[2], ref32[3] = adam_groups_step(*ref32, step, LR, WD, a, w, dtype=np.float32, **kw)
    pick = lambda xs: [torch.from_numpy(np.ascontiguousarray(xs[k])) for k in (0, 2, 3)]
    ok, rows = C.gate([got[k].cpu() for k in (0, 2, 3)], pick(ref), pick(ref32), names=("p", "m", "v"), log=print,
                      tag=f"{case} off={off} {'decoupled' if decoupled else 'coupled'}")
    print(f"param_groups gate {case} off={off} decoupled={decoupled}: worst ratio {max(r['ratio'] for r in rows):.3f}")
    assert ok, rows
    assert all(b.guards_untouched() for b in bufs)


def test_launcher_refuses_before_any_kernel_runs(L, dev, start):
    """seventeen segments, an end that is no multiple of 64, a last end that is not n: an error with a message, and p, m, v and the
    guards keep every bit"""
    from umpr_amd._lib import UmprHipError
    n = 17 * 64
    bufs = [_Guarded(t[:n], 1, dev) for t in start]
    got = [b.t for b in bufs]
    for ends, what in (([64 * k for k in range(1, 18)], "17 segments outside 1..16"), ([65, n], "not a multiple of 64 elements"),
                       ([64, n - 1], "the last segment ends at 1087, not at n = 1088"), ([64, n + 64], "past n = 1088")):
        with pytest.raises(UmprHipError, match="adam_groups: .*" + what):
            _groups(L, got, n, 1, ends, [2.0] * len(ends), [2.0] * len(ends))
    torch.cuda.synchronize()
    for t, ref in zip(got, start):
        assert _eq(t.cpu(), ref[:n])
    assert all(b.guards_untouched() for b in bufs)


@pytest.mark.parametrize("decoupled", [False, True])
@pytest.mark.parametrize("off", OFFSETS)
@pytest.mark.parametrize("case", ["ragged", "second_pass"])
def test_a_non_finite_step_touches_nothing(L, dev, start, case, off, decoupled):
    """the clipped forms with the flag down leave p, m, v and the guards as they were - in decoupled mode the shrink included"""
    n, inner = CASES[case]
    ends = inner + [n]
    lr_mult, wd_mult = _mults(len(ends))
    state = _state(0.0, 0.0, dev)
    for hyper in (None, _hyper(1, dev, decoupled)):
        bufs = [_Guarded(t[:n], off, dev) for t in start]
        got = [b.t for b in bufs]
        got[1][min(77, n - 1)] = float("inf")
        _groups(L, got, n, 1, ends, lr_mult, wd_mult, decoupled, hyper=hyper, state=state)
        for k in (0, 2, 3):
            assert _eq(got[k].cpu(), start[k][:n]), (k, hyper is None)
        assert all(b.guards_untouched() for b in bufs)


# ------------------------------------------------------------------------------------------------ UMPR-R against the oracle
def _umpr_r(dev, **kw):
    from umpr_amd.model import UMPR
    from umpr_amd.synthetic import make_param_state
    P = make_param_state(31, 50, 1000, 1, True, m_scale=0.05)
    model = UMPR(_cfg(review_net_only=True, **kw), P["embedding.weight"].numpy())
    model.load_state_dict(P)
    return model.to(dev)


def _golden_leg(g, leg):
    """{name: (oracle parameter, mask)} of one leg; the decoupled leg's parameters are stored XORed with the coupled leg's"""
    out = {}
    for key in g:
        if key.startswith("coupled/param/"):
            k = key[len("coupled/param/"):]
            ref = g[key] if leg == "coupled" else (g[f"decoupled/param_xor_coupled/{k}"] ^ g[key].view(np.uint32)).view(np.float32)
            mask = np.unpackbits(g[f"{leg}/mask/{k}"])[:ref.size].astype(bool).reshape(ref.shape)
            out[k] = (torch.from_numpy(ref.copy()), torch.from_numpy(mask))
    return out


def _worst_ratio(model, leg):
    """max over the compared elements of |p - oracle| / (2e-5 + 1e-4 |oracle|): the bound of test_train_trajectory_golden, on the
    elements whose oracle gradient was above 1e-4 of its maximum in every step"""
    worst = {}
    for k, p in model.named_parameters():
        if not p.requires_grad:
            continue
        ref, mask = leg[k]
        assert mask.any(), k
        d = (p.detach().cpu() - ref).abs() / (2e-5 + 1e-4 * ref.abs())
        worst[k] = float(d[mask].max())
    return worst


@pytest.mark.parametrize("leg", ["coupled", "decoupled"])
def test_umpr_r_trajectory_vs_oracle_with_param_groups(dev, leg):
    """Four UMPR-R steps against the oracle driven by torch.optim.Adam (lr 1e-3, l2 1e-3) / torch.optim.AdamW (lr 1e-3, l2 1.0) with
    one param group per parameter: lr_scale review_net.r_net.=0.25,review_net.=0.5, wd_scale linear_fusion.=0,
    review_net.s_net_u.=4, a warm-up of 3 steps.  Each wrong variant the oracle ran - no lr scale, no wd scale, the other decay mode,
    no warm-up, no decay, shortest prefix - ends more than 10 x the tolerance away: passing means none of them is at work."""
    from umpr_amd.optim import FusedAdam, parse_scales
    from umpr_amd.synthetic import make_batch
    from umpr_amd.train import train_step
    g = load_golden("param_groups_umpr_r")
    assert float(g["lr"]) == 1e-3 and int(g["warmup_steps"]) == 3
    assert float(g["coupled/l2"]) == 1e-3 and float(g["decoupled/l2"]) == 1.0
    lr_scales, wd_scales = parse_scales(str(g["lr_scale"])), parse_scales(str(g["wd_scale"]))
    assert lr_scales == {"review_net.r_net.": 0.25, "review_net.": 0.5} and wd_scales == {"linear_fusion.": 0.0, "review_net.s_net_u.": 4.0}
    for variant in ("no_lr_scale", "no_wd_scale", "other_decay_mode", "no_warmup", "no_decay", "shortest_prefix"):
        sep = float(g[f"{leg}/separation/{variant}"])
        print(f"{leg}: separation {variant}: {sep:.1f}")
        assert sep > 10, (leg, variant, sep)
    model = _umpr_r(dev)
    opt = FusedAdam(model, float(g["lr"]), float(g[f"{leg}/l2"]), lr_scales=lr_scales, wd_scales=wd_scales,
                    decoupled_decay=leg == "decoupled", warmup_steps=int(g["warmup_steps"]))
    for s in range(4):
        train_step(model, opt, make_batch(500 + s, 4, 1000, review_net_only=True))
    worst = _worst_ratio(model, _golden_leg(g, leg))
    print(f"{leg} leg, error / tolerance:", {k: round(v, 3) for k, v in worst.items()})
    assert max(worst.values()) <= 1.0, worst


def _snap(opt):
    return [t.clone() for g in opt.groups for t in (g.p, g.m, g.v)]


def _same(a, b):
    return len(a) == len(b) and all(_eq(x, y) for x, y in zip(a, b))


def test_graphed_umpr_r_step_with_param_groups_equals_eager(dev):
    """test_graphed_umpr_r_step_with_clipping_equals_eager's batches and geometry with a warm-up of 3, one power-of-two scale,
    decoupled decay and clipping on: the multipliers are static kernel arguments and the warm-up rides in the hyper rows, so four
    replayed steps leave parameters, moments and losses bit-identical to four eager steps"""
    from umpr_amd.graphs import GraphedTrainStep
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_batch, make_param_state
    from umpr_amd.train import train_step
    P = make_param_state(21, 50, 900, 1, True, m_scale=0.05)
    batches = [make_batch(30 + k, 6, 900, review_net_only=True, full_pad=True) for k in range(4)]
    gen = torch.Generator().manual_seed(77)
    for b in batches[1:]:
        b[3][:, -2:] = torch.randint(3, 20, b[3][:, -2:].shape, generator=gen)

    def fresh(max_norm, **kw):
        model = UMPR(_cfg(review_net_only=True), P["embedding.weight"].numpy())
        model.load_state_dict(P)
        model = model.to(dev)
        return model, FusedAdam(model, 1e-3, 0.5, max_grad_norm=max_norm, **kw)

    kw = dict(lr_scales={"review_net.r_net.": 0.25}, decoupled_decay=True, warmup_steps=3)
    model, opt = fresh(1e30, **kw)
    probe = []
    for b in batches[:2]:
        train_step(model, opt, b)
        probe.append(opt.clip_stats()["norm"])
    assert probe[0] != probe[1]
    max_norm = 0.5 * (probe[0] + probe[1])                                  # clips one of the first two steps for certain
    res = {}
    for mode in ("eager", "graph", "plain"):
        model, opt = fresh(max_norm, **({} if mode == "plain" else kw))
        if mode == "graph":
            g = GraphedTrainStep(model, opt, batches[0])
            losses = [float(g(b)[1].detach()) for b in batches]
        else:
            losses = [float(train_step(model, opt, b)[1].detach()) for b in batches]
        assert opt.step_count == 4
        res[mode] = (losses, opt.clip_stats(), _snap(opt))
    assert res["eager"][1]["clipped"] >= 1 and res["eager"][1]["seen"] == 4 and res["eager"][1]["skipped"] == 0
    assert res["eager"][0] == res["graph"][0] and res["eager"][1] == res["graph"][1]
    assert _same(res["eager"][2], res["graph"][2])
    assert not any(_eq(x, y) for x, y in zip(res["eager"][2], res["plain"][2]))   # and the options are not a no-op


def test_resume_inside_the_warm_up_is_exact(dev, tmp_path):
    """four steps equal two steps, save_checkpoint, load_checkpoint into a fresh model and optimiser, two steps - bit for bit, with
    a warm-up of 3 spanning the resume, scales and decoupled decay; the other settings refuse the file"""
    from umpr_amd.checkpoint import load_checkpoint, save_checkpoint
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_batch
    from umpr_amd.train import train_step
    batches = [make_batch(700 + j, 4, 1000, review_net_only=True) for j in range(4)]
    kw = dict(lr_scales={"review_net.r_net.": 0.25, "review_net.": 0.5}, wd_scales={"review_net.s_net_u.": 4.0},
              decoupled_decay=True, warmup_steps=3)
    path = str(tmp_path / "groups.pt")
    model = _umpr_r(dev)
    opt = FusedAdam(model, 1e-3, 0.5, **kw)
    for s, b in enumerate(batches):
        train_step(model, opt, b)
        if s == 1:
            save_checkpoint(path, model, opt, batch_counter=2)
    res_model = _umpr_r(dev)
    res = FusedAdam(res_model, 1e-3, 0.5, **kw)
    assert load_checkpoint(path, res_model, res, map_location=dev)["batch_counter"] == 2 and res.step_count == 2
    assert res.lr_at(3) == 1e-3 and res.lr_at(2) == 1e-3 * (2 / 3)
    for b in batches[2:]:
        train_step(res_model, res, b)
    assert _same(_snap(opt), _snap(res))
    other = FusedAdam(_umpr_r(dev), 1e-3, 0.5, **dict(kw, warmup_steps=0))
    with pytest.raises(ValueError, match="--warmup_steps"):
        load_checkpoint(path, other.model, other, map_location=dev)
    assert other.step_count == 0


def test_sparse_table_rows_take_the_multiplier_of_their_name(dev):
    """lr_scales={"embedding.": 0.5} on a sparse table: its rows and moments equal those of a twin built with lr / 2, every dense
    parameter equals a twin with the plain lr - bit for bit (halving is exact on both hosts)"""
    from umpr_amd.optim import FusedAdam
    from umpr_amd.synthetic import make_batch
    from umpr_amd.train import train_step
    batch = make_batch(500, 4, 1000, review_net_only=True)
    out = {}
    for what, lr, kw in (("scaled", 1e-3, dict(lr_scales={"embedding.": 0.5})), ("half", 5e-4, {}), ("plain", 1e-3, {})):
        model = _umpr_r(dev, train_embedding=True, sparse_embedding=True)
        opt = FusedAdam(model, lr, 1e-3, **kw)
        train_step(model, opt, batch)
        assert opt.sparse is not None
        out[what] = ([opt.sparse.table.detach().clone(), opt.sparse.m.clone(), opt.sparse.v.clone()], _snap(opt))
    assert _same(out["scaled"][0], out["half"][0]) and not _eq(out["scaled"][0][0], out["plain"][0][0])
    assert _same(out["scaled"][1], out["plain"][1]) and not _eq(out["scaled"][1][0], out["half"][1][0])


# ------------------------------------------------------------------------------------------------ the full model
PREFIX = "visual_net.vgg16."
SCALED = dict(lr_scales={PREFIX: 0.25}, wd_scales={PREFIX: 4.0})


@pytest.fixture(scope="module")
def full_state():
    from umpr_amd.synthetic import make_batch, make_param_state
    return make_param_state(121, 50, 500, 1, False, m_scale=0.05), [make_batch(130 + i, 2, 500, 1) for i in range(2)]


@pytest.fixture(scope="module", params=["fp32", "fp32_freeze_conv"])
def full(request, dev, full_state):
    """The full model (B = 2, one view, fp32; 138.6 M parameters, or its classifier's 123.6 M with the conv base frozen) built once
    per variant; every test restarts it from the same state."""
    from umpr_amd.model import UMPR
    P, batches = full_state
    model = UMPR(_cfg(views=["unknown"], freeze_conv=request.param == "fp32_freeze_conv"), P["embedding.weight"].numpy())
    model.load_state_dict(P)
    model = model.to(dev)
    return model, {k: v.detach().clone() for k, v in model.state_dict().items()}, batches


def _start(full, lr=1e-3, l2=1e-3, **kw):
    """A new optimiser on the model put back to its first state (dropout masks are a function of the seed and the call count)."""
    from umpr_amd.optim import FusedAdam
    model, start, _ = full
    torch.manual_seed(5)
    model.load_state_dict(start)
    for m in model.modules():
        if hasattr(m, "_calls"):
            m._calls = 0
    return FusedAdam(model, lr, l2, **kw)


def _twin_property(opt, scaled, quarter, plain):
    """arena elements of parameters under PREFIX (padding included) equal the twin built with lr / 4 and 4 l2, all others the twin
    with plain lr and l2, in p, m and v; both kinds exist and the twins differ on them"""
    from umpr_amd.optim import _pad
    for gi, g in enumerate(opt.groups):
        under = torch.zeros(g.numel, dtype=torch.bool, device=g.p.device)
        for n in g.names:
            if n.startswith(PREFIX):
                off, k = g.offsets[n]
                under[off:off + _pad(k)] = True
        assert under.any() and not under.all()
        for k in range(3):
            s, q, p = scaled[3 * gi + k], quarter[3 * gi + k], plain[3 * gi + k]
            assert _eq(s[under], q[under]) and _eq(s[~under], p[~under]), (gi, "pmv"[k])
            if k == 0:                                   # the twins differ on both kinds: neither comparison is vacuous
                assert not _eq(q[under], p[under]) and not _eq(q[~under], p[~under]), gi


@pytest.mark.parametrize("step_count", [0, 7])
def test_full_model_scaled_modules_equal_twins_built_with_the_scaled_rates(full, step_count):
    """One train_step (the early classifier update armed, and it ran) from a common state with lr_scales = {vgg: 0.25} and
    wd_scales = {vgg: 4}: the VGG's parameters and moments equal a twin built with lr * 0.25 and l2 * 4, all others a twin with
    plain lr and l2, bit for bit - powers of two make both host computations exact.  At step_count 0, and at 7 with non-zero
    moments loaded via load_state_dict."""
    from umpr_amd.train import train_step
    model, _, batches = full
    snaps = {}
    for what, lr, l2, kw in (("scaled", 1e-3, 1e-3, SCALED), ("quarter", 2.5e-4, 4e-3, {}), ("plain", 1e-3, 1e-3, {})):
        opt = _start(full, lr, l2, **kw)
        if step_count:
            state = {"step": step_count, "lr": lr, "base_lr": lr, "m": {}, "v": {}}
            for g in opt.groups:
                for n in g.names:
                    state["m"][n] = torch.full((g.offsets[n][1],), 0.01)
                    state["v"][n] = torch.full((g.offsets[n][1],), 1e-4)
            if kw:
                state["param_groups"] = {"lr_scale": {PREFIX: 0.25}, "wd_scale": {PREFIX: 4.0}, "decoupled_decay": False,
                                         "warmup_steps": 0}
            opt.load_state_dict(state)
            assert opt.step_count == 7
        seen, step = [], opt.step
        opt.step = lambda *a, _s=step, _o=opt, **k: (seen.append(_o._early_done is not None), _s(*a, **k))[1]
        train_step(model, opt, batches[0])
        assert seen == [True] and opt.step_count == step_count + 1          # the classifier slice was updated early
        snaps[what] = _snap(opt)
    assert sum(g.numel for g in opt.groups) > 120_000_000
    _twin_property(opt, snaps["scaled"], snaps["quarter"], snaps["plain"])


def test_full_model_combined_step_accumulated_clipped_averaged_and_scaled(full):
    """One optimiser step over two accumulated micro-batches with clipping (it clips), the moving average and the scales: the same
    twin property - every twin sees the same gradients, hence the same clip coefficient - and the average is a copy of the
    parameters after the first step and torch.lerp of it after a second"""
    from umpr_amd.train import train_step
    model, _, batches = full
    snaps = {}
    for what, lr, l2, kw in (("quarter", 2.5e-4, 4e-3, {}), ("plain", 1e-3, 1e-3, {}), ("scaled", 1e-3, 1e-3, SCALED)):
        opt = _start(full, lr, l2, max_grad_norm=1e-2, ema_decay=0.9, **kw)
        train_step(model, opt, batches[0], update=False)
        train_step(model, opt, batches[1])
        stats = opt.clip_stats()
        assert stats["clipped"] == 1 and stats["seen"] == 1 and opt.step_count == 1 and opt.pending == 0, stats
        snaps[what] = _snap(opt)
    _twin_property(opt, snaps["scaled"], snaps["quarter"], snaps["plain"])
    first = [g.p.clone() for g in opt.groups]
    assert all(_eq(a, p) for a, p in zip(opt._ema.arenas, first))
    train_step(model, opt, batches[0], update=False)
    train_step(model, opt, batches[1])
    for a, p1, g in zip(opt._ema.arenas, first, opt.groups):
        assert _eq(a.cpu(), torch.lerp(p1.cpu(), g.p.cpu(), 1.0 - 0.9)) and not _eq(p1, g.p)
