"""Per-module learning rates, decoupled decay and warm-up (umpr_adam_step_groups, FusedAdam(lr_scales=, wd_scales=,
decoupled_decay=, warmup_steps=), --lr_scale / --wd_scale / --decoupled_decay / --warmup_steps): everything that can be checked
without a GPU - the options and their parsing, every refusal, the longest-prefix choice, the planner, the hyper rows under warm-up,
which entry point a range goes to (a stub in place of the library), the launcher's refusals, the checkpoint, and the float64
restatement the kernel tests use (tests/adam_groups_reference.py) against torch.optim.Adam / AdamW with param groups."""
import ctypes
import math

import numpy as np
import pytest
import torch

from adam_groups_reference import adam_groups_step

EMB = np.random.default_rng(0).standard_normal((30, 6)).astype(np.float32)


@pytest.fixture
def main_config():
    import main
    from umpr_amd.config import Config
    saved = Config._extra
    Config.extend(main.EXTRA_OPTIONS)
    yield lambda *argv: Config(argv=list(argv))
    Config._extra = saved


def _opt(main_config, *argv, lr=1e-3, l2=1e-3, **kw):
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    m = UMPR(main_config("--review_net_only", "True", *argv), EMB)
    return m, FusedAdam(m, lr, l2, **kw)


# ---- the options ------------------------------------------------------------------------------------------------------------------
def test_options_defaults_and_parsing(main_config):
    import main
    from umpr_amd.optim import parse_scales
    assert {k: main.EXTRA_OPTIONS[k] for k in ("lr_scale", "wd_scale", "decoupled_decay", "warmup_steps")} == \
        {"lr_scale": "", "wd_scale": "", "decoupled_decay": False, "warmup_steps": 0}
    cfg = main_config()
    assert (cfg.lr_scale, cfg.wd_scale, cfg.decoupled_decay, cfg.warmup_steps) == ("", "", False, 0)
    main.check_flags(cfg)
    cfg = main_config("--lr_scale", "visual_net.vgg16.=1e-3,embedding.=0.1", "--wd_scale", "embedding.=0", "--decoupled_decay", "True",
                      "--warmup_steps", "500")
    main.check_flags(cfg)
    assert parse_scales(cfg.lr_scale) == {"visual_net.vgg16.": 1e-3, "embedding.": 0.1}
    assert parse_scales(cfg.wd_scale) == {"embedding.": 0.0} and cfg.decoupled_decay is True and cfg.warmup_steps == 500
    assert parse_scales("") == {} and parse_scales(" a.b = 2 , c=0.5,") == {"a.b": 2.0, "c": 0.5}
    for bad, what in (("a.b", "is not <name prefix>=<multiplier>"), ("=2", "is not <name prefix>=<multiplier>"),
                      ("a=1,a=2", "the prefix 'a' is given twice"), ("a=x", "the prefix 'a' is no number")):
        with pytest.raises(ValueError, match=what):
            parse_scales(bad, "lr_scale")
        with pytest.raises(SystemExit, match="--lr_scale"):
            main.check_flags(main_config("--lr_scale", bad))
    for option, bad in (("lr_scale", "a=0"), ("lr_scale", "a=-1"), ("lr_scale", "a=inf"), ("lr_scale", "a=nan"),
                        ("wd_scale", "a=-1"), ("wd_scale", "a=inf"), ("wd_scale", "a=nan")):
        with pytest.raises(SystemExit, match=f"--{option}: the multiplier of the prefix 'a' must be finite"):
            main.check_flags(main_config("--" + option, bad))
    with pytest.raises(SystemExit, match="--decoupled_decay takes True or False"):
        main.check_flags(main_config("--decoupled_decay", "1"))
    for bad in ("-1", "2.5", "True"):
        with pytest.raises(SystemExit, match="--warmup_steps takes a whole number >= 0"):
            main.check_flags(main_config("--warmup_steps", bad))


# ---- the optimiser's refusals and the longest prefix ------------------------------------------------------------------------------
def test_every_refusal_names_its_prefix(main_config):
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match=r"lr_scales: the multiplier of the prefix 'review_net\.' must be finite and > 0"):
            _opt(main_config, lr_scales={"review_net.": bad})
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(ValueError, match=r"wd_scales: the multiplier of the prefix 'review_net\.' must be finite and >= 0"):
            _opt(main_config, wd_scales={"review_net.": bad})
    with pytest.raises(ValueError, match=r"lr_scales: the prefix 'reviev_net\.' matches no trainable parameter"):
        _opt(main_config, lr_scales={"review_net.": 0.5, "reviev_net.": 0.5})
    with pytest.raises(ValueError, match=r"lr_scales: the prefix 'embedding\.' matches no trainable parameter"):
        _opt(main_config, lr_scales={"embedding.": 0.5})                   # frozen by default: not trainable
    with pytest.raises(ValueError, match=r"wd_scales: the prefix 'visual_net\.' matches no parameter with weight decay"):
        _opt(main_config, wd_scales={"visual_net.": 0.5})
    with pytest.raises(ValueError, match=r"wd_scales: the prefix 'linear_fusion\.0\.bias' matches no parameter with weight decay "
                                         r"\(bias parameters and a sparse table have none\)"):
        _opt(main_config, wd_scales={"linear_fusion.0.bias": 0.5})
    with pytest.raises(ValueError, match="decoupled_decay must be True or False"):
        _opt(main_config, decoupled_decay=1)
    for bad in (-1, 2.5, True):
        with pytest.raises(ValueError, match="warmup_steps must be a whole number >= 0"):
            _opt(main_config, warmup_steps=bad)
    # zero is a legitimate decay multiplier, and a trainable table is a trainable parameter
    _opt(main_config, wd_scales={"linear_fusion.": 0.0})
    _, opt = _opt(main_config, "--train_embedding", "True", lr_scales={"embedding.": 0.1}, wd_scales={"embedding.": 0.0})
    assert opt.param_multipliers()["embedding.weight"] == (0.1, 0.0)
    # a sparse table takes the learning-rate multiplier of its name and has no decay to scale
    _, opt = _opt(main_config, "--train_embedding", "True", "--sparse_embedding", "True", lr_scales={"embedding.": 0.5})
    assert opt.sparse is not None and opt.param_multipliers()["embedding.weight"] == (0.5, 1.0)
    with pytest.raises(ValueError, match=r"wd_scales: the prefix 'embedding\.' matches no parameter with weight decay \(bias"):
        _opt(main_config, "--train_embedding", "True", "--sparse_embedding", "True", wd_scales={"embedding.": 0.0})


def test_longest_prefix_wins(main_config):
    from umpr_amd.optim import match_scale
    assert match_scale("a.b.c", {"a.": 2.0, "a.b.": 3.0, "a.b.c.d": 4.0, "b.": 5.0}) == (3.0, "a.b.")
    assert match_scale("x", {"a.": 2.0}) == (1.0, None) and match_scale("x", {}) == (1.0, None)
    _, opt = _opt(main_config, lr_scales={"review_net.": 0.5, "review_net.r_net.": 0.25, "review_net.r_net.M": 8.0},
                  wd_scales={"review_net.s_net_u.": 4.0, "linear_fusion.": 0.0})
    mult = opt.param_multipliers()
    assert set(mult) == {n for n, p in opt.model.named_parameters() if p.requires_grad}
    assert mult["review_net.r_net.M"] == (8.0, 1.0)
    assert mult["review_net.r_net.gru.module.weight_hh_l0"] == (0.25, 1.0)
    assert mult["review_net.r_net.gru.module.bias_hh_l0"] == (0.25, 1.0)
    assert mult["review_net.s_net_u.Ms"] == (0.5, 4.0) and mult["review_net.s_net_i.Ms"] == (0.5, 1.0)
    assert mult["linear_fusion.0.weight"] == (1.0, 0.0) and mult["linear_fusion.0.bias"] == (1.0, 0.0)
    summary = opt.group_summary()
    assert "lr_scale 'review_net.r_net.' = 0.25: 8 parameters" in summary and "lr_scale 'review_net.r_net.M' = 8: 1 parameters" in summary
    assert any(ln.startswith("group 0 (weights, 12 parameters): ") for ln in summary)


# ---- the planner ------------------------------------------------------------------------------------------------------------------
def _check_plan(opt, gi, lo, hi, launches):
    """the launches tile [lo, hi) in order, hold 1..16 segments each, every end but a launch's last is a multiple of 64, and every
    element gets the multipliers of the parameter it (or the padding it lies in) belongs to"""
    from umpr_amd.optim import MAX_SEGMENTS, _pad
    g, mult = opt.groups[gi], opt.param_multipliers()
    want = np.ones((g.numel, 2))
    for n in g.names:
        off, k = g.offsets[n]
        want[off:off + _pad(k)] = mult[n] if g.weight_decay != 0.0 else (mult[n][0], 1.0)
    at = lo
    for l, h, segs in launches:
        assert l == at and h > l and 1 <= len(segs) <= MAX_SEGMENTS
        prev = 0
        for k, (end, a, w) in enumerate(segs):
            assert end > prev and (end % 64 == 0 or k == len(segs) - 1)
            assert (want[l + prev:l + end] == (a, w)).all(), (l, prev, end, a, w)
            prev = end
        assert prev == h - l
        at = h
    assert at == hi


def test_planner_merges_neighbours_and_cuts_through_a_slice(main_config):
    _, opt = _opt(main_config, lr_scales={"review_net.r_net.": 0.25, "review_net.": 0.5}, wd_scales={"linear_fusion.": 0.0})
    g = opt.groups[0]
    # five r_net weights, six other review_net weights, the fusion weight: three segments, not twelve
    whole = opt.plan(0, 0, g.numel)
    assert whole == [(0, g.numel, [(g.offsets["review_net.s_net_u.Ms"][0], 0.25, 1.0),
                                   (g.offsets["linear_fusion.0.weight"][0], 0.5, 1.0), (g.numel, 1.0, 0.0)])]
    _check_plan(opt, 0, 0, g.numel, whole)
    # the bias group has no decay: its segments ignore the decay multiplier
    assert [s for _, _, s in opt.plan(1, 0, opt.groups[1].numel)] == [[(768, 0.25, 1.0), (832, 1.0, 1.0)]]
    # ranges as the early classifier update leaves them: a slice in the middle of a segment, and what lies around it
    lo, hi = g.offsets["review_net.r_net.gru.module.weight_hh_l0"][0], g.offsets["review_net.s_net_i.Ms"][0]
    assert opt.plan(0, lo, hi) == [(lo, hi, [(g.offsets["review_net.s_net_u.Ms"][0] - lo, 0.25, 1.0), (hi - lo, 0.5, 1.0)])]
    for a, b in ((0, lo), (lo, hi), (hi, g.numel), (lo + 64, lo + 128), (lo, lo + 1)):
        _check_plan(opt, 0, a, b, opt.plan(0, a, b))
    # a range that starts off a 64-float boundary: the floats up to the boundary are a launch of their own
    odd = opt.plan(0, lo + 5, hi - 3)
    assert [(l, h) for l, h, _ in odd] == [(lo + 5, lo + 64), (lo + 64, hi - 3)] and len(odd[0][2]) == 1
    _check_plan(opt, 0, lo + 5, hi - 3, odd)
    _check_plan(opt, 0, lo + 5, lo + 9, opt.plan(0, lo + 5, lo + 9))
    assert opt.plan(0, lo, lo) == []


def test_planner_splits_seventeen_segments_into_sixteen_and_one(main_config):
    _, probe = _opt(main_config)
    names = probe.groups[0].names + probe.groups[1].names
    assert len(names) == 17
    scales = {n: 1.0 + 0.125 * k for k, n in enumerate(names)}              # every parameter its own multiplier
    _, opt = _opt(main_config, lr_scales=scales)
    assert [len(opt.plan(gi, 0, g.numel)[0][2]) for gi, g in enumerate(opt.groups)] == [12, 5]
    # one arena of 17 parameters: order_key puts nothing first, and no name holds 'bias' once the groups are merged by hand
    g = opt.groups[0]
    g.names, g.offsets, off = list(names), {}, 0
    for k, n in enumerate(names):
        g.offsets[n] = (off, 100 + k)
        off += 128
    g.numel = off
    launches = opt.plan(0, 0, g.numel)
    assert [len(s) for _, _, s in launches] == [16, 1] and [(l, h) for l, h, _ in launches] == [(0, 16 * 128), (16 * 128, 17 * 128)]
    assert launches[1][2] == [(128, scales[names[16]], 1.0)]
    _check_plan(opt, 0, 0, g.numel, launches)
    assert sum(len(s) for _, _, s in opt.plan(0, 64, g.numel - 64)) == 17
    _check_plan(opt, 0, 64, g.numel - 64, opt.plan(0, 64, g.numel - 64))
    assert "group 0 (weights, 17 parameters): 17 segments in 2 launches" in opt.group_summary()


# ---- the scalars ------------------------------------------------------------------------------------------------------------------
def test_hyper_rows_under_warm_up(main_config):
    N, lr, l2 = 4, 2e-3, 0.5
    for decoupled in (False, True):
        _, opt = _opt(main_config, lr=lr, l2=l2, warmup_steps=N, decoupled_decay=decoupled)
        _, plain = _opt(main_config, lr=lr, l2=l2)
        for t in (1, N, N + 1):
            opt.step_count = plain.step_count = t - 1
            f = min(1.0, t / N)
            rows, ref = opt.hyper_rows(0.25), plain.hyper_rows(0.25)
            assert opt.lr_at(t) == lr * f and plain.lr_at(t) == lr
            for gi, wd in ((0, l2), (1, 0.0)):
                assert rows[gi][0] == 0.25 and rows[gi][2] == ref[gi][2] == 1.0 / math.sqrt(1.0 - 0.999 ** t)
                assert rows[gi][1] == lr * f / (1.0 - 0.9 ** t) and ref[gi][1] == lr / (1.0 - 0.9 ** t)
                assert rows[gi][3] == (lr * f * wd if decoupled else wd) and ref[gi][3] == wd
            assert len(rows) == 2 and all(len(r) == 4 for r in rows)
            if t >= N:
                assert rows[0][1] == ref[0][1]                               # from step N on the rate is the plain one, bit for bit


class _StubLib:
    def __init__(self):
        self.calls = []

    def call(self, name, *args):
        self.calls.append((name, args))


def _route(monkeypatch, opt, step=1, clip_state=None, hyper=None, lo=0, hi=None):
    from umpr_amd import optim
    stub = _StubLib()
    monkeypatch.setattr(optim, "lib", lambda: stub)
    monkeypatch.setattr(optim, "stream_ptr", lambda: 77)
    opt._hyper = hyper
    for gi, g in enumerate(opt.groups):
        opt._adam(gi, lo, g.numel if hi is None else hi, g.g, step, 0.5, clip_state)
    return stub.calls


def test_defaults_and_warm_up_alone_call_the_old_entry_points_with_the_old_arguments(monkeypatch, main_config):
    state, hyper = torch.zeros(8), torch.zeros(2, 4)
    for kw, lr_at_1 in (({}, 1e-3), ({"warmup_steps": 4}, 1e-3 * 0.25), ({"lr_scales": {"review_net.": 1.0}}, 1e-3)):
        _, opt = _opt(main_config, **kw)
        for clip in (None, state):
            calls = _route(monkeypatch, opt, clip_state=clip)
            assert [c[0] for c in calls] == ["umpr_adam_step" if clip is None else "umpr_adam_step_clip"] * 2
            for (name, args), g in zip(calls, opt.groups):
                assert [a.data_ptr() for a in args[:4]] == [g.p.data_ptr(), g.g.data_ptr(), g.m.data_ptr(), g.v.data_ptr()]
                assert args[4:12] == (g.numel, lr_at_1, 0.9, 0.999, 1e-8, g.weight_decay, 1, 0.5)
                assert args[12:] == ((77,) if clip is None else (clip, 77))
            calls = _route(monkeypatch, opt, clip_state=clip, hyper=hyper)
            assert [c[0] for c in calls] == ["umpr_adam_step_dev" if clip is None else "umpr_adam_step_dev_clip"] * 2
            for gi, (name, args) in enumerate(calls):
                assert args[4:8] == (opt.groups[gi].numel, 0.9, 0.999, 1e-8) and args[8].data_ptr() == hyper[gi].data_ptr()
                assert args[9:] == ((77,) if clip is None else (clip, 77))
        assert sorted(opt.state_dict())[:2] == ["base_lr", "lr"]


def test_a_multiplier_or_decoupled_decay_calls_the_new_entry_point(monkeypatch, main_config):
    state, hyper = torch.zeros(8), torch.zeros(2, 4)

    def table(addr, ctype, n):
        return list((ctype * n).from_address(addr))

    _, opt = _opt(main_config, lr_scales={"review_net.r_net.": 0.25}, wd_scales={"review_net.": 4.0}, warmup_steps=2)
    for clip in (None, state):
        for hyp in (None, hyper):
            calls = _route(monkeypatch, opt, clip_state=clip, hyper=hyp)
            assert [c[0] for c in calls] == ["umpr_adam_step_groups"] * 2
            for gi, (name, args) in enumerate(calls):
                g = opt.groups[gi]
                assert args[4:12] == (g.numel, 1e-3 * 0.5, 0.9, 0.999, 1e-8, g.weight_decay, 1, 0.5)
                assert (args[12] is None) == (hyp is None) and (hyp is None or args[12].data_ptr() == hyper[gi].data_ptr())
                assert args[13] is clip and args[18:] == (0, 77)
                n_segs = args[17]
                segs = list(zip(table(args[14], ctypes.c_long, n_segs), table(args[15], ctypes.c_float, n_segs),
                                table(args[16], ctypes.c_float, n_segs)))
                assert segs == opt.plan(gi, 0, g.numel)[0][2]
                assert segs == ([(43264, 0.25, 4.0), (125312, 1.0, 4.0), (125440, 1.0, 1.0)] if gi == 0 else
                                [(768, 0.25, 1.0), (832, 1.0, 1.0)])
    # a range whose multipliers are all 1 still goes to the old entry point: only the fusion layer's weight
    lo = opt.groups[0].offsets["linear_fusion.0.weight"][0]
    opt._hyper = None
    from umpr_amd import optim
    stub = _StubLib()
    monkeypatch.setattr(optim, "lib", lambda: stub)
    opt._adam(0, lo, opt.groups[0].numel, opt.groups[0].g, 5, 1.0, None)
    assert [c[0] for c in stub.calls] == ["umpr_adam_step"] and stub.calls[0][1][4:6] == (128, 1e-3)
    # decoupled decay alone: one segment of (1, 1) per group, the flag set
    _, opt = _opt(main_config, decoupled_decay=True)
    calls = _route(monkeypatch, opt)
    assert [c[0] for c in calls] == ["umpr_adam_step_groups"] * 2
    for gi, (name, args) in enumerate(calls):
        assert args[17:] == (1, 1, 77) and table(args[14], ctypes.c_long, 1) == [opt.groups[gi].numel]
        assert table(args[15], ctypes.c_float, 1) == [1.0] and table(args[16], ctypes.c_float, 1) == [1.0]


def test_sparse_table_takes_its_multiplier_on_the_host(monkeypatch, main_config):
    from umpr_amd import optim
    for kw, want in (({}, 1e-3), ({"lr_scales": {"embedding.": 0.5}}, 5e-4), ({"lr_scales": {"embedding.": 0.5}, "warmup_steps": 4}, 2.5e-4)):
        m, opt = _opt(main_config, "--train_embedding", "True", "--sparse_embedding", "True", **kw)
        stub = _StubLib()
        monkeypatch.setattr(optim, "lib", lambda: stub)
        monkeypatch.setattr(optim, "stream_ptr", lambda: 77)
        m._sparse_rows = type("R", (), {"row_id": torch.zeros(2, dtype=torch.int64), "row_grad": torch.zeros(2, 6), "T": 2})()
        opt.step_count = 2
        opt._step_sparse(1.0, None)
        (name, args), = stub.calls
        assert name == "umpr_sparse_adam_rows" and args[8] == want and args[12:14] == (2, 1.0)


# ---- the launcher's refusals (host work: nothing is launched) ------------------------------------------------------------------------
def test_launcher_refuses_a_bad_segment_table_before_any_launch():
    from umpr_amd._lib import SIGNATURES, UmprHipError, lib
    assert SIGNATURES["umpr_adam_step_groups"] == ("ppppldddddld" "pp" "ppp" "ii" "p", "i")
    L = lib()

    def call(n, ends, lr_mult=None, wd_mult=None, n_segs=None, step=1):
        k = max(len(ends), 1)
        e = (ctypes.c_long * k)(*ends)
        a = (ctypes.c_float * k)(*(lr_mult or [1.0] * len(ends)))
        w = (ctypes.c_float * k)(*(wd_mult or [1.0] * len(ends)))
        L.call("umpr_adam_step_groups", 256, 256, 256, 256, n, 1e-3, 0.9, 0.999, 1e-8, 1e-3, step, 1.0, None, None,
               ctypes.addressof(e), ctypes.addressof(a), ctypes.addressof(w), len(ends) if n_segs is None else n_segs, 0, None)

    call(0, [])                                                            # nothing to do: a successful no-op
    with pytest.raises(UmprHipError, match="adam_groups: 17 segments outside 1..16"):
        call(17 * 64, [64 * (k + 1) for k in range(17)])
    with pytest.raises(UmprHipError, match="adam_groups: 0 segments outside 1..16"):
        call(64, [])
    with pytest.raises(UmprHipError, match="adam_groups: segment 0 ends at 65, not a multiple of 64 elements"):
        call(128, [65, 128])
    with pytest.raises(UmprHipError, match="adam_groups: the last segment ends at 128, not at n = 129"):
        call(129, [64, 128])
    with pytest.raises(UmprHipError, match="adam_groups: segment 1 ends at 192: not behind 64 or past n = 128"):
        call(128, [64, 192])
    with pytest.raises(UmprHipError, match="adam_groups: segment 1 ends at 64: not behind 64"):
        call(128, [64, 64])
    with pytest.raises(UmprHipError, match="adam_groups: segment 0 ends at 0: not behind 0"):
        call(128, [0, 128])
    for bad in (0.0, -1.0, float("inf"), float("nan")):
        with pytest.raises(UmprHipError, match="adam_groups: segment 1: learning-rate multiplier .* is not finite and > 0"):
            call(128, [64, 128], lr_mult=[1.0, bad])
    for bad in (-1.0, float("inf"), float("nan")):
        with pytest.raises(UmprHipError, match="adam_groups: segment 0: decay multiplier .* is not finite and >= 0"):
            call(128, [64, 128], wd_mult=[bad, 1.0])
    with pytest.raises(UmprHipError, match="adam_groups: bad step/n"):
        call(128, [128], step=0)
    with pytest.raises(UmprHipError, match="adam_groups: bad step/n"):
        call(-1, [128])
    with pytest.raises(UmprHipError, match="adam_groups: null segment table"):
        L.call("umpr_adam_step_groups", 256, 256, 256, 256, 64, 1e-3, 0.9, 0.999, 1e-8, 1e-3, 1, 1.0, None, None, None, None, None, 1,
               0, None)


# ---- the checkpoint ---------------------------------------------------------------------------------------------------------------
SETTINGS = {"lr_scales": {"review_net.r_net.": 0.25}, "wd_scales": {"linear_fusion.": 0.0}, "decoupled_decay": True, "warmup_steps": 3}


def test_state_dict_round_trip_and_refusals(main_config, tmp_path):
    from umpr_amd.checkpoint import load_checkpoint, save_checkpoint
    m, opt = _opt(main_config, **SETTINGS)
    st = opt.state_dict()
    assert sorted(st) == ["base_lr", "lr", "m", "param_groups", "step", "v"]
    assert st["param_groups"] == {"lr_scale": {"review_net.r_net.": 0.25}, "wd_scale": {"linear_fusion.": 0.0},
                                  "decoupled_decay": True, "warmup_steps": 3}
    opt.step_count = 2
    path = str(tmp_path / "groups.pt")
    save_checkpoint(path, m, opt)
    m2, again = _opt(main_config, **SETTINGS)
    load_checkpoint(path, m2, again)                                       # through torch.load(weights_only=True)
    assert again.step_count == 2 and again.lr_at(again.step_count + 1) == 1e-3 and again.state_dict()["param_groups"] == st["param_groups"]
    # each single setting alone is written, and each mismatch is refused by name, both ways, before anything is loaded
    _, plain = _opt(main_config)
    assert "param_groups" not in plain.state_dict()
    for key, option in (("lr_scales", "lr_scale"), ("wd_scales", "wd_scale"), ("decoupled_decay", "decoupled_decay"),
                        ("warmup_steps", "warmup_steps")):
        _, one = _opt(main_config, **{key: SETTINGS[key]})
        assert "param_groups" in one.state_dict()
        other = dict(SETTINGS, **{key: {"lr_scales": {"review_net.r_net.": 0.5}, "wd_scales": {"linear_fusion.": 2.0},
                                        "decoupled_decay": False, "warmup_steps": 4}[key]})
        _, differs = _opt(main_config, **other)
        for run, ck in ((plain, one), (one, plain), (differs, opt), (opt, differs)):
            written = ck.state_dict()
            written["step"] = 9
            with pytest.raises(ValueError, match=f"written with --{option} .*, this run has --{option} .*: pass the same --{option}"):
                run.check_state_dict(written)
            with pytest.raises(ValueError, match=f"--{option}"):
                run.load_state_dict(written)
            assert run.step_count in (0, 2)
    with pytest.raises(ValueError, match="--lr_scale 'review_net.r_net.=0.25', this run has --lr_scale ''"):
        plain.check_state_dict(st)
    # a checkpoint from before the key existed is one written with the defaults
    old = plain.state_dict()
    assert sorted(old) == ["base_lr", "lr", "m", "step", "v"]
    plain.check_state_dict(old)
    plain.load_state_dict(old)
    with pytest.raises(ValueError, match="--lr_scale"):
        opt.check_state_dict(old)


# ---- training() -------------------------------------------------------------------------------------------------------------------
def test_training_passes_the_options_on_only_when_they_are_set(monkeypatch, main_config):
    import types
    from umpr_amd import train
    made, lines = [], []

    class Opt:
        max_grad_norm, pending, decoupled_decay, warmup_steps = 0.0, 0, True, 500

        def epoch_end(self):
            pass

        def group_summary(self):
            return ["lr_scale 'review_net.' = 0.5: 15 parameters", "group 0 (weights, 12 parameters): 2 segments in 1 launches"]

    def make(*a, **kw):
        made.append(kw)
        return Opt()

    monkeypatch.setattr(train, "FusedAdam", make)
    monkeypatch.setattr(train, "evaluate_mse", lambda model, loader: 1.0)
    run = lambda *argv: train.training([], [], torch.nn.Linear(1, 1), main_config("--train_epochs", "1", *argv), "unused",
                                       logger=types.SimpleNamespace(info=lines.append))
    run()
    assert made == [{"max_grad_norm": 0.0}] and not any("segments" in ln or "Optimiser" in ln for ln in lines)
    run("--lr_scale", "review_net.=0.5", "--wd_scale", "linear_fusion.=0", "--decoupled_decay", "True", "--warmup_steps", "500")
    assert made[1] == {"max_grad_norm": 0.0, "lr_scales": {"review_net.": 0.5}, "wd_scales": {"linear_fusion.": 0.0},
                       "decoupled_decay": True, "warmup_steps": 500}
    assert any("decoupled weight decay (AdamW), linear warm-up over 500 steps" in ln for ln in lines)
    assert any("lr_scale 'review_net.' = 0.5: 15 parameters" in ln for ln in lines) and any("2 segments in 1 launches" in ln for ln in lines)
    run("--warmup_steps", "7")
    assert made[2] == {"max_grad_norm": 0.0, "warmup_steps": 7}


# ---- the yardstick ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("decoupled", [False, True])
def test_float64_restatement_equals_torch_adam_and_adamw_with_param_groups(decoupled):
    """three steps, three tensors with their own (a, w), a warm-up of 2 and a gradient scale, in double: torch.optim.Adam /
    torch.optim.AdamW with one param group per tensor (the group's lr set per step, as a scheduler would) against the
    restatement on one flat array with per-element multipliers.  1e-13 relative, a dozen double roundings, or 1e-15 absolute
    where a moment is a sum of terms of order one that cancel."""
    lr, wd, N, scale = 1e-2, 0.3, 2, 0.5
    mults = [(0.25, 4.0), (1.0, 0.0), (3.0, 1.0)]
    gen = torch.Generator().manual_seed(4)
    ps = [torch.randn(70, generator=gen, dtype=torch.float64).requires_grad_(True) for _ in mults]
    grads = [[torch.randn(70, generator=gen, dtype=torch.float64) for _ in mults] for _ in range(3)]
    flat = np.concatenate([p.detach().numpy() for p in ps])
    a = np.concatenate([np.full(70, a) for a, _ in mults])
    w = np.concatenate([np.full(70, w) for _, w in mults])
    m, v = np.zeros_like(flat), np.zeros_like(flat)
    opt = (torch.optim.AdamW if decoupled else torch.optim.Adam)(
        [{"params": [p], "lr": lr * a_, "weight_decay": wd * w_} for p, (a_, w_) in zip(ps, mults)], lr=lr)
    for t in (1, 2, 3):
        for p, g_, grp, (a_, _) in zip(ps, grads[t - 1], opt.param_groups, mults):
            p.grad = scale * g_
            grp["lr"] = lr * min(1.0, t / N) * a_
        opt.step()
        flat, m, v = adam_groups_step(flat, np.concatenate([g_.numpy() for g_ in grads[t - 1]]), m, v, t, lr, wd, a, w,
                                      decoupled=decoupled, warmup_steps=N, grad_scale=scale)
        ref = np.concatenate([p.detach().numpy() for p in ps])
        ref_m = np.concatenate([opt.state[p]["exp_avg"].numpy() for p in ps])
        ref_v = np.concatenate([opt.state[p]["exp_avg_sq"].numpy() for p in ps])
        for name, got, want in (("p", flat, ref), ("m", m, ref_m), ("v", v, ref_v)):
            assert np.allclose(got, want, rtol=1e-13, atol=1e-15), (t, name, np.abs(got - want).max())
    # and the two modes are not each other: the yardstick separates what the tests have to separate
    other = adam_groups_step(flat, grads[0][0].numpy().repeat(3), m, v, 4, lr, wd, a, w, decoupled=not decoupled)[0]
    this = adam_groups_step(flat, grads[0][0].numpy().repeat(3), m, v, 4, lr, wd, a, w, decoupled=decoupled)[0]
    assert np.abs(other - this).max() > 1e-4
