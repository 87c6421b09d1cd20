"""Gradient accumulation (FusedAdam.accumulate, train_step(update=), --accum_steps): everything that can be checked without a GPU -
the new entry point's declaration, the option and its refusals, the refusals of the optimiser, the step function and the graph
wrapper, and how training() groups loader batches into optimiser steps (stub model and optimiser)."""
import types

import numpy as np
import pytest
import torch

EMB = np.random.default_rng(0).standard_normal((30, 6)).astype(np.float32)


@pytest.fixture
def main_config():
    import main
    from umpr_amd.config import Config
    saved = Config._extra
    Config.extend(main.EXTRA_OPTIONS)
    yield lambda *argv: Config(argv=list(argv))
    Config._extra = saved


def _opt(main_config, *argv, **kw):
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    m = UMPR(main_config("--review_net_only", "True", *argv), EMB)
    return m, FusedAdam(m, 1e-3, 1e-3, **kw)


# ---- the entry point ------------------------------------------------------------------------------------------------------------
def test_grad_accumulate_is_declared_and_exported():
    import os
    from conftest import ROOT
    from umpr_amd._lib import SIGNATURES, lib
    assert SIGNATURES["umpr_grad_accumulate"] == ("pppiip", "i")
    header = open(os.path.join(ROOT, "include", "umpr_hip.h")).read()
    assert "int umpr_grad_accumulate(float* const* acc, const float* const* grads, const long* counts, int n_arenas, int first," \
        in header
    assert hasattr(lib().cdll, "umpr_grad_accumulate")


def test_grad_accumulate_refusals_and_no_ops_need_no_gpu():
    """everything refused is refused before any launch, and an empty table launches nothing: pure host work"""
    import ctypes
    from umpr_amd._lib import UmprHipError, lib
    L = lib()
    one_p, one_n = (ctypes.c_void_p * 1)(64), (ctypes.c_long * 1)(0)
    tp, tn = ctypes.addressof(one_p), ctypes.addressof(one_n)
    L.call("umpr_grad_accumulate", None, None, None, 0, 1, None)           # no arena
    L.call("umpr_grad_accumulate", tp, tp, tn, 1, 0, None)                 # one arena of no element
    null_p = (ctypes.c_void_p * 1)(None)
    L.call("umpr_grad_accumulate", ctypes.addressof(null_p), ctypes.addressof(null_p), tn, 1, 0, None)   # null with count 0
    for n in (-1, 9):
        with pytest.raises(UmprHipError, match="arenas outside 0..8"):
            L.call("umpr_grad_accumulate", tp, tp, tn, n, 0, None)
    for args in ((None, tp, tn), (tp, None, tn), (tp, tp, None)):
        with pytest.raises(UmprHipError, match="null arena table"):
            L.call("umpr_grad_accumulate", *args, 1, 0, None)
    neg, pos = (ctypes.c_long * 1)(-1), (ctypes.c_long * 1)(4)
    with pytest.raises(UmprHipError, match="bad pointer / count"):
        L.call("umpr_grad_accumulate", tp, tp, ctypes.addressof(neg), 1, 0, None)
    for a, g in ((null_p, one_p), (one_p, null_p)):
        with pytest.raises(UmprHipError, match="bad pointer / count"):
            L.call("umpr_grad_accumulate", ctypes.addressof(a), ctypes.addressof(g), ctypes.addressof(pos), 1, 0, None)
    odd = (ctypes.c_void_p * 1)(66)
    with pytest.raises(UmprHipError, match="not aligned to a float"):
        L.call("umpr_grad_accumulate", ctypes.addressof(odd), tp, tn, 1, 0, None)


# ---- the option -----------------------------------------------------------------------------------------------------------------
def test_accum_steps_flag(main_config):
    import main
    cfg = main_config()
    assert cfg.accum_steps == 1 and isinstance(cfg.accum_steps, int)
    main.check_flags(cfg)
    assert main_config("--accum_steps", "4").accum_steps == 4
    main.check_flags(main_config("--accum_steps", "4", "--grad_clip", "5.0", "--freeze_conv", "True", "--train_embedding", "True"))
    main.check_flags(main_config("--accum_steps", "1", "--train_embedding", "True", "--sparse_embedding", "True", "--grad_clip", "5.0",
                                 "--freeze_conv", "True", "--pool5_store_gb", "1"))
    for bad in ("0", "1.5", "-2", "True", "2.0"):
        with pytest.raises(SystemExit, match="--accum_steps takes a whole number >= 1"):
            main.check_flags(main_config("--accum_steps", bad))
    with pytest.raises(SystemExit, match="--accum_steps > 1 and --sparse_embedding True exclude each other"):
        main.check_flags(main_config("--accum_steps", "2", "--sparse_embedding", "True", "--train_embedding", "True"))


# ---- the optimiser, the step function, the graph wrapper ------------------------------------------------------------------------
def test_accumulate_needs_a_cuda_model(main_config):
    _, opt = _opt(main_config)
    assert opt.pending == 0 and opt.accum_arenas() is None
    with pytest.raises(RuntimeError, match="cuda"):
        opt.accumulate()
    assert opt.pending == 0 and opt.accum_arenas() is None


def test_accumulate_refuses_a_sparse_table_and_graph_mode(main_config):
    _, opt = _opt(main_config, "--train_embedding", "True", "--sparse_embedding", "True")
    assert opt.sparse is not None
    with pytest.raises(NotImplementedError, match="sparse table"):
        opt.accumulate()
    _, opt = _opt(main_config)
    opt._hyper = torch.zeros(len(opt.groups), 4)          # what enable_graph_mode leaves
    with pytest.raises(NotImplementedError, match="graph mode"):
        opt.accumulate()
    assert opt.pending == 0


def test_state_dict_keeps_its_keys(main_config):
    _, opt = _opt(main_config)
    assert sorted(opt.state_dict()) == ["base_lr", "lr", "m", "step", "v"]


class _Tiny(torch.nn.Module):
    """A model with a 'classifier' slice (what FusedAdam.early_bucket looks for) and the callback list the VGG module has."""

    def __init__(self):
        super().__init__()
        self.classifier = torch.nn.Linear(5, 3)
        self.other = torch.nn.Linear(3, 2)
        self.grad_callbacks = []


def test_no_early_update_is_armed_while_micro_batches_are_pending(monkeypatch):
    from umpr_amd import optim
    monkeypatch.setattr(optim, "_EARLY_ADAM", "1")
    opt = optim.FusedAdam(_Tiny(), 1e-3, 1e-3)
    assert opt.early_bucket() is not None
    opt.pending = 1
    opt.arm_early(1.0)
    assert opt._early is None
    opt.pending = 0
    opt.arm_early(1.0)
    assert opt._early == (1.0,)


def test_train_step_accumulates_on_one_rank_only(main_config):
    from umpr_amd.train import train_step
    m, opt = _opt(main_config)
    with pytest.raises(NotImplementedError, match="one rank only"):
        train_step(m, opt, None, world=2, update=False)
    with pytest.raises(NotImplementedError, match="one rank only"):
        train_step(m, opt, None, world=1, reducer=object(), update=False)
    opt.pending = 1                                         # a group is open: its closing step is refused as well
    with pytest.raises(NotImplementedError, match="one rank only"):
        train_step(m, opt, None, world=2)


def test_graphed_step_refuses_pending_micro_batches(main_config):
    from umpr_amd.graphs import GraphedTrainStep
    m, opt = _opt(main_config)
    opt.pending = 2
    with pytest.raises(NotImplementedError, match="single-batch steps"):
        GraphedTrainStep(m, opt, (None,) * 8)
    assert "single-batch steps" in GraphedTrainStep.__doc__


# ---- training(): loader batches -> optimiser steps ---------------------------------------------------------------------------------
class _StubOpt:
    max_grad_norm = 0.0

    def __init__(self, events):
        self.events, self.pending = events, 0

    def step(self):
        assert self.pending > 0
        self.events.append(f"step{self.pending}")
        self.pending = 0

    def epoch_end(self):
        self.events.append("epoch_end")


def _drive(monkeypatch, main_config, n_batches, k, meta=None):
    """training() over `n_batches` loader batches with every collaborator stubbed: the events in order, and (batch_counter,
    batch_in_epoch) of every checkpoint (validation after every optimiser step, each one better than the last)"""
    from umpr_amd import train
    events, saves, mse = [], [], [50.0]

    def train_step(model, opt, batch, world, reducer, update=True):
        events.append(("F", batch, update))
        if update and opt.pending == 0:
            events.append("plain")
        else:
            opt.pending += 1
            if update:
                opt.step()
        return torch.zeros(2), torch.zeros(())

    def evaluate(model, loader):
        mse[0] -= 1.0
        return mse[0]

    def save(path, model, opt, epoch, batch_counter, best_loss, batch_in_epoch=0, epoch_rng=None):
        assert opt.pending == 0                              # only ever right behind an optimiser step
        saves.append((batch_counter, batch_in_epoch))

    monkeypatch.setattr(train, "FusedAdam", lambda *a, **kw: _StubOpt(events))
    monkeypatch.setattr(train, "train_step", train_step)
    monkeypatch.setattr(train, "evaluate_mse", evaluate)
    monkeypatch.setattr(train, "save_checkpoint", save)
    monkeypatch.setattr(train, "load_checkpoint", lambda *a, **kw: meta)
    cfg = main_config("--accum_steps", str(k), "--valid_every", "1", "--train_epochs", "1")
    if meta is not None:
        cfg.resume = "stub"
    train.training(list(range(n_batches)), [], torch.nn.Linear(1, 1), cfg, "unused", logger=types.SimpleNamespace(info=lambda s: None))
    return events, saves


def test_training_groups_five_batches_by_two(monkeypatch, main_config):
    events, saves = _drive(monkeypatch, main_config, 5, 2)
    assert events == [("F", 0, False), ("F", 1, True), "step2", ("F", 2, False), ("F", 3, True), "step2", ("F", 4, False), "step1",
                      "epoch_end"]
    assert saves == [(1, 2), (2, 4), (3, 5)]                # batch_counter counts optimiser steps, batch_in_epoch loader batches


def test_training_without_accumulation_calls_what_it_called(monkeypatch, main_config):
    events, saves = _drive(monkeypatch, main_config, 3, 1)
    assert events == [("F", 0, True), "plain", ("F", 1, True), "plain", ("F", 2, True), "plain", "epoch_end"]
    assert saves == [(1, 1), (2, 2), (3, 3)]


def test_resumed_training_forms_the_same_groups(monkeypatch, main_config):
    events, saves = _drive(monkeypatch, main_config, 5, 2, meta={"epoch": 0, "batch_counter": 2, "batch_in_epoch": 4})
    assert events == [("F", 4, False), "step1", "epoch_end"] and saves == [(3, 5)]
    events, saves = _drive(monkeypatch, main_config, 5, 2, meta={"epoch": 0, "batch_counter": 1, "batch_in_epoch": 2})
    assert events == [("F", 2, False), ("F", 3, True), "step2", ("F", 4, False), "step1", "epoch_end"] and saves == [(2, 4), (3, 5)]


def test_training_refuses_accumulation_when_data_parallel(monkeypatch, main_config):
    from umpr_amd import parallel, train
    monkeypatch.setattr(parallel, "active", lambda: True)
    with pytest.raises(NotImplementedError, match="one rank only"):
        train.training([], [], torch.nn.Linear(1, 1), main_config("--accum_steps", "2"), "unused")
