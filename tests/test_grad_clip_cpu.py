"""Gradient clipping by global norm (FusedAdam(max_grad_norm=), --grad_clip): everything that can be checked without a GPU - the
argument's validation, the command-line option, and that the early classifier update stays off while clipping is on."""
import pytest
import torch


class _Tiny(torch.nn.Module):
    """A model with a 'classifier' slice (what FusedAdam.early_bucket looks for) and the callback list the VGG module has."""

    def __init__(self):
        super().__init__()
        self.classifier = torch.nn.Linear(5, 3)
        self.other = torch.nn.Linear(3, 2)
        self.grad_callbacks = []


def _opt(**kw):
    from umpr_amd.optim import FusedAdam
    torch.manual_seed(0)
    return FusedAdam(_Tiny(), 1e-3, 1e-3, **kw)


@pytest.mark.parametrize("bad", [-1.0, -1e-30, float("inf"), float("-inf"), float("nan")])
def test_max_grad_norm_rejects_negative_and_non_finite_values(bad):
    with pytest.raises(ValueError):
        _opt(max_grad_norm=bad)


def test_max_grad_norm_zero_is_off_and_the_default():
    assert _opt().max_grad_norm == 0.0
    assert _opt(max_grad_norm=0).max_grad_norm == 0.0
    assert _opt(max_grad_norm=0).clip_state is None
    assert _opt(max_grad_norm=5).max_grad_norm == 5.0
    with pytest.raises(RuntimeError):
        _opt().clip_stats()


def test_config_parses_grad_clip_after_extend():
    from umpr_amd.config import Config
    Config.extend({"grad_clip": 0.0})
    assert Config(argv=[]).grad_clip == 0.0
    cfg = Config(argv=["--grad_clip", "5.0"])
    assert cfg.grad_clip == 5.0 and isinstance(cfg.grad_clip, float)


def test_main_registers_grad_clip():
    import os
    from conftest import ROOT
    src = open(os.path.join(ROOT, "main.py")).read()
    assert '"grad_clip": 0.0' in src


def test_early_update_stays_off_while_clipping():
    opt = _opt(max_grad_norm=1.0)
    assert opt.early_bucket() is not None
    before = [(g.p.clone(), g.m.clone(), g.v.clone()) for g in opt.groups]
    opt.arm_early(1.0)
    assert opt._early is None
    opt.early_step(())
    opt._on_classifier_grads()
    assert opt._early is None and opt._early_done is None
    for g, (p, m, v) in zip(opt.groups, before):
        assert torch.equal(g.p, p) and torch.equal(g.m, m) and torch.equal(g.v, v)


def test_early_update_arms_as_before_with_clipping_off(monkeypatch):
    from umpr_amd import optim
    monkeypatch.setattr(optim, "_EARLY_ADAM", "1")
    opt = _opt()
    opt.arm_early(0.5)
    assert opt._early == (0.5,) and opt._early_done is None
    opt.disarm()
    assert opt._early is None


def test_training_log_lines_are_unchanged_with_clipping_off():
    from umpr_amd.train import clip_note
    assert clip_note(_opt()) == ""
