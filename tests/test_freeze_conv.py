"""Frozen conv base (UMPR(freeze_conv=True), main.py --freeze_conv / --pool5_store_gb), host half: main.py's flag checks, which
parameters train and what the optimiser builds for them, the fingerprint a Pool5Store keeps (conv parameters only), and the refusal
of an optimiser state written under the other setting.  No GPU needed."""
import numpy as np
import pytest
import torch

from test_feature_store import _cfg, main_config  # noqa: F401  (fixture)

EMB = np.zeros((40, 50), dtype=np.float32)
PRE = "visual_net.vgg16.0."


# ---- main.py --------------------------------------------------------------------------------------------------------------------
def test_main_flags(main_config):
    import main
    cfg = main_config()
    assert cfg.freeze_conv is False and cfg.pool5_store_gb == 0.0
    main.check_flags(cfg)
    cfg = main_config("--freeze_conv", "True", "--pool5_store_gb", "0.5")
    assert cfg.freeze_conv is True and cfg.pool5_store_gb == 0.5
    for ok in (("--freeze_conv", "True"), ("--freeze_conv", "True", "--pool5_store_gb", "0.5"),
               ("--freeze_conv", "True", "--pool5_store_gb", "0.5", "--photo_store_gb", "1"),
               ("--freeze_conv", "True", "--photo_store_gb", "1"),
               ("--freeze_conv", "True", "--review_net_only", "True"),
               ("--freeze_conv", "True", "--train_embedding", "True", "--sparse_embedding", "True", "--grad_clip", "5.0"),
               ("--freeze_vgg", "True", "--feature_store_gb", "1")):
        main.check_flags(main_config(*ok))
    refused = {("--freeze_conv", "1"): "--freeze_conv takes True or False",
               ("--freeze_conv", "True", "--freeze_vgg", "True"): "--freeze_conv True and --freeze_vgg True exclude each other",
               ("--freeze_conv", "True", "--pool5_store_gb", "-1"): "--pool5_store_gb must be >= 0",
               ("--pool5_store_gb", "1"): "--pool5_store_gb needs --freeze_conv True",
               ("--pool5_store_gb", "1", "--photo_store_gb", "1"): "--pool5_store_gb needs --freeze_conv True",
               ("--freeze_vgg", "True", "--pool5_store_gb", "1"): "--pool5_store_gb needs --freeze_conv True",
               ("--freeze_conv", "True", "--pool5_store_gb", "1", "--feature_store_gb", "1"):
                   "--pool5_store_gb and --feature_store_gb exclude each other",
               ("--freeze_vgg", "True", "--pool5_store_gb", "1", "--feature_store_gb", "1"):
                   "--pool5_store_gb and --feature_store_gb exclude each other"}
    for argv, text in refused.items():
        with pytest.raises(SystemExit, match=text):
            main.check_flags(main_config(*argv))


# ---- the model on the CPU -------------------------------------------------------------------------------------------------------
def _umpr(**kw):
    """On the meta device: names, shapes and requires_grad are what these tests read, and an optimiser for 124 M parameters
    then costs no memory."""
    from umpr_amd.model import UMPR
    return UMPR(_cfg(review_net_only=False, views=["food", "inside"], **kw), EMB).to("meta")


@pytest.fixture(scope="module")
def conv_frozen():
    return _umpr(freeze_conv=True)


@pytest.fixture(scope="module")
def plain():
    return _umpr()


def test_which_parameters_train(conv_frozen, plain):
    from umpr_amd.model import UMPR
    vgg = conv_frozen.visual_net.vgg16[0]
    assert conv_frozen.freeze_conv and not conv_frozen.freeze_vgg and vgg.frozen_conv and not vgg.frozen
    assert plain.freeze_conv is False and plain.visual_net.vgg16[0].frozen_conv is False
    named = dict(conv_frozen.named_parameters())
    off = sorted(k for k, p in named.items() if not p.requires_grad and k != "embedding.weight")
    assert len(off) == 26 and all(k.startswith(PRE + "features.") for k in off)
    on = [k for k, p in named.items() if p.requires_grad]
    assert len([k for k in on if k.startswith(PRE + "classifier.")]) == 6 and len(on) == 37 + 6
    have = {k: tuple(v.shape) for k, v in conv_frozen.state_dict().items()}
    assert have == {k: tuple(v.shape) for k, v in plain.state_dict().items()}
    assert list(conv_frozen.state_dict()) == list(plain.state_dict())
    with pytest.raises(ValueError, match="freeze_vgg and freeze_conv"):
        UMPR(_cfg(review_net_only=False, views=["food"], freeze_conv=True, freeze_vgg=True), EMB)
    r = UMPR(_cfg(review_net_only=True, freeze_conv=True, freeze_vgg=True), EMB)       # nothing to freeze in UMPR-R
    assert r.freeze_conv is False and r.freeze_vgg is False


def test_fused_adam_on_a_frozen_conv_base(conv_frozen):
    from umpr_amd.optim import FusedAdam, _pad
    from umpr_amd.parallel import GradReducer
    opt = FusedAdam(conv_frozen, 1e-3, 1e-3)
    names = [n for g in opt.groups for n in g.names]
    assert names and not any(".features." in n for n in names)
    trainable = {n: p for n, p in conv_frozen.named_parameters() if p.requires_grad}
    assert set(names) == set(trainable)
    eb = opt.early_bucket()
    assert eb is not None and len(eb[3]) == 3 and eb[1] == 0                   # the three classifier weights, at the arena's front
    for g in opt.groups:
        assert g.numel == sum(_pad(trainable[n].numel()) for n in g.names) == g.g.numel()
    assert sum(g.numel for g in opt.groups) < 124_000_000                      # 123.6 M of classifier, no 14.7 M of conv weights
    assert conv_frozen.visual_net.vgg16[0].grad_callbacks != []               # the early classifier update stays wired
    opt.arm_early(1.0)
    assert opt._early is not None
    opt.disarm()
    clipped = FusedAdam(conv_frozen, 1e-3, 1e-3, max_grad_norm=1.0)           # while clipping is on the early update stays off
    clipped.arm_early(1.0)
    assert clipped._early is None
    red = GradReducer(clipped)
    assert red._find_block_slices() == {} and red.block_slices == {}          # no conv weights in the arena: no block bucket
    red.close()


def test_optimizer_state_of_the_other_setting_is_refused(conv_frozen, plain):
    from umpr_amd.optim import FusedAdam
    of, op = FusedAdam(conv_frozen, 1e-3, 1e-3), FusedAdam(plain, 1e-3, 1e-3)
    # what check_state_dict reads of a state: the moments' names and sizes (FusedAdam.state_dict copies them to the host, which a
    # meta arena cannot do)
    state = lambda o: {k: {n: torch.empty(z, device="meta") for n, z in o._moment_sizes().items()} for k in ("m", "v")}   # noqa: E731
    st_frozen, st_plain = state(of), state(op)
    assert len(st_plain["m"]) == len(st_frozen["m"]) + 26
    with pytest.raises(ValueError, match="written with the VGG conv base trainable, this run has it frozen: pass the same --freeze_conv"):
        of.check_state_dict(st_plain)
    with pytest.raises(ValueError, match="written with the VGG conv base frozen, this run has it trainable: pass the same --freeze_conv"):
        op.check_state_dict(st_frozen)
    of.check_state_dict(st_frozen)
    op.check_state_dict(st_plain)


# ---- the store's host half ------------------------------------------------------------------------------------------------------
def test_conv_fingerprint_follows_the_conv_parameters_only():
    from umpr_amd.photos import conv_fingerprint, vgg_fingerprint

    class Tiny(torch.nn.Module):
        def __init__(self):
            super().__init__()
            self.features = torch.nn.Sequential(torch.nn.Conv2d(3, 4, 3), torch.nn.ReLU())
            self.classifier = torch.nn.Sequential(torch.nn.Linear(4, 3))
            self.compute_dtype = "fp32"

    m = Tiny()
    m.features.requires_grad_(False)
    f0, v0 = conv_fingerprint(m), vgg_fingerprint(m)
    assert conv_fingerprint(m) == f0
    with torch.no_grad():
        m.get_parameter("classifier.0.weight").add_(1.0)                       # what an Adam step on the classifier does
    assert conv_fingerprint(m) == f0 and vgg_fingerprint(m) != v0
    with torch.no_grad():
        m.get_parameter("features.0.weight").add_(1.0)
    f1 = conv_fingerprint(m)
    assert f1 != f0
    m.load_state_dict(m.state_dict())                                          # the same values again: still a reload
    f2 = conv_fingerprint(m)
    assert f2 != f1
    m.to(torch.float64)
    f3 = conv_fingerprint(m)
    assert f3 != f2
    m.compute_dtype = "bf16"
    assert conv_fingerprint(m) != f3


def test_pool5_store_needs_a_gpu_and_keeps_the_feature_store_as_it_is():
    from umpr_amd.photos import FeatureStore, Pool5Store
    with pytest.raises(RuntimeError, match="Pool5Store lives on an MI355X \\(no CPU path\\)"):
        Pool5Store("cpu")
    with pytest.raises(RuntimeError, match="FeatureStore lives on an MI355X \\(no CPU path\\)"):
        FeatureStore("cpu")
    assert Pool5Store.F == 25088 and FeatureStore.F == 1000 and issubclass(Pool5Store, FeatureStore)
    assert Pool5Store._registry is not FeatureStore._registry                  # a key space of its own
