"""tests/embed_grad_reference.py on the CPU: the float64 dx and scatter against torch autograd through F.embedding with a trainable
table feeding the oracle's GRU, the helper pinned on a hand-computed example, and the host-side surface of `--train_embedding`
(the option, the model's requires_grad, the new size entry points).  No GPU."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import embed_grad_reference as EG
import gru_reference as G
from oracle import umpr_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = [n + s for s in ("", "_reverse") for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]


@pytest.mark.parametrize("shape", [(5, 4, 3, "rand"), (7, 6, 5, "zeros"), (4, 3, 2, "over"), (3, 5, 1, "tail1")],
                         ids=lambda s: "-".join(map(str, s)))
def test_matches_autograd_through_embedding_and_the_oracle_gru(shape):
    """table.grad of sum(out * dout) with out = improved_rnn(F.embedding(ids, table)) in float64 = scatter(dx(dgx)) with dgx of
    the float64 recurrence: ids repeat (vocab 200, pad id 0 past each length), so rows sum several positions."""
    case = G.make_case(*shape)
    table = case.emb.double().requires_grad_(True)
    P = {"g." + k: w.double() for k, w in zip(NAMES, case.w)}
    out = R.improved_rnn(F.embedding(case.ids, table), case.lengths, P, "g.", aten=False)      # rows in the double un-sort's order
    _, unsorted = R.gru_sort_indices(case.lengths)
    (out * case.dout.double()[unsorted]).sum().backward()                                      # = sum(out_by_input_row * dout)
    ref = G.reference(case)
    dx = EG.dx_reference(ref.dgx.reshape(-1, 6 * G.H).numpy(), case.w[0].numpy(), case.w[4].numpy())
    assert np.abs(dx.reshape(case.N, case.L, -1)[~G.valid(case).numpy()]).max(initial=0.0) == 0.0   # exact zeros past a length
    got = EG.scatter_reference([(case.ids.numpy().reshape(-1), dx)], G.VOCAB, case.E)
    want = table.grad.numpy()
    assert np.abs(want).max() > 0
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max(), np.abs(got - want).max()
    untouched = ~EG.touched_rows([(case.ids.numpy(), dx)], G.VOCAB)
    assert untouched.any() and not got[untouched].any()


def test_helper_is_pinned_on_a_hand_computed_example():
    dgx = np.array([[1.0, 2.0, 0.5, -1.0], [0.0, 1.0, 2.0, 2.0], [3.0, 0.0, 0.0, 1.0]])      # 3H = 2
    wf = np.array([[1.0, 0.0, 2.0], [0.0, 1.0, -1.0]])
    wr = np.array([[2.0, 2.0, 0.0], [1.0, 0.0, 1.0]])
    dx = EG.dx_reference(dgx, wf, wr)
    assert dx.tolist() == [[1.0, 3.0, -1.0], [6.0, 5.0, 1.0], [4.0, 0.0, 7.0]]
    ids = np.array([2, 0, 2])
    d = EG.scatter_reference([(ids[:2], dx[:2]), (ids[2:], dx[2:]), (np.array([9, -1]), np.ones((2, 3)))], 4, 3)
    assert d.tolist() == [[6.0, 5.0, 1.0], [0.0, 0.0, 0.0], [5.0, 3.0, 6.0], [0.0, 0.0, 0.0]]      # ids 9 and -1 are dropped
    assert EG.sorted_positions([ids[:2], ids[2:], np.array([0])]).tolist() == [1, 3, 0, 2]        # stable: position order per id
    assert EG.sorted_positions([]).size == 0
    # the float32 yardstick adds position by position: (1e8 + 1) - 1e8 in float32 loses the 1
    big = np.array([[1e8], [1.0], [-1e8]])
    assert EG.scatter_reference([(np.zeros(3, np.int64), big)], 1, 1, np.float32)[0, 0] == 0.0
    assert EG.scatter_reference([(np.zeros(3, np.int64), big)], 1, 1)[0, 0] == 1.0


def test_id_patterns():
    rng = np.random.default_rng(3)
    assert len(set(EG.make_ids("equal", 300, 1000, rng).tolist())) == 1
    assert len(set(EG.make_ids("distinct", 300, 1000, rng).tolist())) == 300
    z = EG.make_ids("zipf", 2000, 1000, rng)
    counts = np.bincount(z, minlength=1000)
    assert counts[0] > 150 and (counts == 1).sum() > 50
    e = EG.make_ids("ends", 257, 1000, rng)
    assert e[0] == 0 and e[-1] == 999 and (e == 0).sum() >= 2 and (e == 999).sum() >= 2


# ---- the option ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def main_config():
    import main
    from umpr_amd.config import Config
    saved = Config._extra
    Config.extend(main.EXTRA_OPTIONS)
    yield lambda *argv: Config(argv=list(argv))
    Config._extra = saved


def test_train_embedding_flag(main_config):
    import main
    cfg = main_config()
    assert cfg.train_embedding is False
    main.check_flags(cfg)
    cfg = main_config("--train_embedding", "True")
    assert cfg.train_embedding is True
    main.check_flags(cfg)
    main.check_flags(main_config("--train_embedding", "True", "--freeze_vgg", "True", "--feature_store_gb", "0.5"))
    main.check_flags(main_config("--train_embedding", "False", "--review_net_only", "True"))
    for bad in ("1", "0", "'yes'"):
        with pytest.raises(SystemExit, match="--train_embedding takes True or False"):
            main.check_flags(main_config("--train_embedding", bad))


@pytest.mark.parametrize("ronly", [True, False])
def test_model_construction_sets_requires_grad_as_asked(main_config, ronly):
    from umpr_amd.model import UMPR
    emb = np.zeros((30, 6), dtype=np.float32)
    for argv, want in (((), False), (("--train_embedding", "False"), False), (("--train_embedding", "True"), True)):
        cfg = main_config("--review_net_only", str(ronly), *argv)
        m = UMPR(cfg, emb)
        assert m.embedding.weight.requires_grad is want and m.train_embedding is want
        assert ("embedding.weight" in {n for n, p in m.named_parameters() if p.requires_grad}) is want
        assert "embedding.weight" in m.state_dict()
    from umpr_amd.config import Config
    plain = Config(argv=[])                               # a config that has never heard of the option: frozen
    plain.review_net_only = ronly
    assert not hasattr(plain, "train_embedding") or plain.train_embedding is False
    assert UMPR(plain, emb).embedding.weight.requires_grad is False


def test_graphed_step_refuses_a_trainable_table(main_config):
    from umpr_amd.graphs import GraphedTrainStep
    from umpr_amd.model import UMPR
    m = UMPR(main_config("--review_net_only", "True", "--train_embedding", "True"), np.zeros((30, 6), dtype=np.float32))
    with pytest.raises(NotImplementedError, match="trainable embedding table"):
        GraphedTrainStep(m, None, (None,) * 8)


def test_optimizer_refuses_a_checkpoint_of_the_other_setting_before_loading(main_config):
    """FusedAdam.check_state_dict is pure host work on names and sizes: the wording names the option, both ways."""
    from umpr_amd.optim import FusedAdam
    want = {"embedding.weight": 180, "a.weight": 4}
    fake = FusedAdam.__new__(FusedAdam)
    fake.groups = [type("G", (), {"names": list(want), "offsets": {n: (0, k) for n, k in want.items()}})()]
    ok = {k: {n: torch.zeros(v) for n, v in want.items()} for k in ("m", "v")}
    fake.check_state_dict(ok)
    frozen_ck = {k: {"a.weight": torch.zeros(4)} for k in ("m", "v")}
    with pytest.raises(ValueError, match="written with the embedding table frozen, this run has it trainable: pass the same "
                                         "--train_embedding"):
        fake.check_state_dict(frozen_ck)
    fake.groups[0].names = ["a.weight"]
    with pytest.raises(ValueError, match="written with the embedding table trainable, this run has it frozen"):
        fake.check_state_dict(ok)


# ---- the size entry points: pure host arithmetic --------------------------------------------------------------------------------
def test_new_size_entry_points_run_without_a_gpu():
    from umpr_amd._lib import lib
    L = lib()
    chunk = L.fn["umpr_embed_grad_chunk"]()
    assert chunk >= 64 and chunk % 64 == 0
    al = lambda n: (n + 255) // 256 * 256                                     # noqa: E731
    for T in (0, 1, chunk - 1, chunk, chunk + 1, 2 * chunk + 1, 108800, 2 ** 31 - 2000):
        for E in (1, 49, 50, 300):
            want = 0 if T == 0 else al(8 * T) + al(2 * ((T + chunk - 1) // chunk) * E * 4)
            assert L.size("umpr_embed_grad_ws_bytes", T, E) == want, (T, E)
    assert L.size("umpr_embed_grad_ws_bytes", -1, 50) == 0 and L.size("umpr_embed_grad_ws_bytes", 5, 0) == 0


def test_embed_grad_refuses_bad_arguments_without_a_gpu():
    from umpr_amd._lib import lib
    L = lib()
    fn = L.fn["umpr_embed_grad"]
    IDS, DX, POS, OUT, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000        # never dereferenced: every call is refused

    def rc(counts, E=50, vocab=1000, n_src=None, pos=POS, out=OUT, ws=WS, ws_bytes=1 << 30, ids=IDS):
        k = max(len(counts), 1)
        a = (ctypes.c_void_p * k)(*[ids] * len(counts))
        b = (ctypes.c_void_p * k)(*[DX] * len(counts))
        c = (ctypes.c_long * k)(*counts)
        code = fn(ctypes.addressof(a), ctypes.addressof(b), ctypes.addressof(c), len(counts) if n_src is None else n_src, E, vocab,
                  pos, out, ws, ws_bytes, None)
        return code, L.last_error()

    cases = {"5 sources outside": rc([1] * 5), "bad E=0": rc([4], E=0), "vocab=0": rc([4], vocab=0), "d_emb": rc([4], out=None),
             "bad count -1": rc([-1]), "bad count": rc([2 ** 31 - 10]), "sorted_pos is NULL": rc([4], pos=None),
             "workspace too small": rc([4], ws_bytes=8), "null ids": rc([4], ids=None),
             "8-byte aligned": rc([4], ws=WS + 4)}
    for text, (code, err) in cases.items():
        assert code == -1 and text in err, (text, code, err)
