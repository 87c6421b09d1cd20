"""tests/sparse_adam_reference.py on the CPU: the float64 row update against torch.optim.SparseAdam on nn.Embedding(sparse=True), and
the host-side surface of `--sparse_embedding` (the option and its two refusals, the model's construction, FusedAdam's grouping,
the checkpoint refusal, the refusals on more than one rank, the new entry points' argument checks).  No GPU."""
import ctypes

import numpy as np
import pytest
import torch
from torch import nn

import sparse_adam_reference as SA

EMB = np.random.default_rng(0).standard_normal((30, 6)).astype(np.float32)


def test_row_update_matches_torch_sparse_adam_over_three_steps():
    """repeated ids, the pad index 0 with a zero gradient (the model's table has no padding_idx: a padded position names row 0 and
    its token gradient is zero, so row 0 is in the coalesced index set with a zero row), and a third step whose
    id set is disjoint from the second's: parameters and both moments to 1e-12, rows outside each step's set untouched"""
    vocab, E, lr = 12, 5, 1e-2
    g = torch.Generator().manual_seed(1)
    emb = nn.Embedding(vocab, E, sparse=True).double()
    with torch.no_grad():
        emb.weight.copy_(torch.randn(vocab, E, generator=g, dtype=torch.float64))
    opt = torch.optim.SparseAdam([emb.weight], lr=lr, betas=(0.9, 0.999), eps=1e-8)
    p = emb.weight.detach().numpy().copy()
    m, v = np.zeros_like(p), np.zeros_like(p)
    steps = [[3, 3, 0, 7, 3, 0, 11], [7, 0, 2, 2, 7], [1, 5, 5, 9]]
    assert not set(steps[1]) & set(steps[2])
    for t, ids in enumerate(steps, 1):
        ids_t = torch.tensor(ids)
        w = torch.randn(len(ids), E, generator=g, dtype=torch.float64) * (ids_t != 0).unsqueeze(1)
        opt.zero_grad()
        (emb(ids_t) * w).sum().backward()
        grad = emb.weight.grad.coalesce()
        rows = SA.named_rows([np.array(ids)], vocab)
        assert grad.indices()[0].tolist() == rows.tolist()                    # the pad row is in the index set ...
        if 0 in ids:
            assert not grad.values()[0].any()                                 # ... with a zero gradient
        dense = np.zeros((vocab, E))
        np.add.at(dense, np.array(ids), w.numpy())
        before = (p.copy(), m.copy(), v.copy())
        p, m, v = SA.row_update(p, m, v, rows, dense[rows], t, lr)
        opt.step()
        st = opt.state[emb.weight]
        for name, mine, theirs in (("p", p, emb.weight), ("m", m, st["exp_avg"]), ("v", v, st["exp_avg_sq"])):
            assert np.abs(mine - theirs.detach().numpy()).max() <= 1e-12, (t, name)
        out = np.setdiff1d(np.arange(vocab), rows)
        for a, b in zip(before, (p, m, v)):
            assert np.array_equal(a[out], b[out])
    assert np.abs(m[3]).max() > 0 and np.abs(m[4]).max() == 0                 # row 4 was never named: its moments are exactly zero


def test_row_update_grad_scale_and_float32_yardstick():
    rng = np.random.default_rng(2)
    p, m, v = rng.standard_normal((6, 4)), rng.standard_normal((6, 4)), rng.random((6, 4))
    g = rng.standard_normal((2, 4))
    a = SA.row_update(p, m, v, [5, 1], g, 7, 1e-3, grad_scale=0.5)
    b = SA.row_update(p, m, v, [5, 1], 0.5 * g, 7, 1e-3)
    c = SA.row_update(p, m, v, [5, 1], g, 7, 1e-3, grad_scale=0.5, dtype=np.float32)
    for x, y, z in zip(a, b, c):
        assert np.array_equal(x, y) and z.dtype == np.float32 and 0 < np.abs(z - x).max() < 1e-5
    with pytest.raises(AssertionError, match="distinct"):
        SA.row_update(p, m, v, [1, 1], g, 1, 1e-3)
    assert SA.named_rows([np.array([4, -1, 4, 6]), np.array([[0, 9]])], 6).tolist() == [0, 4]


# ---- the option ---------------------------------------------------------------------------------------------------------------
@pytest.fixture
def main_config():
    import main
    from umpr_amd.config import Config
    saved = Config._extra
    Config.extend(main.EXTRA_OPTIONS)
    yield lambda *argv: Config(argv=list(argv))
    Config._extra = saved


def test_sparse_embedding_flag(main_config):
    import main
    cfg = main_config()
    assert cfg.sparse_embedding is False
    main.check_flags(cfg)
    cfg = main_config("--train_embedding", "True", "--sparse_embedding", "True")
    assert cfg.sparse_embedding is True and cfg.train_embedding is True
    main.check_flags(cfg)
    main.check_flags(main_config("--train_embedding", "True", "--sparse_embedding", "False"))
    for bad in ("1", "0", "'yes'"):
        with pytest.raises(SystemExit, match="--sparse_embedding takes True or False"):
            main.check_flags(main_config("--train_embedding", "True", "--sparse_embedding", bad))
    for argv in (("--sparse_embedding", "True"), ("--sparse_embedding", "True", "--train_embedding", "False")):
        with pytest.raises(SystemExit, match="--sparse_embedding needs --train_embedding True"):
            main.check_flags(main_config(*argv))


@pytest.mark.parametrize("ronly", [True, False])
def test_model_construction(main_config, ronly):
    from umpr_amd.model import UMPR
    for argv, want in ((("--train_embedding", "True"), False), (("--train_embedding", "True", "--sparse_embedding", "True"), True),
                       (("--sparse_embedding", "True"), False)):            # (without a trainable table there is nothing to update)
        m = UMPR(main_config("--review_net_only", str(ronly), *argv), EMB)
        assert m.sparse_embedding is want
        assert m.embedding.weight.requires_grad is ("--train_embedding" in argv)
        assert m.sparse_table_grad() is None
        assert getattr(m.embedding.weight, "_umpr_direct", False) is (m.train_embedding and not want)
    from umpr_amd.config import Config
    plain = Config(argv=[])
    plain.review_net_only = ronly
    assert UMPR(plain, EMB).sparse_embedding is False


def _opt(main_config, *argv, **kw):
    from umpr_amd.model import UMPR
    from umpr_amd.optim import FusedAdam
    m = UMPR(main_config("--review_net_only", "True", "--train_embedding", "True", *argv), EMB)
    return m, FusedAdam(m, 1e-3, 1e-3, **kw)


def test_fused_adam_keeps_the_sparse_table_out_of_every_group(main_config):
    m, opt = _opt(main_config, "--sparse_embedding", "True", max_grad_norm=1.0)
    table = m.embedding.weight
    for g in opt.groups:
        assert "embedding.weight" not in g.names and all(p is not table for p in g.params)
    assert table.grad is None and np.array_equal(table.detach().numpy(), EMB)
    name, p, mo, vo = opt.sparse
    assert name == "embedding.weight" and p is table and mo.shape == vo.shape == table.shape and not mo.any() and not vo.any()
    st = opt.state_dict()
    assert st["sparse_embedding"] is True and st["m"]["embedding.weight"].numel() == table.numel()
    opt.check_state_dict(st)
    opt.zero_grad()                                                           # nothing to drop yet: must not fail
    with pytest.raises(RuntimeError, match="cuda"):
        opt.step()
    m2, dense = _opt(main_config)
    assert dense.sparse is None and dense.groups[0].names[0] == "embedding.weight" and "sparse_embedding" not in dense.state_dict()
    # no gradient arena for the table: the weight group is smaller by the table's (padded) share, the bias group the same
    assert dense.groups[0].numel - opt.groups[0].numel == (table.numel() + 63) // 64 * 64 and dense.groups[1].numel == opt.groups[1].numel
    assert [a.numel() for a in opt.grad_arenas()] == [g.numel for g in opt.groups]


def test_checkpoint_of_the_other_sparse_setting_is_refused_before_loading(main_config):
    _, sparse = _opt(main_config, "--sparse_embedding", "True")
    _, dense = _opt(main_config)
    s_st, d_st = sparse.state_dict(), dense.state_dict()
    assert {k: v.numel() for k, v in s_st["m"].items()} == {k: v.numel() for k, v in d_st["m"].items()}     # same names and sizes
    with pytest.raises(ValueError, match="written with --sparse_embedding False.*pass the same --sparse_embedding"):
        sparse.load_state_dict(d_st)
    with pytest.raises(ValueError, match="written with --sparse_embedding True.*pass the same --sparse_embedding"):
        dense.load_state_dict(s_st)
    assert sparse.step_count == 0 and dense.step_count == 0
    sparse.load_state_dict(s_st)
    dense.load_state_dict(d_st)


def test_more_than_one_rank_is_refused(main_config):
    from umpr_amd.parallel import GradReducer
    from umpr_amd.train import train_step
    m, opt = _opt(main_config, "--sparse_embedding", "True")
    with pytest.raises(NotImplementedError, match="--sparse_embedding runs on one rank only"):
        GradReducer(opt)
    with pytest.raises(NotImplementedError, match="--sparse_embedding runs on one rank only"):
        train_step(m, opt, None, world=2)
    with pytest.raises(NotImplementedError, match="--sparse_embedding runs on one rank only"):
        train_step(m, opt, None, world=1, reducer=object())


def test_graphed_step_and_pretraining_keep_their_rules(main_config):
    from umpr_amd.graphs import GraphedTrainStep
    m, opt = _opt(main_config, "--sparse_embedding", "True")
    with pytest.raises(NotImplementedError, match="trainable embedding table"):
        GraphedTrainStep(m, opt, (None,) * 8)


# ---- the entry points' argument checks: pure host work --------------------------------------------------------------------------
def test_size_query_and_refusals_without_a_gpu():
    from umpr_amd._lib import lib
    L = lib()
    chunk = L.fn["umpr_embed_grad_chunk"]()
    for T in (0, 1, chunk, 2 * chunk + 77, 108800):
        for E in (1, 50, 300):
            assert L.size("umpr_embed_grad_rows_ws_bytes", T, E) == L.size("umpr_embed_grad_ws_bytes", T, E)
    IDS, DX, POS, RID, RG, WS = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000, 0x60000     # never dereferenced: every call is refused
    rows = L.fn["umpr_embed_grad_rows"]

    def rc(n=100, E=50, vocab=1000, tables=True, pos=POS, rid=RID, rg=RG, ws=WS, ws_bytes=None):
        iarr, darr, counts = (ctypes.c_void_p * 1)(IDS), (ctypes.c_void_p * 1)(DX), (ctypes.c_long * 1)(n)
        need = L.size("umpr_embed_grad_rows_ws_bytes", n, E)
        return rows(ctypes.addressof(iarr) if tables else None, ctypes.addressof(darr) if tables else None,
                    ctypes.addressof(counts) if tables else None, 1, E, vocab, pos, rid, rg, ws, need if ws_bytes is None else ws_bytes,
                    None)

    assert rc(tables=False) != 0 and "null source table" in L.last_error()
    assert rc(pos=None) != 0 and "sorted_pos" in L.last_error()
    assert rc(rid=None) != 0 and rc(rg=None) != 0 and "row_id / row_grad" in L.last_error()
    assert rc(ws_bytes=L.size("umpr_embed_grad_rows_ws_bytes", 100, 50) - 1) != 0 and "workspace too small" in L.last_error()
    assert rc(ws=None) != 0 and "workspace too small" in L.last_error()
    assert rc(ws=WS + 4) != 0 and "8-byte aligned" in L.last_error()
    assert rc(E=0) != 0 and rc(vocab=0) != 0
    assert rc(n=0, rid=None, rg=None, ws=None, ws_bytes=0) == 0                # T = 0: a successful no-op, no launch
    adam = L.fn["umpr_sparse_adam_rows"]

    def arc(p=0x10000, m=0x20000, v=0x30000, vocab=1000, E=50, rid=RID, rg=RG, T=10, step=1):
        return adam(p, m, v, vocab, E, rid, rg, T, 1e-3, 0.9, 0.999, 1e-8, step, 1.0, None, None)

    for kw in (dict(E=0), dict(vocab=0), dict(step=0), dict(T=-1), dict(p=None), dict(m=None), dict(v=None), dict(rid=None),
               dict(rg=None)):
        assert arc(**kw) != 0 and "sparse_adam_rows" in L.last_error(), kw
    assert arc(T=0, p=None, m=None, v=None, rid=None, rg=None) == 0            # T = 0: a successful no-op
