"""tests/gru_reference.py on the CPU: the float64 recurrence and its hand-written backward against autograd through the
oracle's time loop and through torch.nn.GRU on packed sequences, against the reference's own fixtures, and the gate against
five deliberately wrong variants.  No GPU."""
import numpy as np
import pytest
import torch

import gru_reference as G
from conftest import load_golden
from oracle import umpr_ref as R

H = G.H
_REFS = {}


def _refs(shape):
    """(case, float64 reference, float32 yardstick) of one GPU case, computed once"""
    if shape not in _REFS:
        case = G.make_case(*shape)
        _REFS[shape] = (case, G.reference(case), G.reference(case, torch.float32))
    return _REFS[shape]


def _close(name, got, want, tol=1e-12):
    d = G.distances(got, want)
    assert max(d) <= tol, (name, d)


def _autograd(case, out_fn):
    """out [N][L][128] of out_fn(x, w) in float64 on leaf copies, backward with the case's dout: (out, dx, eight gradients)"""
    x = case.x.double().requires_grad_(True)
    w = [p.double().requires_grad_(True) for p in case.w]
    out = out_fn(x, w)
    out.backward(case.dout.double())
    return out.detach(), x.grad, [p.grad for p in w]


def _check_against(case, ref, out, dx, grads, what):
    _close(f"{what} out", ref.out, out)
    assert float((ref.out - out).abs().max()) <= 1e-12
    for name, g in zip(G.GRADS, grads):
        _close(f"{what} {name}", ref.grads[name], g)
    # dgx is not a leaf of the module: x.grad = dgx_f W_ih_f + dgx_r W_ih_r carries it
    dx_ref = ref.dgx[..., :3 * H] @ case.w[0].double() + ref.dgx[..., 3 * H:] @ case.w[4].double()
    _close(f"{what} dx", dx_ref, dx)


@pytest.mark.parametrize("shape", G.CASES, ids=lambda s: "-".join(map(str, s)))
def test_matches_autograd_through_the_oracle_loop(shape):
    """every kind, lengths of 0 and above L included: oracle.umpr_ref.gru_cell_seq masks with `lengths > t`"""
    case, ref, _ = _refs(shape)

    def oracle(x, w):
        return torch.cat([R.gru_cell_seq(x, case.lengths, *w[:4], reverse=False),
                          R.gru_cell_seq(x, case.lengths, *w[4:], reverse=True)], -1)
    _check_against(case, ref, *_autograd(case, oracle), "oracle")


@pytest.mark.parametrize("shape", [s for s in G.CASES if s[3] not in ("zeros", "over")], ids=lambda s: "-".join(map(str, s)))
def test_matches_nn_gru_on_packed_sequences(shape):
    """torch.nn.GRU(bidirectional=True) in double under pack_padded_sequence / pad_packed_sequence, for every kind the
    packed form accepts (1 <= length <= L)"""
    case, ref, _ = _refs(shape)
    assert int(case.lengths.min()) >= 1 and int(case.lengths.max()) <= case.L
    gru = torch.nn.GRU(case.E, H, batch_first=True, bidirectional=True).double()

    def packed(x, w):
        names = [n + s for s in ("", "_reverse") for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
        pk = torch.nn.utils.rnn.pack_padded_sequence(x, case.lengths, batch_first=True, enforce_sorted=False)
        res, _ = torch.func.functional_call(gru, dict(zip(names, w)), (pk,))
        return torch.nn.utils.rnn.pad_packed_sequence(res, batch_first=True, total_length=case.L)[0]
    _check_against(case, ref, *_autograd(case, packed), "nn.GRU")


def test_gates_are_the_steps_own_values():
    """the records of one case recomputed from out alone: h' = (1 - z) n + z h_prev at every valid position, both directions"""
    case, ref, _ = _refs((33, 9, 50, "tail1"))
    lens = G.clamped(case)
    for d in range(2):
        o = ref.out[..., d * H:(d + 1) * H]
        prev = torch.zeros_like(o)
        if d == 0:
            prev[:, 1:] = o[:, :-1]
        else:
            prev[:, :-1] = o[:, 1:]         # zero at t = len - 1: out is zero past the length
        r, z, n, hn = ref.gates[d].unbind(2)
        m = G.valid(case)
        assert float((((1 - z) * n + z * prev) - o)[m].abs().max()) <= 1e-15
        w_hh, b_hh = case.w[4 * d + 1].double(), case.w[4 * d + 3].double()
        assert float((prev @ w_hh[2 * H:].t() + b_hh[2 * H:] - hn)[m].abs().max()) <= 1e-15
        assert bool((ref.gates[d][~m] == 0).all()) and bool((o[~m] == 0).all())
        assert int(lens.max()) > 1


@pytest.mark.parametrize("tag", ["toy", "true"])
def test_reproduces_the_references_fixtures(tag):
    """out of the reference's own ImprovedRnn (double un-sort included: out[n] = BiGRU(x[unsorted[n]])) at the tolerance
    tests/test_oracle_golden.py holds the oracle to; the backward against the fixture's parameter gradients likewise."""
    g = load_golden("improved_rnn_" + tag)
    names = [n + s for s in ("", "_reverse") for n in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")]
    case = G.case_of(torch.from_numpy(g["x"]), torch.from_numpy(g["lengths"]), [torch.from_numpy(g["param/module." + n]) for n in names])
    assert np.array_equal(G.sorted_order(case).numpy(), g["sorted_indices"])
    unsorted = torch.from_numpy(g["unsorted_indices"]).long()
    out, gates = G.forward64(case)
    np.testing.assert_allclose(out[unsorted].numpy(), g["out"], atol=2e-6, rtol=0)
    # out[n] = rows[unsorted[n]], so the gradient of rows[m] is gout[sorted[m]]
    dout = torch.from_numpy(g["gout"])[torch.from_numpy(g["sorted_indices"]).long()]
    grads, dgx = G.backward64(case, (out, gates), dout)
    for gname, n in zip(G.GRADS, names):
        np.testing.assert_allclose(grads[gname].numpy(), g["grad/module." + n], atol=2e-5, rtol=1e-4)
    Hh = case.w[1].shape[1]
    dx = dgx[..., :3 * Hh] @ case.w[0].double() + dgx[..., 3 * Hh:] @ case.w[4].double()
    np.testing.assert_allclose(dx.numpy(), g["gx"], atol=1e-5, rtol=1e-4)


@pytest.mark.parametrize("shape", G.CASES, ids=lambda s: "-".join(map(str, s)))
def test_float32_yardstick_is_inside_the_starting_gate(shape):
    """On every GPU case the float32 evaluation passes the gate at K = 4 (ratio <= 1 by construction), its distances are of
    float32 rounding size, and no reference tensor is zero except dW_hh where no sequence has a second step."""
    case, ref, ref32 = _refs(shape)
    lines = []
    names = G.GRADS + ("dgx",)
    r64 = [ref.grads[n] for n in G.GRADS] + [ref.dgx]
    r32 = [ref32.grads[n] for n in G.GRADS] + [ref32.dgx]
    ok, rows = G.gate(r32, r64, r32, names=names, K=G.K_START, log=lines.append, tag=case.tag)
    row = G.gate_abs(ref32.out, ref.out, ref32.out, "out", K=G.K_START, log=lines.append, tag=case.tag)
    print("\n".join(lines))
    assert ok and row["ok"] and all(r["ratio"] <= 1 for r in rows + [row])
    assert row["r_max"] <= 2e-6
    for r, t in zip(rows, r64):
        assert max(r["r_max"], r["r_l2"]) <= 5e-6, r
        zero = float(t.abs().max()) == 0
        assert zero == (r["name"].startswith("dw_hh") and G.whh_is_zero(case)), r["name"]
    assert G.whh_is_zero(case) == (shape in ((1, 1, 1, "full"), (32, 4, 5, "ones")))
    assert float(ref.out.abs().max()) <= 1
    m = G.valid(case)
    if bool(m.any()):
        assert float(ref.out[m].abs().min()) > 0
        for q in range(4):
            assert float(ref.gates[:, m][:, :, q].abs().max()) > 0


def _judge(case, ref, ref32, wrong, tag):
    """the gate's verdict on a wrong variant `wrong` (a namespace like ref): (passed, worst distance / bound)"""
    lines = []
    ok, rows = G.gate([wrong.grads[n] for n in G.GRADS], [ref.grads[n] for n in G.GRADS], [ref32.grads[n] for n in G.GRADS],
                      names=G.GRADS, K=G.K, log=lines.append, tag=f"{case.tag} {tag}")
    row = G.gate_abs(wrong.out, ref.out, ref32.out, "out", K=G.K, log=lines.append, tag=f"{case.tag} {tag}")
    worst = max(r["over"] for r in rows + [row])
    print("\n".join(lines) + f"\n{case.tag} {tag}: worst distance / bound = {worst:.1f}x")
    return ok and row["ok"], worst


@pytest.mark.parametrize("variant,shape", [
    ("dout_element_dropped", (33, 9, 50, "tail1")), ("dout_element_dropped", (65, 12, 300, "rand")),
    ("hprev_own_output", (15, 5, 3, "rand")), ("hprev_own_output", (16, 12, 8, "one_long")),
    ("bhn_outside", (1, 1, 1, "full")), ("bhn_outside", (33, 9, 50, "tail1")),
    ("reverse_from_L", (15, 5, 3, "rand")), ("reverse_from_L", (33, 9, 50, "tail1")),
    ("reset_at_length_change", (15, 5, 3, "rand")), ("reset_at_length_change", (33, 9, 50, "tail1"))])
def test_gate_rejects_wrong_variants(variant, shape):
    """Each wrong variant of the reference, evaluated in float64 (no rounding of its own), is outside the gate by a factor
    of at least 10."""
    case, ref, ref32 = _refs(shape)
    if variant == "dout_element_dropped":
        dout = case.dout.clone()
        dout[G.dropped_dout_element(case)] = 0
        wrong = G.reference(case, dout=dout)
    elif variant in G.WRONG_BWD:
        wrong = G.reference(case, wrong_bwd=variant)
    else:
        wrong = G.reference(case, wrong_fwd=variant)
    ok, worst = _judge(case, ref, ref32, wrong, variant)
    assert not ok
    assert worst >= 10, worst
