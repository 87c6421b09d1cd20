"""tests/classifier_reference.py on the CPU, at reduced widths (200 -> 64 -> 64 -> 40: N = 40 is no multiple of 32 here either): the
hand-written float64 forward and backward against float64 autograd through Linear-ReLU-Dropout-Linear-ReLU-Dropout-Linear, the case
table, the generated-mask replica with the chosen seeds, and the gate against six deliberately wrong backwards.  No GPU."""
import pytest
import torch
import torch.nn.functional as F

import classifier_reference as CR

DIMS = ((200, 64), (64, 64), (64, 40))
HID = DIMS[0][1]


def _close(name, got, want, tol=1e-12):
    d = CR.distances(got, want)
    assert max(d) <= tol, (name, d)


def _autograd(case, params64, masks):
    """float64 autograd of the chain on leaf copies: (fc, drop, out, the six gradients, d_pool5); dropout as mask / (1 - p)"""
    ps = [p.clone().requires_grad_(True) for p in params64]
    x = case.pool5.double().requires_grad_(True)
    fc, drop, h = [], [], x
    for j in range(3):
        h = F.linear(h, ps[2 * j], ps[2 * j + 1])
        if j < 2:
            h = torch.relu(h)
            fc.append(h)
            if masks is not None:
                h = h * masks[j].double() / (1.0 - CR.P_DROP)
                drop.append(h)
    h.backward(case.d_out.double())
    return [t.detach() for t in fc], [t.detach() for t in drop], h.detach(), [p.grad for p in ps], x.grad


def _single_row(case):
    case.d_out[:-1] = 0
    return case


SMALL_CASES = {
    "eval n33": lambda: CR.make_case(33, "eval", "dense", DIMS),
    "masks n33": lambda: CR.make_case(33, "masks", "dense", DIMS),
    "masks n33 ordinary rows": lambda: CR.make_case(33, "masks", "ordinary", DIMS),
    "masks n2": lambda: CR.make_case(2, "masks", "dense", DIMS),
    "masks n5 zero rows": lambda: CR.make_case(5, "masks", "dense", DIMS),        # n >= 3: the last row of pool5 is all zero
    "eval n33 one d_out row": lambda: CR.make_case(33, "eval", "row32", DIMS),
    "masks n7 one d_out row": lambda: _single_row(CR.make_case(7, "masks", "dense", DIMS)),
}


@pytest.mark.parametrize("name", SMALL_CASES)
def test_reference_matches_autograd(name):
    """Forward chain, per-layer forward from autograd's own layer inputs, and the backward fed autograd's fc / drop: every tensor to
    1e-12 of its maximum - eval, injected masks, all-zero and constant pool5 rows, a single nonzero d_out row."""
    case = SMALL_CASES[name]()
    _, p64 = CR.weights(DIMS)
    fc, drop, out, grads, dx = _autograd(case, p64, case.masks)
    fc_r, drop_r, out_r = CR.classifier_forward(case.pool5, p64, case.masks)
    for j in range(2):
        _close(f"fc{j + 1}", fc_r[j], fc[j])
        if case.masks is not None:
            _close(f"drop{j + 1}", drop_r[j], drop[j])
            assert torch.equal(CR.dropout_forward(fc[j], case.masks[j]), drop[j])
    _close("out", out_r, out)
    xs = CR.layer_inputs(case.pool5, fc, drop, case.dropout)
    for j, want in enumerate(fc + [out]):
        _close(CR.FWD_NAMES[j], CR.layer_forward(xs[j], p64[2 * j], p64[2 * j + 1], j < 2), want)
    g, d_pool5 = CR.classifier_backward(case.pool5, fc, drop, p64, case.d_out, case.masks)
    for nm, got, want in zip(CR.GRAD_NAMES, g, grads):
        _close(nm, got, want)
    _close("d_pool5", d_pool5, dx)
    if case.n >= 3 and case.kind != "ordinary":
        z, c = (0, 1) if case.kind == "row32" else (-1, -2)
        assert float(case.pool5[z].abs().max()) == 0 and float(case.pool5[c].min()) == float(case.pool5[c].max()) > 0


def test_bf16_variant_rounds_every_product_operand():
    """On operands that are bf16 values already the bf16 forms equal the plain float64 ones (the rounding is the only difference);
    on general operands they equal autograd through Linear layers that round their operands as _QLinear of test_gpu_bf16.py."""
    case = CR.make_case(17, "masks", "dense", DIMS)
    p32, _ = CR.weights(DIMS)
    q = CR.bf16_round

    class QLinear(torch.autograd.Function):
        @staticmethod
        def forward(ctx, x, w, b):
            ctx.save_for_backward(x, w)
            return (q(x).double() @ q(w).double().t() + b.double()).float()

        @staticmethod
        def backward(ctx, g):
            x, w = ctx.saved_tensors
            gq = q(g).double()
            return (gq @ q(w).double()).float(), (gq.t() @ q(x).double()).float(), g.double().sum(0).float()

    ps = [p.clone().requires_grad_(True) for p in p32]
    x = case.pool5.clone().requires_grad_(True)
    fc, drop, h = [], [], x
    for j in range(3):
        h = QLinear.apply(h, ps[2 * j], ps[2 * j + 1])
        if j < 2:
            h = torch.relu(h)
            fc.append(h.detach())
            h = h * case.masks[j].float() * 2.0
            drop.append(h.detach())
    h.backward(case.d_out)
    xs = CR.layer_inputs(case.pool5, fc, drop, True)
    for j, want in enumerate(fc + [h.detach()]):
        _close(CR.FWD_NAMES[j], CR.layer_forward_bf16(xs[j], p32[2 * j], p32[2 * j + 1], j < 2).float(), want.double(), 1e-7)
    g, d_pool5 = CR.classifier_backward_bf16(case.pool5, fc, drop, p32, case.d_out, case.masks)
    for nm, got, p in zip(CR.GRAD_NAMES, g, ps):
        _close(nm, got.float(), p.grad.double(), 2e-7)          # autograd's results are rounded to float32 once
    _close("d_pool5", d_pool5, x.grad.double(), 2e-7)
    exact = [q(p) for p in p32]
    xq = q(case.pool5)
    _close("bf16 form on bf16 operands", CR.layer_forward_bf16(xq, exact[0], exact[1], True),
           CR.layer_forward(xq, exact[0].double(), exact[1].double(), True))


def test_case_table_and_yardstick():
    """The table holds every row count, mode and kind the GPU tests promise.  For every case (at reduced widths - the structure of a
    case does not depend on them): the float32 yardstick's own gate ratio is finite and below 1 (it is the yardstick), and no
    reference tensor is identically zero unless the case says so (kind = zero: every gradient; row32: nothing)."""
    rows = {n for n, _, _ in CR.CASES}
    assert rows >= set(CR.ROWS) and set(CR.ROWS) >= {1, 2, 31, 32, 33, 63, 64, 65, 127, 128, 129, 160}
    assert {n for n, m, _ in CR.CASES if m == "masks"} >= {1, 33, 64, 127, 129}
    assert {(n, m) for n, m, _ in CR.CASES if m.startswith("gen")} == {(n, m) for n in (33, 64) for m in ("gen0", "gen1")}
    assert (33, "eval", "row32") in CR.CASES and (5, "eval", "zero") in CR.CASES and len(set(CR.CASES)) == len(CR.CASES)
    assert any(k == "ordinary" and n % 2 for n, _, k in CR.CASES)      # an odd n whose last pool5 row is not zero
    assert CR.GEN_SEEDS["gen1"] == CR.GEN_SEEDS["gen0"] + 1
    p32, p64 = CR.weights(DIMS)
    for n, mode, kind in CR.CASES:
        case = CR.make_case(n, mode, kind, DIMS)
        masks = CR.generated_masks(case.seed, n, HID) if case.train else case.masks
        fc, drop, out = CR.classifier_forward(case.pool5, p64, masks)
        fc32, drop32, out32 = CR.classifier_forward(case.pool5, p32, masks, torch.float32)
        g64, dx64 = CR.classifier_backward(case.pool5, fc, drop, p64, case.d_out, masks)
        g32, dx32 = CR.classifier_backward(case.pool5, fc, drop, p32, case.d_out, masks, torch.float32)
        names = CR.FWD_NAMES + CR.GRAD_NAMES + ("d_pool5",)
        ref, ref32 = fc + [out] + g64 + [dx64], fc32 + [out32] + g32 + [dx32]
        ok, rs = CR.gate(ref32, ref, ref32, names=names, K=CR.K)
        for r in rs:
            assert r["ratio"] == r["ratio"] and r["ratio"] <= 1.0, (case.tag, r)
        for nm, t in zip(names, ref):
            zero = float(t.abs().max()) == 0
            assert zero == (kind == "zero" and nm not in CR.FWD_NAMES), (case.tag, nm)


def test_generated_mask_replica_and_chosen_seeds():
    """The replica of the counter hash is a pure function of (seed, layer, element index): rows of a larger batch are the smaller
    batch's.  The two chosen seeds meet every condition test_gpu_classifier.py asserts of the generated masks, at both row counts
    it runs (n = 33 and 64, hidden = 4096): checked here, on the CPU, so that the GPU assertion cannot be a draw."""
    s0, s1 = CR.GEN_SEEDS["gen0"], CR.GEN_SEEDS["gen1"]
    m64 = CR.generated_masks(s0, 64)
    assert torch.equal(CR.generated_masks(s0, 33), m64[:, :33]) and not torch.equal(m64[0], m64[1])
    for n in (33, 64):
        a, b = CR.generated_masks(s0, n), CR.generated_masks(s1, n)
        assert a.dtype == torch.uint8 and a.shape == (2, n, 4096)
        assert CR.mask_conditions(a, b) == [] and CR.mask_conditions(b, a) == []
    broken = m64.clone()
    broken[1, 5] = broken[0, 9]
    assert CR.mask_conditions(broken) == ["two rows are equal"]
    assert CR.mask_conditions(torch.ones_like(m64))[0].startswith("layer 0: keep fraction")


# ------------------------------------------------------------------------------------------------------- sensitivity
def _wrong_backward(variant, pool5, fc, drop, params, d_out, masks, stale_drop=None):
    """vgg_decisions.classifier_backward in float64 with ONE defect"""
    cv = lambda t: t.detach().double()           # noqa: E731
    p = CR.P_DROP
    n = pool5.shape[0]
    grads, g = [None] * 6, cv(d_out)
    for j in (2, 1, 0):
        if j < 2:
            if masks is not None:
                mk = masks[0] if variant == "layer-1 mask used for layer 2" else masks[j]
                g = g * cv(mk) / (1.0 if variant == "1/(1-p) missing" else 1.0 - p)
            relu_src = stale_drop[j] if variant == "ReLU mask from the dropout output" else fc[j]
            g = g * (cv(relu_src) > 0)
        xin = cv(pool5) if j == 0 else cv(drop[j - 1]) if masks is not None else cv(fc[j - 1])
        rows = n - 1 if variant == "last odd batch row dropped from dW" else n
        grads[2 * j] = g[:rows].t() @ xin[:rows]
        grads[2 * j + 1] = g[:n - 1].sum(0) if variant == "db summed over n-1 rows" else g.sum(0)
        W = cv(params[2 * j])
        g = g[:, :-8] @ W[:-8] if variant == "last 8 of N columns dropped from dx" else g @ W
    return grads, g


VARIANTS = ("last odd batch row dropped from dW", "last 8 of N columns dropped from dx", "layer-1 mask used for layer 2",
            "1/(1-p) missing", "ReLU mask from the dropout output", "db summed over n-1 rows")


@pytest.mark.parametrize("variant", VARIANTS)
def test_gate_rejects_wrong_variants(variant):
    """Six wrong backwards, each at least 10x outside the gate at K_MAX on at least one tensor (n = 33: an odd batch).  The ReLU
    variant runs in eval mode on a drop region left over from an earlier training forward with other masks - what a backward that
    read the wrong region would see there; the five others run with injected masks."""
    stale = variant == "ReLU mask from the dropout output"
    case = CR.make_case(33, "eval" if stale else "masks", "dense" if stale else "ordinary", DIMS)
    p32, p64 = CR.weights(DIMS)
    fc, drop, _ = CR.classifier_forward(case.pool5, p64, case.masks)
    stale_drop = None
    if stale:
        other = CR.make_case(33, "masks", "dense", DIMS, seed=99).masks
        stale_drop = [CR.dropout_forward(fc[j], other[j]) for j in range(2)]
    g64, dx64 = CR.classifier_backward(case.pool5, fc, drop, p64, case.d_out, case.masks)
    g32, dx32 = CR.classifier_backward(case.pool5, fc, drop, p32, case.d_out, case.masks, torch.float32)
    gw, dxw = _wrong_backward(variant, case.pool5, fc, drop, p64, case.d_out, case.masks, stale_drop)
    names = CR.GRAD_NAMES + ("d_pool5",)
    ok, rows = CR.gate(gw + [dxw], g64 + [dx64], g32 + [dx32], names=names, K=CR.K_MAX)
    factors = {r["name"]: r["over"] for r in rows}
    print(f"{variant}: x K_MAX bound per tensor: " + ", ".join(f"{k}={v:.3g}" for k, v in factors.items()))
    assert not ok and max(factors.values()) >= 10, factors
    right, _ = CR.gate(g64 + [dx64], g64 + [dx64], g32 + [dx32], names=names, K=CR.K)
    assert right
