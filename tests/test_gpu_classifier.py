"""The fp32 VGG16 classifier through the C ABI (umpr_vgg16_classifier_{fwd,bwd}_compact and the full-arena forms: the ten kernels of
fc_small.hip, the dropout kernels, umpr_colsum_rows and, above 128 rows, the generic GEMM) against the float64 references of
tests/classifier_reference.py.

Every layer output is compared with the reference of that layer's own HIP input, read from the arena; every drop region must equal
where(mask, 2 fc, 0) bit for bit; the six gradients and d_pool5 are compared with vgg_decisions.classifier_backward fed the arena's
fc / drop regions and the masks the call used (injected, or read back when generated).  Every tensor is held to K x the distance the
float32 CPU evaluation of the same formulas has from float64 (CR.k_of: 4 unless classifier_reference.py states otherwise, never above
14; floor 2^-22) - five orders of magnitude below what one lost batch row, eight lost columns, a wrong mask or a missing scale moves
(test_classifier_reference.py::test_gate_rejects_wrong_variants).  The row counts are the smallest at which each tile, pair and route
edge of the kernels can go wrong (CR.ROWS).  Every call runs on buffers the test allocates: out, the fc / drop regions, the gradients,
d_pool5 and the workspaces (exactly the queried size) NaN-filled, generated masks pre-filled with 0xFF, each with a guard band behind
it that must come back untouched.  Every distance is logged to classifier.log beside the parity tests' log before it is judged.
"""
import os
from types import SimpleNamespace

import pytest
import torch

import classifier_reference as CR
import vgg_decisions as V
from test_gpu_parity import LOG as PARITY_LOG
from test_gpu_parity import L, dev, poison_lds, st   # noqa: F401  (fixtures: the library, the device, NaN-poisoned LDS)

pytestmark = pytest.mark.gpu

LOG = os.path.join(os.path.dirname(PARITY_LOG), "classifier.log")
GUARD = 4096                      # floats (or bytes x 4 for the masks) behind every buffer a call writes
NAN_BITS = 0x7FC00000             # what torch.full(nan) stores: the guard bands are compared as bit patterns
F_IN, HID, F_OUT = CR.DIMS[0][0], CR.DIMS[0][1], CR.DIMS[2][1]
_DEVW = {}


def log(msg):
    os.makedirs(os.path.dirname(LOG), exist_ok=True)
    with open(LOG, "a") as f:
        f.write(msg + "\n")


_POOL = {}


class _Buf:
    """a NaN-filled float buffer of `numel` with a NaN guard band behind it.  pooled: carved from one device allocation per pool
    name that only ever grows - the workspaces and the full arena are several GB and differ in size from case to case, and a fresh
    device allocation of that size per case costs more than the case itself"""

    def __init__(self, dev, numel, name, pooled=None):
        self.name, self.numel = name, numel
        if pooled is None:
            self.all = torch.full((numel + GUARD,), float("nan"), device=dev)
        else:
            if pooled not in _POOL or _POOL[pooled].numel() < numel + GUARD:
                _POOL.pop(pooled, None)
                _POOL[pooled] = torch.empty(numel + GUARD, device=dev)
            self.all = _POOL[pooled][:numel + GUARD]
            self.all.fill_(float("nan"))
        self.t = self.all[:numel]

    def guard_ok(self):
        return bool((self.all[self.numel:].view(torch.int32) == NAN_BITS).all())

    def untouched(self):
        return bool((self.all.view(torch.int32) == NAN_BITS).all())


def _dev_weights(dev):
    """the six parameters on the device (classifier_reference's one shared copy) and the 32-pointer table (the 26 convolution
    entries point at W1: never read)"""
    if dev not in _DEVW:
        from umpr_amd.model import _ptr_array
        params = CR.device_weights(dev)
        keep, parr = _ptr_array([params[0]] * 26 + params)
        _DEVW[dev] = (params, keep, parr)
    return _DEVW[dev]


@pytest.fixture(scope="module")
def weights(dev):
    """(float32 parameters on the CPU: the yardstick's; float64 on the device: the reference's, released with the module, as are
    the pooled workspaces)"""
    p64 = [p.double() for p in _dev_weights(dev)[0]]
    yield CR.weights32(), p64
    del p64[:]
    _POOL.clear()
    torch.cuda.empty_cache()


def _regions(arena, n, form):
    """(pool5, fc [2], drop [2]) views of a flat arena: the compact layout, or the full activation arena's"""
    if form == "compact":
        offs = [0] + [n * F_IN + j * n * HID for j in range(4)]
    else:
        lay = V.arena_layout(n)
        offs = [lay["pool_off"][4]] + lay["fc_off"] + lay["drop_off"]
    pool5 = arena[offs[0]:offs[0] + n * F_IN].view(n, F_IN)
    r = [arena[o:o + n * HID].view(n, HID) for o in offs[1:]]
    return pool5, r[:2], r[2:]


def _forward(L, dev, case, form="compact"):
    """The forward on fresh buffers.  Returns a namespace: arena / out / ws (_Buf), the mask bytes with their guard, the regions."""
    n = case.n
    params, _, parr = _dev_weights(dev)
    f = SimpleNamespace(form=form)
    if form == "compact":
        nb = L.size("umpr_vgg16_cls_arena_bytes", n)
        assert nb == (n * F_IN + 4 * n * HID) * 4
        entry = "umpr_vgg16_classifier_fwd_compact"
    else:
        nb = L.size("umpr_vgg16_act_bytes", n)
        assert V.arena_layout(n)["pool_off"][4] * 4 == L.size("umpr_vgg16_pool5_offset", n) and V.arena_layout(n)["end"] * 4 <= nb
        entry = "umpr_vgg16_classifier_fwd"
    f.arena = _Buf(dev, nb // 4, "arena", pooled=None if form == "compact" else "full arena")
    f.pool5, f.fc, f.drop = _regions(f.arena.t, n, form)
    f.pool5.copy_(case.pool5.to(dev))
    f.mask_all = torch.full((2 * n * HID + 4 * GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    f.masks = f.mask_all[:2 * n * HID].view(2, n, HID)
    if case.masks is not None:
        f.masks.copy_(case.masks.to(dev))
    f.out = _Buf(dev, n * F_OUT, "out")
    wsb = L.size("umpr_vgg16_fwd_ws_bytes", n)
    assert wsb % 4 == 0
    f.ws = _Buf(dev, wsb // 4, "fwd ws", pooled="ws")
    L.call(entry, parr, n, case.train, case.use_masks, case.seed, f.arena.t, f.masks, f.out.t, f.ws.t, wsb, st())
    torch.cuda.synchronize()
    f.ws_guard_ok = f.ws.guard_ok()
    del f.ws                        # the pooled workspace is the backward's next
    return f


def _backward(L, dev, case, f):
    """The backward on the forward's arena and masks, on fresh gradient buffers; the 26 convolution entries of the gradient table
    point at one NaN buffer that must stay untouched."""
    from umpr_amd.model import _ptr_array
    n = case.n
    params, _, parr = _dev_weights(dev)
    b = SimpleNamespace()
    b.grads = [_Buf(dev, p.numel(), nm) for nm, p in zip(CR.GRAD_NAMES, params)]
    b.unused = _Buf(dev, 64, "convolution gradients")
    b.d_pool5 = _Buf(dev, n * F_IN, "d_pool5")
    wsb = L.size("umpr_vgg16_classifier_bwd_ws_bytes", n)
    assert wsb % 4 == 0
    ws = _Buf(dev, wsb // 4, "bwd ws", pooled="ws")
    keep, garr = _ptr_array([b.unused.t] * 26 + [g.t for g in b.grads])
    entry = "umpr_vgg16_classifier_bwd_compact" if f.form == "compact" else "umpr_vgg16_classifier_bwd"
    d_out = case.d_out.to(dev)
    L.call(entry, parr, n, int(case.dropout), f.arena.t, f.masks, d_out, garr, b.d_pool5.t, ws.t, wsb, st())
    torch.cuda.synchronize()
    b.ws_guard_ok = ws.guard_ok()
    return b


def _judge(tag, rows):
    bad = [(r["name"], r["d_max"], r["r_max"], r["ratio"]) for r in rows if not r["ok"]]
    assert not bad, (tag, bad)


def _gate(tag, name, got, ref, ref32):
    """one tensor through the gate, on the device the float64 reference lives on (the float32 CPU yardstick is uploaded)"""
    return CR.gate([got.detach().reshape(ref.shape)], [ref], [ref32.to(ref.device)], names=[name], K=CR.k_of(name), log=log, tag=tag)[1]


@pytest.mark.parametrize("spec", CR.CASES, ids=CR.case_id)
def test_classifier_case(L, dev, weights, spec):
    """One row of the case table: forward per layer, dropout bit for bit, the six gradients and d_pool5, guard bands, no NaN where a
    call must have written, NaN still where it must not (the drop regions in eval, the convolution entries of the gradient table).
    Generated masks: bytes 0 / 1, the replica's bytes, every statistical condition, the same bytes from a second call."""
    case = CR.make_case(*spec)
    n, tag = case.n, case.tag
    p32, p64 = weights
    f = _forward(L, dev, case)
    fails, rows = [], []
    # ---- what the forward wrote
    for buf, ok in ((f.arena, f.arena.guard_ok()), (f.out, f.out.guard_ok())):
        if not ok:
            fails.append(f"guard band of {buf.name} written")
    if not f.ws_guard_ok:
        fails.append("guard band of the forward workspace written")
    if not bool((f.mask_all[2 * n * HID:] == 0xFF).all()):
        fails.append("guard band of the masks written")
    if not torch.equal(f.pool5.cpu(), case.pool5):
        fails.append("pool5 changed")
    written = [("out", f.out.t)] + [(f"fc{j + 1}", f.fc[j]) for j in range(2)]
    if case.dropout:
        written += [(f"drop{j + 1}", f.drop[j]) for j in range(2)]
    else:
        for j in range(2):
            if not bool((f.drop[j].view(torch.int32) == NAN_BITS).all()):
                fails.append(f"drop{j + 1} written in eval")
    nan = [nm for nm, t in written if bool(torch.isnan(t).any())]
    if nan:
        fails.append(f"NaN left in {nan}")
    # ---- masks
    if case.use_masks:
        masks = case.masks
        if not torch.equal(f.masks.cpu(), masks):
            fails.append("injected mask bytes changed")
    elif case.train:
        masks = f.masks.cpu()
        other = CR.generated_masks(CR.GEN_SEEDS["gen1" if case.mode == "gen0" else "gen0"], n)
        fails += CR.mask_conditions(masks, other)
        if not torch.equal(masks, CR.generated_masks(case.seed, n)):
            fails.append("generated masks are not the counter hash of (seed, layer, element index)")
        again = _forward(L, dev, case)
        if not (torch.equal(again.masks, f.masks) and torch.equal(again.out.t.view(torch.int32), f.out.t.view(torch.int32))):
            fails.append("a second call with the same seed gave other masks or another output")
        del again
    else:
        masks = None
        if not bool((f.mask_all == 0xFF).all()):
            fails.append("mask bytes written in eval")
    # ---- dropout output bit for bit
    if case.dropout and not nan and bool((f.masks <= 1).all()):
        for j in range(2):
            want = CR.dropout_forward(f.fc[j], f.masks[j])
            if not torch.equal(want.view(torch.int32), f.drop[j].view(torch.int32)):
                fails.append(f"drop{j + 1} is not where(mask, 2 fc{j + 1}, 0) bit for bit")
    # ---- forward, layer by layer from the layer's own HIP input: float64 on the device, float32 on the CPU
    fc, drop = [t.cpu() for t in f.fc], [t.cpu() for t in f.drop]
    xs_dev = CR.layer_inputs(f.pool5, f.fc, f.drop, case.dropout)
    xs = CR.layer_inputs(case.pool5, fc, drop, case.dropout)
    for j, got in enumerate(f.fc + [f.out.t.view(n, F_OUT)]):
        if bool(torch.isnan(xs[j]).any()):
            continue                 # already a failure above; nothing to compute a reference from
        ref = CR.layer_forward(xs_dev[j], p64[2 * j], p64[2 * j + 1], j < 2, device=dev)
        ref32 = CR.layer_forward(xs[j], p32[2 * j], p32[2 * j + 1], j < 2, torch.float32)
        rows += _gate(tag, CR.FWD_NAMES[j], got, ref, ref32)
    # ---- backward
    b = _backward(L, dev, case, f)
    for buf in b.grads + [b.d_pool5]:
        if not buf.guard_ok():
            fails.append(f"guard band of {buf.name} written")
        if bool(torch.isnan(buf.t).any()):
            fails.append(f"NaN left in {buf.name}")
    if not b.ws_guard_ok:
        fails.append("guard band of the backward workspace written")
    if not b.unused.untouched():
        fails.append("a convolution entry of the gradient table was written")
    if not nan and (masks is None or bool((masks <= 1).all())):
        g64, dx64 = CR.classifier_backward(f.pool5, f.fc, f.drop, p64, case.d_out, masks, device=dev)
        g32, dx32 = CR.classifier_backward(case.pool5, fc, drop, p32, case.d_out, masks, torch.float32)
        for nm, buf, r, r32 in zip(CR.GRAD_NAMES + ("d_pool5",), b.grads + [b.d_pool5], g64 + [dx64], g32 + [dx32]):
            rows += _gate(tag, nm, buf.t, r, r32)
        dw1_max = float(g64[0].abs().max())
        del g64, g32
        if case.kind in ("row32", "ordinary") and not dw1_max > 0:
            fails.append("the reference dW1 is identically zero: the case does not test what it is there for")
        if case.kind == "row32":
            if not bool((b.d_pool5.t.view(n, F_IN)[:32] == 0).all()):
                fails.append("d_pool5 rows 0..31 are not exactly zero")
        if case.kind == "zero":
            for buf in b.grads + [b.d_pool5]:
                if not bool((buf.t == 0).all()):
                    fails.append(f"{buf.name} is not exactly zero")
    if fails:
        log(f"{tag} FAILURES: {fails}")
    assert not fails, (tag, fails)
    _judge(tag, rows)


@pytest.mark.parametrize("n", [3, 33])
def test_full_arena_form_equals_compact(L, dev, n):
    """umpr_vgg16_classifier_fwd / _bwd on a full NaN-filled activation arena (pool5 at umpr_vgg16_pool5_offset, the fc / drop regions
    where vgg_decisions.arena_layout puts them), injected masks: out, all seven gradients and the fc / drop regions bit-equal to the
    compact form's; nothing else of the arena is written."""
    case = CR.make_case(n, "masks", "dense")
    bits = lambda t: t.contiguous().view(torch.int32)       # noqa: E731
    c = _forward(L, dev, case)
    cb = _backward(L, dev, case, c)
    fu = _forward(L, dev, case, "full")
    fb = _backward(L, dev, case, fu)
    fails = []
    for nm, a, b in [("out", c.out.t, fu.out.t)] + [(f"fc{j + 1}", c.fc[j], fu.fc[j]) for j in range(2)] + \
                    [(f"drop{j + 1}", c.drop[j], fu.drop[j]) for j in range(2)] + \
                    [(x.name, x.t, y.t) for x, y in zip(cb.grads + [cb.d_pool5], fb.grads + [fb.d_pool5])]:
        if bool(torch.isnan(a).any()) or not torch.equal(bits(a), bits(b)):
            fails.append(nm)
    lay = V.arena_layout(n)
    other = fu.arena.all.view(torch.int32) != NAN_BITS
    other[lay["pool_off"][4]:lay["pool_off"][4] + n * F_IN] = False
    other[lay["fc_off"][0]:lay["end"]] = False
    if bool(other.any()):
        fails.append(f"{int(other.sum())} floats of the arena outside pool5 / fc / drop (or its guard band) were written")
    for x in (fu.out, fb.d_pool5, *fb.grads):
        if not x.guard_ok():
            fails.append(f"guard band of {x.name}")
    if not (fu.ws_guard_ok and fb.ws_guard_ok and fb.unused.untouched()):
        fails.append("workspace guard band or convolution gradient entry written")
    log(f"cls full arena n{n}: {'bit-equal to compact' if not fails else fails}")
    assert not fails, fails


def test_refusals_leave_every_buffer_untouched(L, dev):
    """A workspace one byte short of the queried size, n = 0 and a NULL arena are refused by the forward and backward entry points
    (full arena, compact and compact bf16) with the library's error, before anything is launched: every buffer is still all NaN."""
    from umpr_amd._lib import UmprHipError
    from umpr_amd.model import _ptr_array
    n = 2
    params, _, parr = _dev_weights(dev)
    arena = _Buf(dev, L.size("umpr_vgg16_act_bytes", n) // 4, "arena")
    out, d_pool5 = _Buf(dev, n * F_OUT, "out"), _Buf(dev, n * F_IN, "d_pool5")
    grads = [_Buf(dev, p.numel(), nm) for nm, p in zip(CR.GRAD_NAMES, params)]
    masks = torch.full((2, n, HID), 0xFF, dtype=torch.uint8, device=dev)
    d_out = torch.zeros(n, F_OUT, device=dev)
    wsb_f, wsb_b = L.size("umpr_vgg16_fwd_ws_bytes", n), L.size("umpr_vgg16_classifier_bwd_ws_bytes", n)
    ws = _Buf(dev, max(wsb_f, wsb_b) // 4, "ws")
    keep, garr = _ptr_array([grads[0].t] * 26 + [g.t for g in grads])
    for form in ("", "_compact", "_compact_bf16"):
        for nn, short, ar, what in ((n, 1, arena.t, "workspace too small"), (0, 0, arena.t, "bad arguments"),
                                    (n, 0, None, "bad arguments")):
            with pytest.raises(UmprHipError, match=what):
                L.call("umpr_vgg16_classifier_fwd" + form, parr, nn, 1, 1, 0, ar, masks, out.t, ws.t, wsb_f - short, st())
            assert "classifier_fwd" in L.last_error()
            with pytest.raises(UmprHipError, match=what):
                L.call("umpr_vgg16_classifier_bwd" + form, parr, nn, 1, ar, masks, d_out, garr, d_pool5.t, ws.t,
                       wsb_b - short, st())
            assert "classifier_bwd" in L.last_error()
    torch.cuda.synchronize()
    for buf in [arena, out, d_pool5, ws] + grads:
        assert buf.untouched(), buf.name
    assert bool((masks == 0xFF).all())
