"""Optimiser of the reference's training loop (main.py:22-26,31-37) on flat HBM arenas.

The reference builds ``torch.optim.Adam`` with two parameter groups - names without 'bias' get coupled L2
(weight_decay = l2_regularization), names with 'bias' get none - and an ``ExponentialLR`` stepped once per epoch.
Here every trainable parameter of a group is re-pointed into ONE contiguous fp32 arena (same for its gradient and the
two Adam moments), so an optimiser step is one dense Adam launch per group, ``zero_grad`` is one memset, and
the data-parallel gradient exchange is a handful of large RCCL all-reduces on the arena instead of one per tensor.

``FusedAdam.step`` is the one step path: gradient source (gradient or accumulation arenas), the clip norm if clipping is on,
the per-group ranges, the sparse rows.  Every dense launch goes through ``FusedAdam._adam``, which picks one of the library's
four entry points - ``umpr_adam_step[_dev][_clip]``, one kernel template in csrc/optim.hip - from graph mode and clipping, or,
for a range with per-module multipliers or under decoupled decay, ``umpr_adam_step_groups`` with the segments ``plan()`` made.
"""
from __future__ import annotations

import contextlib
import ctypes
import math
import os
import weakref
from typing import Any, NamedTuple

import torch

from .streams import wait_for_gradients
from ._lib import lib, stream_ptr


# "1" (default): on; "0": off.
_EARLY_ADAM = os.environ.get("UMPR_EARLY_ADAM", "1")


class WeakCallback:
    """Entry of a module's ``grad_callbacks``: holds its target method weakly, so an optimiser / reducer that has been
    dropped (and its ~2 GB of flat arenas) is not kept alive - or called - by the model it was once bound to."""

    def __init__(self, method):
        self.ref = weakref.WeakMethod(method)

    def __call__(self):
        m = self.ref()
        if m is not None:
            m()

    def targets(self, method):
        m = self.ref()
        return m is not None and m == method


def add_callback(module, method):
    module.grad_callbacks[:] = [cb for cb in module.grad_callbacks if not (isinstance(cb, WeakCallback) and cb.ref() is None)]
    module.grad_callbacks.append(WeakCallback(method))


def remove_callback(module, method):
    module.grad_callbacks[:] = [cb for cb in module.grad_callbacks
                                if not (isinstance(cb, WeakCallback) and (cb.ref() is None or cb.targets(method)))]


def has_callback(module, method):
    return any(isinstance(cb, WeakCallback) and cb.targets(method) for cb in module.grad_callbacks)


def _is_classifier(name):
    return name.startswith("classifier.") or ".classifier." in name


def _parallel_active():
    from . import parallel
    return parallel.active()


_ALIGN = 64      # floats
MAX_SEGMENTS = 16    # of one umpr_adam_step_groups launch (csrc/optim.hip::ADAM_MAX_SEGS)


def _pad(k):
    return (k + _ALIGN - 1) // _ALIGN * _ALIGN


def parse_scales(text, option="scale"):
    """'visual_net.vgg16.=1e-3,embedding.=0.1' -> {'visual_net.vgg16.': 0.001, 'embedding.': 0.1}: what --lr_scale and --wd_scale
    take.  '' is {}.  Raises ValueError on an entry without '=', an empty or repeated prefix, or a multiplier that is no number."""
    out = {}
    for item in (t.strip() for t in str(text).split(",")):
        if not item:
            continue
        prefix, eq, value = item.rpartition("=")
        prefix = prefix.strip()
        if not eq or not prefix:
            raise ValueError(f"--{option}: {item!r} is not <name prefix>=<multiplier>")
        if prefix in out:
            raise ValueError(f"--{option}: the prefix {prefix!r} is given twice")
        try:
            out[prefix] = float(value)
        except ValueError:
            raise ValueError(f"--{option}: the multiplier of the prefix {prefix!r} is no number: {value.strip()!r}") from None
    return out


def match_scale(name, scales):
    """(multiplier, prefix) of the longest prefix in `scales` that `name` starts with, (1.0, None) if there is none"""
    best = None
    for prefix in scales:
        if name.startswith(prefix) and (best is None or len(prefix) > len(best)):
            best = prefix
    return (1.0, None) if best is None else (float(scales[best]), best)


class _Group:
    def __init__(self, named_params, weight_decay, device):
        self.names = [n for n, _ in named_params]
        self.params = [p for _, p in named_params]
        self.weight_decay = weight_decay
        # every parameter starts on a 256-byte boundary of the arenas: the kernels read weights as float4 / whole 128-B lines, and a
        # one-element bias in front of the 411 MB fc1 matrix must not leave it (and every tensor behind it) at an odd offset.  The
        # padding elements are zeros with zero gradients; Adam leaves them at zero, collectives carry them along.
        n = sum(_pad(p.numel()) for p in self.params)
        self.numel = n
        self.p = torch.zeros(n, dtype=torch.float32, device=device)
        self.g = torch.zeros(n, dtype=torch.float32, device=device)
        self.m = torch.zeros(n, dtype=torch.float32, device=device)
        self.v = torch.zeros(n, dtype=torch.float32, device=device)
        off = 0
        self.offsets = {}
        with torch.no_grad():
            for name, p in zip(self.names, self.params):
                k = p.numel()
                self.p[off:off + k].copy_(p.reshape(-1))
                p.data = self.p[off:off + k].view(p.shape)
                p.grad = self.g[off:off + k].view(p.shape)
                self.offsets[name] = (off, k)
                off += _pad(k)
        # parameters whose backward node writes the gradient in place (model.py::_grad_targets): their arena slices need
        # no zero fill; everything else is zeroed as merged ranges
        self.direct = [p for p in self.params if getattr(p, "_umpr_direct", False)]
        self.zero_ranges = []
        for name, p in zip(self.names, self.params):
            if getattr(p, "_umpr_direct", False):
                continue
            lo, k = self.offsets[name]
            if self.zero_ranges and self.zero_ranges[-1][1] == lo:
                self.zero_ranges[-1][1] = lo + _pad(k)          # (the padding behind a parameter belongs to its range)
            else:
                self.zero_ranges.append([lo, lo + _pad(k)])


class _Sparse(NamedTuple):
    """A table updated row-wise: its parameter name, the parameter, dense moments [vocab][E]."""
    name: str
    table: Any
    m: Any
    v: Any


class _Clip(NamedTuple):
    """Device state of the clipping path and the two host tables umpr_grad_norm reads (n_arenas dense arenas in them)."""
    state: Any
    ws: Any
    ws_bytes: int
    ptrs: Any
    counts: Any
    n_arenas: int


class _Accum(NamedTuple):
    """One accumulation arena per group and the host tables of umpr_grad_accumulate over the n_arenas non-empty ones."""
    arenas: list
    acc_ptrs: Any
    grad_ptrs: Any
    counts: Any
    n_arenas: int


class _Ema(NamedTuple):
    """One EMA arena per group and the host tables of umpr_ema_update / umpr_arena_swap over the n_arenas non-empty ones."""
    arenas: list
    ema_ptrs: Any
    param_ptrs: Any
    counts: Any
    n_arenas: int


_GROUP_DEFAULTS = {"lr_scale": {}, "wd_scale": {}, "decoupled_decay": False, "warmup_steps": 0}


class FusedAdam:
    """Adam(betas=(0.9,0.999), eps=1e-8) with the reference's grouping; ``lr_decay`` per ``epoch_end()``.

    ``max_grad_norm`` > 0 clips the gradient by its global 2-norm inside ``step()``, as ``torch.nn.utils.clip_grad_norm_(...,
    max_grad_norm)`` between ``backward()`` and ``step()`` would: the norm is that of the gradient the update uses (after
    ``grad_scale``, before the coupled L2 term), the coefficient is min(1, max_grad_norm / (norm + 1e-6)).  One reduction over the
    gradient arenas (``umpr_grad_norm``: fixed grid, no atomics, bit-reproducible) leaves the coefficient in device memory and the
    Adam kernels read it from there: no host round trip, so it also runs inside a captured graph.  A step whose norm is not finite
    (an inf or NaN anywhere in the gradient) is SKIPPED: parameters and moments stay as they are.  ``step_count`` still advances
    on a skipped step - the bias corrections are computed on the host, which does not wait for the flag.  While clipping is on the
    early update of the classifier slice is off (``arm_early``): the coefficient is not known before every gradient exists.
    0 (the default) is off: the step launches exactly what it launches without this argument.

    A model with ``sparse_embedding`` (``--sparse_embedding True``) keeps its word table OUT of both groups: the table is not
    re-pointed into an arena and has no gradient arena.  This optimiser owns dense moments [vocab][E] for it, and ``step()``
    launches ``umpr_sparse_adam_rows`` behind the dense groups: the rows the step's batch named - ``model._sparse_rows``, written
    by the backward - are updated as ``torch.optim.SparseAdam(lr, betas, eps)`` updates them (no L2, eps added to sqrt(v)), every
    other row keeps each byte of its value and moments.  With clipping the row gradients are one more arena of the norm, and
    the row kernel reads the same coefficient.

    ``accumulate()`` makes one step out of several micro-batches, as ``(loss / k).backward()`` k times before ``step()`` does:
    called behind each backward it folds the gradient arenas into accumulation arenas of the same size (``umpr_grad_accumulate``:
    the first micro-batch overwrites them, the others add, one fp32 add per element in micro-batch order) and counts in
    ``pending``.  The next ``step(grad_scale)`` then reads the accumulation arenas in place of the gradient arenas with the scale
    ``grad_scale / pending`` - the mean over the micro-batches, which the norm of a clipped step sees as well - and sets
    ``pending`` back to 0.  No early classifier update while anything is pending; not with a sparse table (its rows differ per
    micro-batch) and not in graph mode.  An optimiser that never accumulates allocates and launches nothing for it.

    ``ema_decay`` = d in (0.5, 1) keeps an exponential moving average of the trainable parameters beside the step, as
    ``torch.optim.swa_utils.AveragedModel(model, multi_avg_fn=get_ema_multi_avg_fn(d))`` with ``update_parameters`` behind every
    ``optimizer.step()`` does: one more arena per group (allocated by the first ``step()``), and every ``step()`` ends with ONE
    ``umpr_ema_update`` over all groups on the calling stream, behind the last Adam launch and behind the wait for the early
    classifier update.  The first update copies the parameters, every later one is ``ema = fmaf(1 - d, p - ema, ema)`` - the bits
    of ``torch.lerp(ema, p, 1 - d)`` on the CPU.  It counts optimiser steps, so a group of accumulated micro-batches is one
    update; a step that clipping skips still updates (the average moves towards the parameters that stayed) and no device flag
    is read.  ``ema_tensors()`` shows the average per parameter name, ``swapped_ema()`` puts it under the model for an
    evaluation, ``state_dict()`` carries it as "ema" / "ema_decay".  Not with a sparse table (it lives outside the arenas, and
    averaging it would touch every row each step) and not in graph mode (the first update is another kernel than the captured
    one).  Data parallel needs nothing: every rank holds the same parameters and computes the same bits - built, not run on
    more than one rank.  0 (the default) is off: nothing is allocated, launched or stored for it.

    ``lr_scales`` / ``wd_scales`` map parameter-name prefixes to multipliers of the learning rate / of the decay; the longest
    prefix a name starts with wins, a name no prefix matches keeps 1.  ``decoupled_decay`` takes the decay out of the gradient
    and shrinks the parameter instead, as ``torch.optim.AdamW`` does; ``warmup_steps`` = N > 0 ramps the learning rate linearly
    over the first N optimiser steps.  For a parameter with multipliers (a, w), at optimiser step t (1-based, the one the bias
    corrections use):  lr_t = lr * min(1, t / N) * a;  coupled (default): g' = grad_scale * clip_coef * g + (wd * w) * p, then Adam
    with lr_t - today's update with a and w applied;  decoupled: p <- p * (1 - lr_t * wd * w), then Adam with lr_t on
    grad_scale * clip_coef * g alone.  Bias parameters keep wd = 0 in both modes (a ``wd_scales`` entry has no effect on them),
    the clip norm is that of the gradient before any decay term, and a step that clipping skips touches nothing, the shrink
    included.  A sparse table takes lr_t with the a of its own name and has no decay, as before.  One launch still covers a whole
    group: ``umpr_adam_step_groups`` carries up to 16 segments of (end, a, w) in its kernel arguments, ``plan()`` merges
    neighbours with equal multipliers into one segment and cuts a range with more segments into several launches.  A range
    whose multipliers are all 1 under coupled decay goes to the entry points it went to before, with the arguments it had:
    the warm-up changes scalars only.  ``param_multipliers()`` shows (a, w) per name; ``state_dict()`` carries the four settings
    as "param_groups" when any of them is set, and a checkpoint written under other settings is refused.  Graph mode works
    unchanged: the multipliers are static kernel arguments and the warm-up rides in the hyper rows, whose fourth float is
    lr_t(a = 1) * wd in decoupled mode.  Data parallel needs nothing: every rank computes the same scalars - built, not run on
    more than one rank.  With all four at their defaults nothing is planned, launched or stored for them."""

    sparse = None      # _Sparse: a table updated row-wise (a model with sparse_embedding)
    _hyper = None       # device float32 [groups][4] of enable_graph_mode: the per-step scalars of the device-scalar kernels
    ema_decay = 0.0     # the moving average of the parameters is off
    ema_ready = False   # True from the first update of the average on
    _ema = None         # _Ema, made by the first step() with ema_decay > 0
    _swapped = False    # inside swapped_ema(): the parameters hold the average, the EMA arenas the raw weights
    lr_scales = {}      # per-module multipliers, decoupled decay and warm-up are off (__init__ binds dicts of its own)
    wd_scales = {}
    decoupled_decay = False
    warmup_steps = 0

    def __init__(self, model, lr, l2_regularization, lr_decay=1.0, betas=(0.9, 0.999), eps=1e-8, order_key=None,
                 max_grad_norm=0.0, ema_decay=0.0, lr_scales=None, wd_scales=None, decoupled_decay=False, warmup_steps=0):
        if not isinstance(decoupled_decay, bool):
            raise ValueError(f"decoupled_decay must be True or False, got {decoupled_decay!r}")
        if isinstance(warmup_steps, bool) or not isinstance(warmup_steps, int) or warmup_steps < 0:
            raise ValueError(f"warmup_steps must be a whole number >= 0 (0 turns the warm-up off), got {warmup_steps!r}")
        self.lr_scales = {str(k): float(v) for k, v in (lr_scales or {}).items()}
        self.wd_scales = {str(k): float(v) for k, v in (wd_scales or {}).items()}
        self.decoupled_decay = decoupled_decay
        self.warmup_steps = warmup_steps
        for prefix, a in self.lr_scales.items():
            if not math.isfinite(a) or a <= 0.0:
                raise ValueError(f"lr_scales: the multiplier of the prefix {prefix!r} must be finite and > 0, got {a}")
        for prefix, w in self.wd_scales.items():
            if not math.isfinite(w) or w < 0.0:
                raise ValueError(f"wd_scales: the multiplier of the prefix {prefix!r} must be finite and >= 0, got {w}")
        max_grad_norm = float(max_grad_norm)
        if not math.isfinite(max_grad_norm) or max_grad_norm < 0.0:
            raise ValueError(f"max_grad_norm must be finite and >= 0 (0 turns clipping off), got {max_grad_norm}")
        self.max_grad_norm = max_grad_norm
        self._clip = None           # _Clip, made by the first clipped step
        self.pending = 0            # micro-batches folded into the accumulation arenas since the last step
        self._acc = None            # _Accum, made by the first accumulate()
        ema_decay = float(ema_decay)
        if ema_decay != 0.0 and not 0.5 < ema_decay < 1.0:
            raise ValueError(f"ema_decay must be 0 (off) or lie in the open interval (0.5, 1), got {ema_decay}")
        if ema_decay > 0.0 and getattr(model, "sparse_embedding", False):
            raise NotImplementedError("FusedAdam(ema_decay=): not with a sparse table (--sparse_embedding True): the table lives "
                                      "outside the arenas, and averaging it would touch every row each step (average with "
                                      "--sparse_embedding False)")
        self.ema_decay = ema_decay
        named = [(n, p) for n, p in model.named_parameters() if p.requires_grad]
        if getattr(model, "sparse_embedding", False):
            table = model.embedding.weight
            (name,) = [n for n, p in named if p is table]
            named = [(n, p) for n, p in named if p is not table]
            self.sparse = _Sparse(name, table, torch.zeros_like(table), torch.zeros_like(table))
        if order_key is None:
            # the VGG classifier's gradients are produced first in backward and are 89 % of all gradient bytes: put them
            # at the front of the arena so that one contiguous slice can be all-reduced while the conv backward runs
            order_key = lambda name: 0 if _is_classifier(name) else 1
        named.sort(key=lambda np_: order_key(np_[0]))  # stable: model order inside each class
        if not named:
            raise ValueError("FusedAdam: the model has no trainable parameter")
        # a prefix nothing starts with is a typing error, not a wish (the sparse table is trainable, and has no decay)
        trainable = [n for n, _ in named] + ([self.sparse.name] if self.sparse is not None else [])
        for prefix in self.lr_scales:
            if not any(n.startswith(prefix) for n in trainable):
                raise ValueError(f"lr_scales: the prefix {prefix!r} matches no trainable parameter")
        for prefix in self.wd_scales:
            if not any(n.startswith(prefix) and 'bias' not in n for n, _ in named):
                raise ValueError(f"wd_scales: the prefix {prefix!r} matches no parameter with weight decay"
                                 + (" (bias parameters and a sparse table have none)"
                                    if any(n.startswith(prefix) for n in trainable) else ""))
        device = named[0][1].device
        self.groups = [_Group([(n, p) for n, p in named if 'bias' not in n], l2_regularization, device),
                       _Group([(n, p) for n, p in named if 'bias' in n], 0.0, device)]
        # nothing scaled, coupled decay: _adam never plans (the warm-up alone changes scalars only)
        self._plain = not (self.lr_scales or self.wd_scales or self.decoupled_decay)
        self._plans = {}            # (group, lo, hi) -> the launches of plan() with their host tables, built on first use
        self.model = model
        self.base_lr = lr
        self.lr = lr
        self.lr_decay = lr_decay
        self.betas = betas
        self.eps = eps
        self.step_count = 0
        # Early update of the VGG classifier slice (89 % of all parameters): its gradients are final as soon as the
        # classifier's backward node has run, long before the convolutional backward ends.  When train_step has armed it,
        # the Adam kernel for that slice runs on a side stream underneath the conv backward (behind the slice's
        # all-reduce when data parallel) instead of after everything: 0.75 of the 0.85 ms the optimiser takes at batch 64
        # leaves the critical path.  Elementwise, so the result is bit-identical to the late update.
        self._early = None          # (grad_scale,) while armed
        self._early_done = None     # (lo, hi, event) once the slice has been updated in this step
        self._early_stream = None
        self.reducer = None         # set by parallel.GradReducer: it then calls early_step after launching its all-reduce
        # one optimiser per model: binding a new one (a resumed run, a second test leg) detaches the old one's callbacks
        prev = getattr(model, "_umpr_optimizer", None)
        prev = prev() if prev is not None else None
        if prev is not None and prev is not self:
            prev.close()
        model._umpr_optimizer = weakref.ref(self)
        # a frozen VGG (UMPR(freeze_vgg=True)) leaves no classifier slice in the arenas: no early update, no callback
        self._has_classifier = self.early_bucket() is not None
        if self._has_classifier:
            for m in model.modules():
                if hasattr(m, "grad_callbacks"):
                    add_callback(m, self._on_classifier_grads)

    def close(self):
        """Detach from the model: remove this optimiser's callbacks (and its reducer's).  The parameters stay views of the
        arenas (they own them from here on); a new FusedAdam on the same model re-points them into its own."""
        if self.reducer is not None:
            self.reducer.close()
        for m in self.model.modules():
            if hasattr(m, "grad_callbacks"):
                remove_callback(m, self._on_classifier_grads)
        self._early = self._early_done = None

    # ---- hipGraph support: the Adam kernel's per-step scalars live in device memory (umpr_adam_step_dev) --------------------
    def enable_graph_mode(self, hyper=None):
        """From now on step() launches the device-scalar form of the kernel; prepare_step() must run before every step (eager or
        replayed) to refresh the scalars for the step about to be taken.  The update is bit-identical to the plain form.
        `hyper`: a device float32 [groups][4] view the CALLER keeps fresh from hyper_rows() (umpr_amd/graphs.py carries the scalars
        inside its one upload per step); prepare_step() is then not used."""
        if self.ema_decay > 0.0:
            raise NotImplementedError("FusedAdam.enable_graph_mode: not with ema_decay > 0: the first update of the average is "
                                      "another kernel than the one a captured step would replay")
        dev = self.groups[0].p.device
        if hyper is not None:
            assert hyper.shape == (len(self.groups), 4) and hyper.dtype == torch.float32 and hyper.device == dev
            self._hyper = hyper
            self._hyper_host = None
            return
        self._hyper = torch.zeros(len(self.groups), 4, device=dev, dtype=torch.float32)
        self._hyper_host = [torch.zeros(len(self.groups), 4, dtype=torch.float32).pin_memory() for _ in range(8)]
        self._hyper_ev = [None] * 8
        self._hyper_k = 0

    def hyper_rows(self, grad_scale=1.0):
        """[grad_scale, lr / (1 - b1^t), 1 / sqrt(1 - b2^t), weight_decay] per group for the step about to be taken (float64 on
        the host, as the plain kernel's launcher computes them).  lr is the warmed-up rate of step t (``lr_at``); with
        ``decoupled_decay`` the fourth float is lr * weight_decay, the fraction an unscaled parameter shrinks by."""
        t = self.step_count + 1
        lr = self.lr_at(t)
        return [[float(grad_scale), float(lr / (1.0 - self.betas[0] ** t)), float(1.0 / (1.0 - self.betas[1] ** t) ** 0.5),
                 float(lr * g.weight_decay if self.decoupled_decay else g.weight_decay)] for g in self.groups]

    # ---- per-module multipliers, decoupled decay, warm-up ------------------------------------------------------------------------
    def lr_at(self, step):
        """the learning rate of optimiser step `step` (1-based) before any multiplier: lr * min(1, step / warmup_steps)"""
        return self.lr if step >= self.warmup_steps else self.lr * (step / self.warmup_steps)

    def param_multipliers(self):
        """{parameter name: (a, w)}: the learning-rate and decay multipliers of every trainable parameter, by longest prefix.
        (w has no effect on a parameter without decay: a bias, a sparse table.)"""
        names = [n for g in self.groups for n in g.names] + ([self.sparse.name] if self.sparse is not None else [])
        return {n: (match_scale(n, self.lr_scales)[0], match_scale(n, self.wd_scales)[0]) for n in names}

    def _spans(self, gi):
        """[(start, stop, a, w)] over group `gi`'s arena: neighbours with equal multipliers merged, the padding behind a
        parameter with the parameter.  A group without decay ignores w."""
        g = self.groups[gi]
        spans = []
        for n in g.names:
            off, k = g.offsets[n]
            a, w = match_scale(n, self.lr_scales)[0], match_scale(n, self.wd_scales)[0] if g.weight_decay != 0.0 else 1.0
            if spans and spans[-1][2:] == (a, w):
                spans[-1] = (spans[-1][0], off + _pad(k), a, w)
            else:
                spans.append((off, off + _pad(k), a, w))
        return spans

    def plan(self, gi, lo, hi):
        """The launches that update elements [lo, hi) of group `gi`: [(lo', hi', [(end, a, w), ...]), ...] with at most 16
        segments each, `end` relative to lo'.  Every end but a launch's last is a multiple of 64: parameters start on 64-float
        boundaries, and a range that does not (no caller has one) gets the floats up to the next boundary as a launch of their
        own.  Pure host arithmetic."""
        spans = self._spans(gi)
        head = min(hi, _pad(lo))
        launches = []
        for l, h in ((lo, head), (head, hi)):
            if h <= l:
                continue
            segs = [(min(stop, h), a, w) for start, stop, a, w in spans if stop > l and start < h]
            for k in range(0, len(segs), MAX_SEGMENTS):
                base = segs[k - 1][0] if k else l
                chunk = segs[k:k + MAX_SEGMENTS]
                launches.append((base, chunk[-1][0], [(end - base, a, w) for end, a, w in chunk]))
        return launches

    def _planned(self, gi, lo, hi):
        """plan(gi, lo, hi) with the three host tables of each launch; None if every multiplier in the range is 1 and the
        decay coupled: the range then goes to the plain entry points"""
        key = (gi, lo, hi)
        if key not in self._plans:
            launches = self.plan(gi, lo, hi)
            if not self.decoupled_decay and all(a == 1.0 and w == 1.0 for _, _, segs in launches for _, a, w in segs):
                self._plans[key] = None
            else:
                self._plans[key] = [(l, h, (ctypes.c_long * len(s))(*[e for e, _, _ in s]),
                                     (ctypes.c_float * len(s))(*[a for _, a, _ in s]),
                                     (ctypes.c_float * len(s))(*[w for _, _, w in s]), len(s)) for l, h, s in launches]
        return self._plans[key]

    def group_summary(self):
        """lines for the log: the multipliers per prefix with parameter counts, and the segments and launches per group"""
        mult = self.param_multipliers()
        lines = []
        for what, scales, col in (("lr_scale", self.lr_scales, 0), ("wd_scale", self.wd_scales, 1)):
            for prefix in scales:
                hit = [n for n in mult if match_scale(n, scales)[1] == prefix]
                lines.append(f"{what} {prefix!r} = {scales[prefix]:g}: {len(hit)} parameters")
        for gi, g in enumerate(self.groups):
            launches = self.plan(gi, 0, g.numel)
            lines.append(f"group {gi} ({'weights' if gi == 0 else 'biases'}, {len(g.names)} parameters): "
                         f"{sum(len(s) for _, _, s in launches)} segments in {len(launches)} launches")
        return lines

    def prepare_step(self, grad_scale=1.0):
        rows = self.hyper_rows(grad_scale)
        assert self._hyper_host is not None, "prepare_step: this optimiser's scalars live in a caller-owned buffer (hyper_rows())"
        k = self._hyper_k % 8
        self._hyper_k += 1
        if self._hyper_ev[k] is not None:
            self._hyper_ev[k].synchronize()
        h = self._hyper_host[k]
        h.copy_(torch.tensor(rows, dtype=torch.float32))
        self._hyper.copy_(h, non_blocking=True)
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self._hyper.device))
        self._hyper_ev[k] = ev

    def zero_grad(self):
        for g in self.groups:
            for lo, hi in g.zero_ranges:
                g.g[lo:hi].zero_()
            for p in g.direct:
                p._umpr_fresh = True
        if self.sparse is not None:
            self.model.drop_sparse_grad()

    def arm_early(self, grad_scale=1.0):
        """train_step: the coming backward belongs to exactly one optimiser step with this gradient scale.
        UMPR_EARLY_ADAM=0 turns it off.  Worth 0.3-0.5 ms per step behind the all-reduce in the RCCL rehearsal (43.16 vs
        43.49 ms fp32, 16.06 vs 16.51 ms bf16); on a single GPU 0.1-0.3 ms in bf16 (9.56 vs 9.71 ms) and nothing in fp32.  Its stream is one more next to main / text / weight-gradient / RCCL:
        umpr_amd/__init__.py sets GPU_MAX_HW_QUEUES, the number of hardware queues they share."""
        self._not_swapped("arm_early")
        if _EARLY_ADAM == "0" or self.max_grad_norm > 0.0:   # clipping: the coefficient needs every gradient first
            return
        if not self._has_classifier:                         # frozen VGG: there is no slice to update early
            return
        if self.pending > 0:                                 # the slice of the last micro-batch is not the group's gradient
            return
        self._early = (float(grad_scale),)
        self._early_done = None

    def disarm(self):
        self._early = None

    def _on_classifier_grads(self):
        # data parallel without a GradReducer (train_step's allreduce_arenas path): the slice is only summed over the ranks
        # AFTER backward, so an update from here would use this rank's local gradient - never early in that case
        if self._early is not None and self.reducer is None and not _parallel_active():
            self.early_step(())

    def early_step(self, handles, stream=None):
        """Adam on the classifier-weight slice, on a side stream; `handles`: the slice's pending async all-reduces;
        `stream`: run it there (the reducer's exchange stream, already ordered behind the slice's in-stream all-reduce)."""
        if self._early is None or self._early_done is not None:
            return
        eb = self.early_bucket()
        if eb is None or self.groups[0].p.device.type != "cuda":
            return
        (scale,) = self._early
        g = self.groups[0]
        _, lo, hi, _ = eb
        dev = g.p.device
        if stream is not None:
            self._early_stream = stream
        if self._early_stream is None:
            # Without a gradient exchange the update rides on the library's weight-gradient stream (Adam is HBM-bound, the
            # weight-gradient kernels behind it MFMA-bound): a sixth stream of its own - main, text, weight-gradient, copy
            # and this one - cost 1.8 ms (bf16) / 3.7 ms (fp32) per step as soon as per-step uploads ran on a copy stream
            # (bench.py --h2d: 11.6 vs 9.79 ms, 45.3 vs 41.4 ms).  Behind an all-reduce it keeps its own stream: the
            # weight-gradient kernels must not queue behind the collective.
            ws = lib().fn["umpr_vgg16_wgrad_stream"]() if not handles else None
            self._early_stream = torch.cuda.ExternalStream(ws, device=dev) if ws else torch.cuda.Stream(dev)
        main = torch.cuda.current_stream(dev)
        self._early_stream.wait_stream(main)            # the gradients were written on the backward's stream
        with torch.cuda.stream(self._early_stream):
            for h in handles:
                h.wait()                                # orders this stream behind the collective, not the host
            self._adam(0, lo, hi, g.g, self.step_count + 1, scale, None)
            ev = torch.cuda.Event()
            ev.record(self._early_stream)
        self._early_done = (lo, hi, ev)

    # ---- clipping by global norm (max_grad_norm > 0) -------------------------------------------------------------------------
    def _clip_buffers(self):
        """The _Clip of the clipping path; the arenas never move, so the two host tables umpr_grad_norm reads are built once.
        (A sparse table's row gradients take one more slot behind them, which _sparse_arena refreshes per step.)"""
        if self._clip is None:
            dev = self.groups[0].p.device
            arenas = self.grad_arenas()
            slots = max(len(arenas) + (self.sparse is not None), 1)
            ptrs = (ctypes.c_void_p * slots)(*[a.data_ptr() for a in arenas])
            counts = (ctypes.c_long * slots)(*[a.numel() for a in arenas])
            state = torch.zeros(8, dtype=torch.float32, device=dev)
            ws_bytes = lib().size("umpr_grad_norm_ws_bytes")
            ws = torch.empty(ws_bytes // 8, dtype=torch.float64, device=dev)
            self._clip = _Clip(state, ws, ws_bytes, ptrs, counts, len(arenas))
        return self._clip

    @property
    def clip_state(self):
        """The 8-float device state umpr_grad_norm maintains (include/umpr_hip.h), or None while clipping is off."""
        return self._clip_buffers().state if self.max_grad_norm > 0.0 else None

    def clip_stats(self):
        """{"norm", "coef", "clipped", "skipped", "seen"}: the last step's gradient norm (scaled, before clipping) and
        coefficient, and how many steps were clipped / skipped / taken with clipping on.  Reads device memory, so it
        SYNCHRONISES: call it where the loop logs, not per step."""
        if self.max_grad_norm <= 0.0:
            raise RuntimeError("clip_stats: clipping is off (FusedAdam(max_grad_norm=0))")
        host = self._clip_buffers().state.cpu()
        cnt = host.view(torch.int32)
        return {"norm": float(host[1]), "coef": float(host[0]), "clipped": int(cnt[5]), "skipped": int(cnt[6]),
                "seen": int(cnt[4])}

    def _grad_norm(self, grad_scale, accumulated):
        """The one umpr_grad_norm call of a clipped step; returns the device state the Adam kernels then read."""
        c = self._clip_buffers()
        if accumulated:                                # the norm of the accumulated gradient: the same counts, the other arenas
            ptrs, n_arenas = self._acc.acc_ptrs, c.n_arenas
        else:
            ptrs, n_arenas = c.ptrs, self._sparse_arena(c.ptrs, c.counts, c.n_arenas)
        # every group carries the same grad_scale: in graph mode the norm kernel reads the first group's from device memory
        lib().call("umpr_grad_norm", ctypes.addressof(ptrs), ctypes.addressof(c.counts), n_arenas, self.max_grad_norm,
                   float(grad_scale), self._hyper[0] if self._hyper is not None else None, c.ws, c.ws_bytes, c.state,
                   stream_ptr())
        return c.state

    # ---- accumulation over micro-batches ---------------------------------------------------------------------------------------
    def _zero_unwritten(self, g):
        for p in g.direct:
            if getattr(p, "_umpr_fresh", False):       # no backward node wrote it since zero_grad: its gradient is zero
                p.grad.zero_()
                p._umpr_fresh = False

    def accumulate(self):
        """Fold the gradient the last backward left in the arenas into the accumulation arenas: the step's first micro-batch
        overwrites them (they are never zeroed, and what a skipped step left in them is never read), every later one adds."""
        if self.sparse is not None:
            raise NotImplementedError("FusedAdam.accumulate: not with a sparse table (--sparse_embedding True): every micro-batch "
                                      "names other rows (accumulate with --sparse_embedding False)")
        if self._hyper is not None:
            raise NotImplementedError("FusedAdam.accumulate: not in graph mode: a captured step is one batch, one update")
        self._not_swapped("accumulate")
        if self.groups[0].p.device.type != "cuda":
            raise RuntimeError("FusedAdam.accumulate launches a HIP kernel: the model must be on a cuda device")
        if self._early_done is not None:
            raise RuntimeError("FusedAdam.accumulate: this backward was armed for an early update (arm_early) and the classifier "
                               "slice has already been stepped with its gradient alone")
        self._early = None
        wait_for_gradients(self.groups[0].p.device)    # in-place gradients written from a side stream (umpr_amd/streams.py)
        for g in self.groups:
            self._zero_unwritten(g)
        if self._acc is None:
            live = [g for g in self.groups if g.numel]
            arenas = [torch.empty_like(g.g) for g in self.groups]
            table = lambda ts: (ctypes.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
            self._acc = _Accum(arenas, table([a for a in arenas if a.numel()]), table([g.g for g in live]),
                               (ctypes.c_long * max(len(live), 1))(*[g.numel for g in live]), len(live))
        a = self._acc
        lib().call("umpr_grad_accumulate", ctypes.addressof(a.acc_ptrs), ctypes.addressof(a.grad_ptrs), ctypes.addressof(a.counts),
                   a.n_arenas, int(self.pending == 0), stream_ptr())
        self.pending += 1

    # ---- the row-wise update of a sparse table ---------------------------------------------------------------------------------
    def _sparse_rows(self):
        """(row_id, row_grad, T) of the step's sparse table gradient, or None: no sparse table, or no backward reached it"""
        rows = self.model._sparse_rows if self.sparse is not None else None
        return None if rows is None or not rows.T else (rows.row_id, rows.row_grad, rows.T)

    def _sparse_arena(self, ptrs, counts, n_arenas):
        """the row gradients as one more arena of umpr_grad_norm: the first T rows of the buffer - the pointer is refreshed here,
        so a buffer that grew (and moved) is followed - or nothing in a step whose backward did not reach the table"""
        rows = self._sparse_rows()
        if rows is None:
            return n_arenas
        _, row_grad, T = rows
        ptrs[n_arenas] = row_grad.data_ptr()
        counts[n_arenas] = T * row_grad.shape[1]
        return n_arenas + 1

    def _step_sparse(self, grad_scale, clip_state):
        rows = self._sparse_rows()
        if rows is None:
            return
        row_id, row_grad, T = rows
        p, m, v = self.sparse.table, self.sparse.m, self.sparse.v
        lr = self.lr_at(self.step_count)               # warmed up, times the multiplier of the table's own name: host scalars
        if self.lr_scales:
            lr = lr * match_scale(self.sparse.name, self.lr_scales)[0]
        lib().call("umpr_sparse_adam_rows", p, m, v, p.shape[0], p.shape[1], row_id, row_grad, T, lr, self.betas[0],
                   self.betas[1], self.eps, self.step_count, float(grad_scale), clip_state, stream_ptr())

    def _adam(self, gi, lo, hi, grads, step, grad_scale, clip_state):
        """The one dense Adam launch: elements [lo, hi) of group `gi` from the arena `grads`, as step number `step`.  Graph mode
        takes the per-step scalars from device memory (`step` and `grad_scale` are then in ``_hyper``), `clip_state` the clip
        coefficient: the same kernel with two switches (csrc/optim.hip).  A range with a multiplier other than 1, or any range
        under decoupled decay, goes through ``plan()`` to ``umpr_adam_step_groups`` - the kernel's other two switches - in as
        many launches as the plan has; every other range is launched as it always was, with the warmed-up learning rate."""
        if hi <= lo:
            return
        g = self.groups[gi]
        lr = self.lr_at(step)
        planned = None if self._plain else self._planned(gi, lo, hi)
        if planned is not None:
            hyper = self._hyper[gi] if self._hyper is not None else None
            for l, h, ends, lr_mult, wd_mult, n_segs in planned:
                lib().call("umpr_adam_step_groups", g.p[l:h], grads[l:h], g.m[l:h], g.v[l:h], h - l, lr, self.betas[0],
                           self.betas[1], self.eps, g.weight_decay, step, grad_scale, hyper, clip_state, ctypes.addressof(ends),
                           ctypes.addressof(lr_mult), ctypes.addressof(wd_mult), n_segs, int(self.decoupled_decay), stream_ptr())
            return
        arenas = (g.p[lo:hi], grads[lo:hi], g.m[lo:hi], g.v[lo:hi], hi - lo)
        tail = (stream_ptr(),) if clip_state is None else (clip_state, stream_ptr())
        if self._hyper is not None:
            lib().call("umpr_adam_step_dev" if clip_state is None else "umpr_adam_step_dev_clip", *arenas, self.betas[0],
                       self.betas[1], self.eps, self._hyper[gi], *tail)
        else:
            lib().call("umpr_adam_step" if clip_state is None else "umpr_adam_step_clip", *arenas, lr, self.betas[0],
                       self.betas[1], self.eps, g.weight_decay, step, grad_scale, *tail)

    def step(self, grad_scale=1.0):
        if self.groups[0].p.device.type != "cuda":
            raise RuntimeError("FusedAdam.step launches a HIP kernel: the model must be on a cuda device")
        self._not_swapped("step")
        self.step_count += 1
        accumulated = self.pending > 0
        if accumulated:
            # the step of a group of micro-batches: accumulate() has waited for and folded each of them, the last one included;
            # the kernels below read the accumulation arenas, and the mean over the group rides on the gradient scale
            grads, grad_scale, self.pending = self._acc.arenas, grad_scale / self.pending, 0
        else:
            wait_for_gradients(self.groups[0].p.device)    # in-place gradients written from a side stream (umpr_amd/streams.py)
            grads = [g.g for g in self.groups]
            for g in self.groups:                      # the norm reads every arena: all stale slices are zeroed before it
                self._zero_unwritten(g)
        done, self._early_done, self._early = self._early_done, None, None
        assert not (accumulated and done is not None)  # accumulate() refuses a backward that was stepped early
        clip_state = None
        if self.max_grad_norm > 0.0:
            assert done is None                        # arm_early never armed
            clip_state = self._grad_norm(grad_scale, accumulated)
        for gi, g in enumerate(self.groups):
            ranges = [(0, g.numel)]
            if gi == 0 and done is not None:           # the classifier slice was updated during backward
                lo, hi, ev = done
                ranges = [(0, lo), (hi, g.numel)]
                torch.cuda.current_stream(g.p.device).wait_event(ev)
            for lo, hi in ranges:
                self._adam(gi, lo, hi, grads[gi], self.step_count, grad_scale, clip_state)
        self._step_sparse(grad_scale, clip_state)
        if self.ema_decay > 0.0:
            self._ema_update()

    # ---- the exponential moving average of the parameters (ema_decay > 0) ------------------------------------------------------
    def _not_swapped(self, what):
        if self._swapped:
            raise RuntimeError(f"FusedAdam.{what}: inside swapped_ema() the parameters hold the averaged weights; leave the "
                               "context first")

    def _ema_buffers(self):
        """The _Ema: one more copy of the trainable parameters.  The arenas never move, so the host tables are built once."""
        if self._ema is None:
            live = [g for g in self.groups if g.numel]
            arenas = [torch.empty_like(g.p) for g in self.groups]
            table = lambda ts: (ctypes.c_void_p * max(len(ts), 1))(*[t.data_ptr() for t in ts])
            self._ema = _Ema(arenas, table([a for a in arenas if a.numel()]), table([g.p for g in live]),
                             (ctypes.c_long * max(len(live), 1))(*[g.numel for g in live]), len(live))
        return self._ema

    def _ema_update(self):
        """behind the step's last launch on the calling stream (which has waited for the early classifier update's event)"""
        e = self._ema_buffers()
        lib().call("umpr_ema_update", ctypes.addressof(e.ema_ptrs), ctypes.addressof(e.param_ptrs), ctypes.addressof(e.counts),
                   e.n_arenas, self.ema_decay, int(not self.ema_ready), stream_ptr())
        self.ema_ready = True

    def ema_bytes(self):
        """what the EMA arenas take (or will take, before the first step): one more copy of the trainable parameters"""
        return 4 * sum(g.numel for g in self.groups) if self.ema_decay > 0.0 else 0

    def ema_tensors(self):
        """{parameter name: view of the EMA arena in the parameter's shape}.  Inside swapped_ema() the views show the raw
        weights."""
        if self.ema_decay <= 0.0:
            raise RuntimeError("ema_tensors: the moving average is off (FusedAdam(ema_decay=0))")
        if not self.ema_ready:
            raise RuntimeError("ema_tensors: no average yet: the first step() makes it")
        out = {}
        for g, arena in zip(self.groups, self._ema.arenas):
            for n, p in zip(g.names, g.params):
                off, k = g.offsets[n]
                out[n] = arena[off:off + k].view(p.shape)
        return out

    def _swap(self):
        e = self._ema
        lib().call("umpr_arena_swap", ctypes.addressof(e.param_ptrs), ctypes.addressof(e.ema_ptrs), ctypes.addressof(e.counts),
                   e.n_arenas, stream_ptr())

    @contextlib.contextmanager
    def swapped_ema(self):
        """Inside the context the model's parameters hold the averaged weights and the EMA arenas the raw ones: one
        umpr_arena_swap launch over all groups on entry and one on exit (also when the body raises), on the calling stream.
        step(), accumulate() and arm_early() raise while it is open.  The exchange is made by a library kernel, so no parameter's
        ``_version`` moves.  That is right: the feature / pool5 stores key on VGG weights that are frozen, hence outside the
        arenas, hence not swapped; nothing else caches a function of a trainable parameter across steps (the Adam kernels do
        not move ``_version`` either)."""
        if self.ema_decay <= 0.0 or not self.ema_ready:
            raise RuntimeError("swapped_ema: no average to swap in: " + ("the moving average is off (FusedAdam(ema_decay=0))"
                                                                         if self.ema_decay <= 0.0 else "the first step() makes it"))
        if self._swapped:
            raise RuntimeError("swapped_ema: already inside swapped_ema()")
        self._swap()
        self._swapped = True
        try:
            yield self
        finally:
            self._swap()
            self._swapped = False

    def epoch_end(self):
        """ExponentialLR.step() (main.py:54)."""
        self.lr *= self.lr_decay

    def state_dict(self):
        """Adam moments per parameter NAME (independent of the arena order), step count and current learning rate."""
        self._not_swapped("state_dict")
        st = {"step": self.step_count, "lr": float(self.lr), "base_lr": float(self.base_lr), "m": {}, "v": {}}
        for g in self.groups:
            for n in g.names:
                off, k = g.offsets[n]
                st["m"][n] = g.m[off:off + k].detach().cpu().clone()
                st["v"][n] = g.v[off:off + k].detach().cpu().clone()
        if self.sparse is not None:
            s = self.sparse
            st["m"][s.name], st["v"][s.name] = s.m.detach().cpu().reshape(-1).clone(), s.v.detach().cpu().reshape(-1).clone()
            st["sparse_embedding"] = True
        if self.ema_decay > 0.0:
            # the average per parameter name, like the moments; empty before the first update
            st["ema"] = {n: t.detach().cpu().reshape(-1).clone() for n, t in self.ema_tensors().items()} if self.ema_ready else {}
            st["ema_decay"] = float(self.ema_decay)
        if self._group_settings() != _GROUP_DEFAULTS:
            st["param_groups"] = self._group_settings()    # (the warm-up has no state of its own: it follows "step")
        return st

    def _group_settings(self):
        return {"lr_scale": dict(self.lr_scales), "wd_scale": dict(self.wd_scales),
                "decoupled_decay": self.decoupled_decay, "warmup_steps": self.warmup_steps}

    def _moment_sizes(self):
        want = {n: g.offsets[n][1] for g in self.groups for n in g.names}
        if self.sparse is not None:
            want[self.sparse.name] = self.sparse.table.numel()
        return want

    def check_state_dict(self, st):
        """Raises unless `st` holds Adam moments for exactly the parameters this optimiser trains, in their sizes - a checkpoint
        written with the VGG (or its conv base, --freeze_conv) frozen resumed with it trainable, or the other way round, does not; nor does one written under the other
        --train_embedding setting.  Nor does one written under the other --sparse_embedding setting: the table's moments have the
        same names and sizes there, but not the same meaning (lazily kept per row, no L2 in them).  Nor does one written with a
        moving average (--ema_decay) for a run without one, or the other way round; another decay value is accepted, and the
        run's own value holds.  Nor does one written under another --lr_scale, --wd_scale, --decoupled_decay or --warmup_steps
        (a checkpoint without "param_groups" was written with all four at their defaults): the moments would continue under
        another update rule."""
        was, now = {**_GROUP_DEFAULTS, **st.get("param_groups", {})}, self._group_settings()
        for option in _GROUP_DEFAULTS:
            if was[option] != now[option]:
                show = lambda x: ",".join(f"{k}={v:g}" for k, v in x.items()) if isinstance(x, dict) else x
                raise ValueError(f"optimizer state does not match this run: the checkpoint was written with --{option} "
                                 f"{show(was[option])!r}, this run has --{option} {show(now[option])!r}: pass the same --{option}")
        was, now = bool(st.get("sparse_embedding", False)), self.sparse is not None
        if was != now:
            raise ValueError("optimizer state does not match this run: the checkpoint was written with --sparse_embedding "
                             f"{was}, this run has --sparse_embedding {now}: pass the same --sparse_embedding")
        was, now = "ema" in st, self.ema_decay > 0.0
        if was != now:
            raise ValueError("optimizer state does not match this run: the checkpoint was written with --ema_decay "
                             f"{float(st.get('ema_decay', 0.0))}, this run has --ema_decay {self.ema_decay}: pass "
                             + (f"--ema_decay {float(st.get('ema_decay', 0.0))} (or another value in (0.5, 1))" if was
                                else "--ema_decay 0"))
        for key in ("m", "v") + (("ema",) if st.get("ema") else ()):
            have = {n: int(t.numel()) for n, t in st[key].items()}
            want = self._moment_sizes()
            if have != want:
                missing, extra = sorted(set(want) - set(have)), sorted(set(have) - set(want))
                sized = sorted(n for n in set(want) & set(have) if want[n] != have[n])
                vgg = [n for n in missing + extra if ".vgg16." in n]
                hint = (" (the checkpoint was written with the VGG " + ("frozen" if any(n in missing for n in vgg) else "trainable")
                        + ", this run has it " + ("trainable" if any(n in missing for n in vgg) else "frozen")
                        + ": pass the same --freeze_vgg)") if vgg else ""
                # only conv moments differ and the classifier's are on both sides: the other --freeze_conv setting
                if vgg and all(".features." in n for n in vgg) and any(".vgg16." in n and ".classifier." in n
                                                                       for n in set(want) & set(have)):
                    hint = (" (the checkpoint was written with the VGG conv base "
                            + ("frozen" if any(n in missing for n in vgg) else "trainable") + ", this run has it "
                            + ("trainable" if any(n in missing for n in vgg) else "frozen") + ": pass the same --freeze_conv)")
                table = [n for n in missing + extra if n == "embedding.weight" or n.endswith(".embedding.weight")]
                if table:
                    hint += (" (the checkpoint was written with the embedding table "
                             + ("frozen" if any(n in missing for n in table) else "trainable") + ", this run has it "
                             + ("trainable" if any(n in missing for n in table) else "frozen") + ": pass the same --train_embedding)")
                raise ValueError(f"optimizer state does not match the trainable parameters{hint}: {len(missing)} parameters "
                                 f"without moments {missing[:3]}, {len(extra)} moments without a trainable parameter {extra[:3]}, "
                                 f"{len(sized)} of another size {sized[:3]}")

    def load_state_dict(self, st):
        self.check_state_dict(st)
        self.step_count = int(st["step"])
        self.lr = float(st["lr"])
        self.base_lr = float(st.get("base_lr", self.base_lr))
        for g in self.groups:
            for n in g.names:
                off, k = g.offsets[n]
                g.m[off:off + k].copy_(st["m"][n])
                g.v[off:off + k].copy_(st["v"][n])
        if self.sparse is not None:
            s = self.sparse
            s.m.copy_(st["m"][s.name].view_as(s.m))
            s.v.copy_(st["v"][s.name].view_as(s.v))
        if self.ema_decay > 0.0:
            self.ema_ready = bool(st["ema"])
            if self.ema_ready:
                for g, arena in zip(self.groups, self._ema_buffers().arenas):
                    arena.zero_()                       # the padding between parameters, as in the parameter arenas
                    for n in g.names:
                        off, k = g.offsets[n]
                        arena[off:off + k].copy_(st["ema"][n])

    def grad_arenas(self):
        return [g.g for g in self.groups if g.numel]

    def accum_arenas(self):
        """The accumulation arenas, one per entry of grad_arenas(), or None before the first accumulate().  After a step they
        still hold the sum that step used."""
        return None if self._acc is None else [a for a in self._acc.arenas if a.numel()]

    def early_bucket(self):
        """(arena, lo, hi, parameters) of the classifier-weight slice of the weight arena, or None.  The slice is
        complete once every one of `parameters` has had its gradient accumulated (one backward node returns all of
        them, and autograd does not promise an order among their AccumulateGrad nodes)."""
        g = self.groups[0]
        names = [n for n in g.names if _is_classifier(n)]
        if not names:
            return None
        lo = min(g.offsets[n][0] for n in names)
        hi = max(g.offsets[n][0] + g.offsets[n][1] for n in names)
        params = [p for n, p in zip(g.names, g.params) if n in set(names)]
        return (g.g, lo, hi, params)
