"""Training / evaluation drivers mirroring main.py:16-61 and src/evaluate.py:6-14."""
from __future__ import annotations

import time

import torch

from . import parallel
from .checkpoint import load_checkpoint, save_checkpoint
from .optim import FusedAdam, parse_scales


def evaluate_mse(model, dataloader):
    """Sum of squared errors over all samples / N (src/evaluate.py:6-14); summed over ranks when distributed.
    The per-batch sums are accumulated ON THE DEVICE by a library kernel (float64 accumulator, `umpr_sq_err_accumulate`)
    and read back once at the end: the reference's `.item()` per batch is a host sync per batch."""
    from ._lib import lib, stream_ptr
    acc = None
    with torch.no_grad():
        model.eval()
        for batch in dataloader:
            if batch[0].shape[0] == 0:   # this rank's chunk of a short last batch is empty (parallel.shard_bounds)
                continue
            pred, _ = model(*batch)
            lab = batch[-1].to(pred.device, non_blocking=True).float().contiguous()
            if acc is None:
                acc = torch.zeros(2, dtype=torch.float64, device=pred.device)
            lib().call("umpr_sq_err_accumulate", pred.contiguous(), lab, pred.numel(), acc, stream_ptr())
    dev = next(model.parameters()).device
    se, cnt = (acc.tolist() if acc is not None else (0.0, 0.0))
    se, cnt = parallel.allreduce_scalars([se, cnt], dev)
    return se / max(cnt, 1)


_ONES = {}


def _one_like(loss):
    key = (loss.device, loss.dtype)
    t = _ONES.get(key)
    if t is None:
        t = _ONES[key] = torch.ones((), device=loss.device, dtype=loss.dtype)
    return t


def train_step(model, opt: FusedAdam, batch, world=1, reducer=None, update=True):
    """model.train(); pred, loss = model(*batch); loss.mean(); zero_grad; backward; step  (main.py:32-37).
    With world > 1 the gradients are summed over ranks (RCCL) - by `reducer` overlapped with backward if given.
    `update=False` makes `batch` a micro-batch of a later step: forward, zero_grad, backward and opt.accumulate(), no step.  The
    call with `update=True` that follows folds its own micro-batch in as well and takes ONE step on the mean gradient of the
    group - `(loss / k).backward()` k times before `step()`; with nothing pending it is the plain step."""
    model.train()
    if (world > 1 or reducer is not None) and getattr(opt, "sparse", None) is not None:
        raise NotImplementedError("train_step: --sparse_embedding runs on one rank only: the table's sparse gradient has no arena "
                                  "to all-reduce (train with --sparse_embedding False on more than one)")
    accumulating = not update or getattr(opt, "pending", 0) > 0
    if accumulating and (world > 1 or reducer is not None):
        raise NotImplementedError("train_step: gradient accumulation (update=False, --accum_steps) runs on one rank only: the "
                                  "accumulated arenas have no exchange")
    n_active = getattr(batch, "n_active", world)     # ranks with a non-empty chunk of this batch (parallel.Shard)
    if batch[0].shape[0] == 0:
        # Fewer samples than ranks in a short last batch: DataParallel would run fewer replicas (main.py:82).  This rank
        # contributes zero gradients but joins every collective, then applies the same averaged update as its peers.
        dev = next(model.parameters()).device
        opt.zero_grad()
        if reducer is not None:
            reducer.skip_backward()
            reducer.finish()
        else:
            for a in opt.grad_arenas():
                a.zero_()
            for g in opt.groups:
                for p in g.direct:
                    p._umpr_fresh = False
            parallel.allreduce_arenas(opt.grad_arenas())
        opt.step(grad_scale=1.0 / n_active)
        return torch.empty(0, device=dev), torch.zeros((), device=dev)
    pred, loss = model(*batch)
    if loss.dim() > 0:               # main.py:34 takes the mean over DataParallel's per-replica losses; one process per
        loss = loss.mean()           # GPU returns a scalar, whose mean is itself (and costs five tiny kernels)
    opt.zero_grad()
    if accumulating:
        # no early update of the classifier slice: the gradient of one micro-batch is not the group's
        loss.backward(gradient=_one_like(loss))
        opt.accumulate()
        if update:
            opt.step(grad_scale=1.0 / n_active)
        return pred, loss
    if world == 1 or reducer is not None:
        # the classifier slice may be updated as soon as its gradients are final: at once on one GPU, behind the reducer's
        # all-reduce of that slice when data parallel.  Without a reducer the exchange only happens after backward
        # (allreduce_arenas below), so the early update stays off (it would use the local gradient).
        opt.arm_early(1.0 / n_active)
    loss.backward(gradient=_one_like(loss))     # a cached device scalar: autograd's implicit ones_like is a fill kernel per step
    if world > 1 or reducer is not None:
        if reducer is not None:
            reducer.finish()
        else:
            parallel.allreduce_arenas(opt.grad_arenas())
    opt.step(grad_scale=1.0 / n_active)
    return pred, loss


def clip_note(opt):
    """'; grad norm ...; clipped a/n, skipped b' for a log line while gradient clipping is on, '' otherwise (the line then
    stays as it was).  Synchronises (FusedAdam.clip_stats)."""
    if opt.max_grad_norm <= 0.0:
        return ""
    st = opt.clip_stats()
    return f"; grad norm {st['norm']:.4f}; clipped {st['clipped']}/{st['seen']}, skipped {st['skipped']}"


def _shuffle_generator(loader):
    """The torch.Generator that orders a (possibly wrapped) DataLoader's epochs, or None."""
    seen = 0
    while loader is not None and seen < 4:
        g = getattr(loader, "generator", None)
        if isinstance(g, torch.Generator):
            return g
        loader = getattr(loader, "loader", None)
        seen += 1
    return None


def _set_epoch(loader, epoch):
    """Tells a (possibly wrapped) loader that draws per epoch which epoch begins: the outermost set_epoch along the `.loader`
    chain (main.ShardedLoader, reviews.StoreLoader).  A loader without one draws nothing per epoch."""
    seen = 0
    while loader is not None and seen < 4:
        f = getattr(loader, "set_epoch", None)
        if callable(f):
            f(epoch)
            return
        loader = getattr(loader, "loader", None)
        seen += 1


def training(train_dataloader, valid_dataloader, model, config, model_path, logger=None, world=1, rank=0):
    """main.py:16-61.  Returns (optimiser, saved): `saved` says whether THIS run wrote `model_path`.
    Not in the reference: `config.resume` continues a run exactly - parameters, Adam moments, learning rate, the
    epoch's shuffle order, the position inside the epoch and the dropout counters all come from the checkpoint, so the
    resumed run visits the batches the uninterrupted run would have visited next.  `config.grad_clip` > 0 clips the gradient to
    that global 2-norm inside the optimiser step (FusedAdam(max_grad_norm=)); the log lines then carry the last norm and the
    clipped / skipped counts.  `config.accum_steps` = k > 1 takes one optimiser step per k consecutive loader batches, on the mean
    of their gradients (train_step(update=False) k - 1 times, then update=True), and one more for the k' < k batches an epoch may
    end with.  `batch_counter` - validation interval, the 50000 limit, the checkpoint - then counts optimiser steps; checkpoints
    are written right behind a step only, with `batch_in_epoch` the loader batches consumed, so a resumed run forms the same
    groups.  Loss sums and log lines stay per loader batch.  `config.ema_decay` = d > 0 keeps an exponential moving average of
    the weights beside the step (FusedAdam(ema_decay=)): every validation behind a step then runs on the averaged weights, inside
    `opt.swapped_ema()`, and says so in its log line, so the checkpoint is chosen by the average's validation MSE.  The
    checkpoint itself is written outside the swap: "model" keeps the raw weights (an exact resume, the same state_dict
    interchange), the average travels in ck["optimizer"]["ema"] (load_checkpoint(weights="ema")).  The initial validation is on
    the raw weights: no average exists yet.  `config.lr_scale` / `config.wd_scale` ("prefix=multiplier,..."),
    `config.decoupled_decay` and `config.warmup_steps` give modules their own learning rate and decay, AdamW's decoupled decay
    and a linear warm-up (FusedAdam(lr_scales=, wd_scales=, decoupled_decay=, warmup_steps=)); each is passed on only when it is
    set, and the log then lists the multipliers per prefix and the segments per group.  A model built with `config.photo_flip` /
    `config.photo_crop` augments its photos in every train_step (model.UMPR.photo_augment; validation sees plain photos): one log
    line says so.  `config.mask_padding` is read by the model (model.UMPR.mask_padding); one log line states the setting, the
    checkpoints record it, and `config.resume` under the other setting is refused by load_checkpoint; `config.mask_control` and
    `config.unsort_gru` (model.UMPR.mask_control / .unsort_gru) are treated the same way.  A training loader with `set_epoch`
    (reviews.StoreLoader with a ReviewDraw: --review_pool / --word_dropout) is told the epoch at its head; its draws are a function
    of (seed, epoch, sample), so a run resumed inside an epoch skips the consumed batches and draws what the uninterrupted run
    drew, without a checkpoint key."""
    accum = int(getattr(config, "accum_steps", 1))
    if accum > 1 and parallel.active():
        raise NotImplementedError("training: --accum_steps > 1 runs on one rank only (no gradient exchange for accumulated arenas)")
    log = logger.info if logger else print
    valid_mse = evaluate_mse(model, valid_dataloader)
    log(f'Initial validation mse is {valid_mse:.6f}')
    start = time.perf_counter()
    ema_decay = float(getattr(config, "ema_decay", 0.0))
    averaged = {"ema_decay": ema_decay} if ema_decay > 0.0 else {}      # (off: the call is the one it was)
    grouped = {}                                                         # (each of the four passed on only when it is set)
    if getattr(config, "lr_scale", ""):
        grouped["lr_scales"] = parse_scales(config.lr_scale, "lr_scale")
    if getattr(config, "wd_scale", ""):
        grouped["wd_scales"] = parse_scales(config.wd_scale, "wd_scale")
    if getattr(config, "decoupled_decay", False):
        grouped["decoupled_decay"] = True
    if getattr(config, "warmup_steps", 0):
        grouped["warmup_steps"] = config.warmup_steps
    opt = FusedAdam(model, config.learning_rate, config.l2_regularization, config.lr_decay,
                    max_grad_norm=float(getattr(config, "grad_clip", 0.0)), **averaged, **grouped)
    if grouped:
        log('Optimiser: ' + ('decoupled weight decay (AdamW)' if opt.decoupled_decay else 'coupled L2')
            + (f', linear warm-up over {opt.warmup_steps} steps' if opt.warmup_steps else ''))
        for line in opt.group_summary():
            log('  ' + line)
    if averaged:
        log(f'Moving average of the weights: decay {ema_decay}, {opt.ema_bytes() / 1e6:.0f} MB more; validation and the '
            f'checkpoint choice run on the averaged weights')
    augment = getattr(model, "photo_augment", None)
    if augment is not None:
        log('Photo augmentation at the fetch, training forwards only: '
            + (f'random crop of {augment.min_area:.0%} to 100% of the image, sides 3:4 to 4:3' if augment.min_area < 1 else 'no crop')
            + ('; horizontal flip with probability 1/2' if augment.flip else '; no flip'))
    log('Padding mask in the ReviewNet softmaxes (--mask_padding): '
        + ('on - co-attention and S-Net word attention run over real tokens only' if getattr(model, "mask_padding", False)
           else 'off - padding takes part, as in the reference'))
    log('Padding mask in the ControlNet (--mask_control): '
        + ('ignored - UMPR-R has no ControlNet' if getattr(model, "review_net_only", False) and getattr(model, "mask_control", False)
           else 'on - C-Net maxima and the control S-Net run over real tokens only, a padded sentence contributes 0'
           if getattr(model, "mask_control", False) else 'off - padding takes part, as in the reference'))
    log('GRU output rows (--unsort_gru): '
        + ('on - every sentence keeps its own states' if getattr(model, "unsort_gru", False)
           else "off - the reference's double un-sort: a row holds the states of the sentence at its rank in the batch's length sort"))
    reducer = parallel.GradReducer(opt) if parallel.active() else None
    best_loss, batch_counter, first_epoch, skip, saved = 100, 0, 0, 0, False
    valid_every = int(getattr(config, "valid_every", 500))   # the reference hard-codes 500 (main.py:43)
    gen = _shuffle_generator(train_dataloader)
    resume = getattr(config, "resume", "")
    if resume:
        meta = load_checkpoint(resume, model, opt, map_location=next(model.parameters()).device)
        first_epoch, batch_counter = meta.get("epoch", 0), meta.get("batch_counter", 0)
        best_loss = meta.get("best_loss", best_loss)
        skip = meta.get("batch_in_epoch", 0)
        if gen is not None and "epoch_rng" in meta:
            gen.set_state(meta["epoch_rng"].cpu())
        log(f'Resumed from {resume}: epoch {first_epoch}, batch {batch_counter} ({skip} batches into the epoch)')

    def stepped(consumed):
        """behind every optimiser step; `consumed`: loader batches of this epoch the step has used up"""
        nonlocal batch_counter, best_loss, saved
        batch_counter += 1
        if batch_counter % valid_every == 0:
            if averaged:
                with opt.swapped_ema():
                    valid_mse = evaluate_mse(model, valid_dataloader)
            else:
                valid_mse = evaluate_mse(model, valid_dataloader)
            log(f'Epoch {epoch:2d}; batch {batch_counter:5d}; train loss {total_loss / max(total_samples, 1):.6f}; '
                f'valid mse{" (ema)" if averaged else ""} {valid_mse:.6f}' + clip_note(opt))
            if best_loss > valid_mse:        # valid_mse is all-reduced: every rank takes the same branch
                best_loss = valid_mse
                if rank == 0:
                    save_checkpoint(model_path, model, opt, epoch, batch_counter, best_loss, batch_in_epoch=consumed,
                                    epoch_rng=epoch_rng)
                saved = True
                if parallel.active():        # nobody runs ahead (and later loads) while rank 0 is still writing
                    torch.distributed.barrier()

    for epoch in range(first_epoch, config.train_epochs):
        total_loss, total_samples, consumed = 0.0, 0, 0
        t0 = time.perf_counter()
        epoch_rng = gen.get_state() if gen is not None else None
        _set_epoch(train_dataloader, epoch)
        for bi, batch in enumerate(train_dataloader):
            consumed = bi + 1
            if epoch == first_epoch and bi < skip:   # consumed before the checkpoint was taken
                continue
            update = consumed % accum == 0           # (always, without --accum_steps)
            pred, loss = train_step(model, opt, batch, world, reducer, update)
            total_loss += loss.item() * len(pred)
            total_samples += len(pred)
            if update:
                stepped(consumed)
        if accum > 1 and opt.pending > 0:            # the epoch ended inside a group: one step on the k' < k it holds
            opt.step()
            stepped(consumed)
        opt.epoch_end()
        dt = time.perf_counter() - t0
        log(f'Epoch {epoch:3d} done; train loss {total_loss / max(total_samples, 1):.6f}; '
            f'{world * total_samples / max(dt, 1e-9):.1f} samples/s' + clip_note(opt))
        if batch_counter > 50000:
            break
    sec = int(time.perf_counter() - start)
    log(f'End of training! Time used {sec // 3600}:{sec % 3600 // 60}:{sec % 60}.')
    return opt, saved
