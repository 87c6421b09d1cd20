"""Checkpoint interchange and resume.

The reference only ever pickles the whole module when validation improves (main.py:43-52) and keeps no optimiser /
scheduler / epoch state.  Here a checkpoint is a plain dict of tensors and numbers (loadable with
``torch.load(..., weights_only=True)``): the model ``state_dict`` under the reference's key names - so the weights
move between the two implementations by ``state_dict`` - plus, optionally, the Adam moments, step count and learning
rate for an exact resume.  ``mask_padding`` records whether the ReviewNet ran with its padding mask (model.UMPR.mask_padding):
loading into a model built with the other setting is refused, and a file without the key counts as False.  ``mask_control`` and
``unsort_gru`` (model.UMPR.mask_control, .unsort_gru) are recorded and checked in the same way.
"""
from __future__ import annotations

import os

import torch

_META = ("epoch", "batch_counter", "best_loss", "batch_in_epoch", "epoch_rng", "rng_calls")


def save_checkpoint(path, model, opt=None, epoch=0, batch_counter=0, best_loss=None, batch_in_epoch=None,
                    epoch_rng=None):
    """`batch_in_epoch` batches of epoch `epoch` were consumed when the checkpoint was taken and `epoch_rng` is the state
    the loader's shuffle generator had when that epoch began: together they let a resumed run replay the epoch's order
    and skip what was already trained on.  The file appears atomically (written beside the target, then renamed)."""
    ck = {"model": {k: v.detach().cpu() for k, v in model.state_dict().items()},
          "epoch": int(epoch), "batch_counter": int(batch_counter)}
    if best_loss is not None:
        ck["best_loss"] = float(best_loss)
    if batch_in_epoch is not None:
        ck["batch_in_epoch"] = int(batch_in_epoch)
    if epoch_rng is not None:
        ck["epoch_rng"] = epoch_rng.clone()
    # forward-call counters that seed the dropout masks (model.VGG16._calls): part of an exact resume
    # --mask_padding changes what the ReviewNet computes without adding a parameter: recorded, and checked by load_checkpoint
    ck["mask_padding"] = bool(getattr(model, "mask_padding", False))
    ck["mask_control"] = bool(getattr(model, "mask_control", False))     # likewise: the ControlNet's mask ...
    ck["unsort_gru"] = bool(getattr(model, "unsort_gru", False))         # ... and which sentence's GRU states a row holds
    ck["rng_calls"] = {n: int(m._calls) for n, m in model.named_modules() if hasattr(m, "_calls")}
    if opt is not None:
        ck["optimizer"] = opt.state_dict()
    tmp = f"{path}.tmp{os.getpid()}"
    torch.save(ck, tmp)
    os.replace(tmp, path)


def load_checkpoint(path, model, opt=None, map_location="cpu", weights="model"):
    """Returns the metadata dict (epoch, batch_counter, best_loss).  Accepts a checkpoint of save_checkpoint or a bare
    state_dict file (e.g. ``torch.save(reference_model.state_dict(), path)`` written on the reference side).
    `weights="ema"` loads the state dict as `weights="model"` does, then copies each tensor of the moving average a run with
    --ema_decay left in ``ck["optimizer"]["ema"]`` over the parameter of that name: the model to validate and test with."""
    if weights not in ("model", "ema"):
        raise ValueError(f"load_checkpoint: weights must be 'model' or 'ema', got {weights!r}")
    ck = torch.load(path, map_location=map_location, weights_only=True)
    sd = ck["model"] if isinstance(ck, dict) and "model" in ck and isinstance(ck["model"], dict) else ck
    # before anything is written: weights trained with the padding mask are other weights than those trained without it (a
    # checkpoint from before the option, or a bare state_dict, was trained without)
    saved_mask = bool(ck.get("mask_padding", False)) if sd is not ck else False
    if saved_mask != bool(getattr(model, "mask_padding", False)):
        raise ValueError(f"{path} was written with --mask_padding {saved_mask} and the model is built with --mask_padding "
                         f"{not saved_mask}: resume or test it with --mask_padding {saved_mask} (the weights themselves are "
                         "interchangeable by state_dict)")
    for opt_name in ("mask_control", "unsort_gru"):
        was = bool(ck.get(opt_name, False)) if sd is not ck else False
        if was != bool(getattr(model, opt_name, False)):
            raise ValueError(f"{path} was written with --{opt_name} {was} and the model is built with --{opt_name} {not was}: "
                             f"resume or test it with --{opt_name} {was} (the weights themselves are interchangeable by state_dict)")
    ema = None
    if weights == "ema":                                # before anything is written
        ema = ck["optimizer"].get("ema") if isinstance(ck, dict) and isinstance(ck.get("optimizer"), dict) else None
        if not ema:
            raise ValueError(f"{path} holds no moving average of the weights: it was not written by a run with --ema_decay "
                             "(or before that run's first step); load it with weights='model' (--ema_decay 0)")
        params = dict(model.named_parameters())
        wrong = sorted(n for n, t in ema.items() if n not in params or params[n].numel() != t.numel())
        if wrong:
            raise ValueError(f"{path}: the moving average (--ema_decay) does not match the model's parameters: {wrong[:3]}")
    if opt is not None and isinstance(ck, dict) and "optimizer" in ck:
        opt.check_state_dict(ck["optimizer"])       # e.g. moments of a trainable VGG for a frozen one: before anything is overwritten
    model.load_state_dict(sd)
    # a bare state_dict: model.load_state_dict copied the parameters INTO the optimiser's arena views, so they stay attached -
    # nothing to restore, the moments stay fresh
    if opt is not None and isinstance(ck, dict) and "optimizer" in ck:
        opt.load_state_dict(ck["optimizer"])
    if ema is not None:
        with torch.no_grad():
            for n, t in ema.items():
                params[n].copy_(t.view(params[n].shape))
    meta = {k: ck[k] for k in _META if isinstance(ck, dict) and k in ck}
    for n, m in model.named_modules():
        if hasattr(m, "_calls") and n in meta.get("rng_calls", {}):
            m._calls = int(meta["rng_calls"][n])
    return meta
