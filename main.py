#!/usr/bin/env python3
"""Entry point mirroring the reference's main.py (config surface: config.py, run recipes: readme.md:70-92).

    python main.py --data_dir synthetic --batch_size 64                       # single MI355X
    python main.py --data_dir synthetic --learning_rate 1e-3 --grad_clip 5.0  # clip the gradient to a global 2-norm of 5
    python main.py --data_dir synthetic --batch_size 32 --accum_steps 8       # one Adam step per 8 batches of 32: an effective 256
    python main.py --data_dir synthetic --learning_rate 1e-3 --ema_decay 0.999    # validate, choose the checkpoint and test on an
                                                                                  # exponential moving average of the weights
    python main.py --data_dir data/music --learning_rate 1e-3 --lr_scale visual_net.vgg16.=1e-3 --decoupled_decay True \
                   --warmup_steps 500                                         # fine-tune the VGG at 1e-6 while the rest trains at
                                                                              # 1e-3, AdamW's decay, 500 steps of linear warm-up
    python main.py --data_dir data/music --freeze_vgg True --feature_store_gb 1   # VGG as a fixed feature extractor, its output
                                                                                  # for every photo kept in 1 GB of HBM
    python main.py --data_dir data/music --freeze_conv True --pool5_store_gb 8    # freeze the conv base, train the classifier on
                                                                                  # each photo's pool5 row kept in 8 GB of HBM
    python main.py --data_dir data/music --photo_store_gb 1 --photo_flip True --photo_crop 0.3   # augment the photos of every
                                                                              # training step on the GPU: random crop >= 30 %, flip
    python main.py --data_dir data/music --review_net_only True --review_store True   # tokenised reviews kept in HBM: a batch
                                                                                      # travels as indices, one kernel pads its ids
    python main.py --data_dir data/music --review_net_only True --review_store True --review_pool 200 --word_dropout 0.1
                                                # every epoch shows a fresh draw of max_sent_count sentences out of up to 200 per
                                                # user and item, and replaces a tenth of the tokens by <UNK>, in the collate kernel
    python main.py --data_dir data/music --train_embedding True               # fine-tune the word vectors (frozen by default)
    python main.py --data_dir data/music --mask_padding True                  # attention softmaxes of the ReviewNet skip padding
    python main.py --data_dir data/music --mask_padding True --mask_control True --unsort_gru True   # ... the ControlNet skips it
                                                # too and every sentence keeps its own GRU states: batch-invariant predictions
    python main.py --data_dir data/music --train_embedding True --sparse_embedding True   # ... updating only the rows a step names
    python -m torch.distributed.run --nproc-per-node 8 --master-addr 127.0.0.1 main.py --data_dir synthetic

The model / optimiser / train / evaluate drivers are the MI355X-native ones (umpr_amd).  With a data_dir that holds
train.csv / valid.csv / test.csv / photos.json (the reference's layout, readme.md:41-60) the CSV + GloVe + JPEG
pipeline of umpr_amd/data.py feeds them; `--data_dir synthetic` trains on synthetic batches of exactly the layout
`batch_loader` produces (src/dataset.py:173-182), which is what the throughput numbers are quoted on.  Multi-GPU: every
rank collates the same global batch and keeps its contiguous chunk (DataParallel's scatter, main.py:82).
"""
import os
import sys
import time

import torch

from umpr_amd import parallel
from umpr_amd.config import Config
from umpr_amd.model import UMPR
from umpr_amd.optim import parse_scales
from umpr_amd.synthetic import make_batch
from umpr_amd.train import evaluate_mse, training


class SyntheticLoader:
    """Iterable of collated batches (the 8-tuple of src/dataset.py:173-182); lengths stay on the host."""

    def __init__(self, n_batches, config, vocab, seed, device):
        self.batches = []
        for i in range(n_batches):
            b = make_batch(seed + i, config.batch_size, vocab, len(config.views), config.photo_count,
                           config.max_sent_count, config.min_sent_count, config.max_ui_sent_count,
                           config.max_sent_length, review_net_only=config.review_net_only)
            self.batches.append(b)

    def __iter__(self):
        return iter(self.batches)

    def __len__(self):
        return len(self.batches)


class ShardedLoader:
    """DataLoader whose collate already cut every batch to this rank's contiguous chunk (DataParallel's scatter,
    main.py:82) - see umpr_amd.data.batch_loader(shard=...): indices are sharded BEFORE the photos are decoded.  Yields
    parallel.Shard tuples: the 8 tensors plus `.n_active`; a chunk may be empty when the last batch is short."""

    def __init__(self, loader, rank, world):
        self.loader, self.rank, self.world = loader, rank, world

    def __iter__(self):
        for b in self.loader:
            if self.world <= 1:
                yield b
                continue
            s = parallel.Shard(b[:8])
            s.n_active = int(b[8])
            yield s

    def __len__(self):
        return len(self.loader)

    def set_epoch(self, epoch):
        """passed on to a loader that draws per epoch (reviews.StoreLoader with a ReviewDraw)"""
        inner = getattr(self.loader, "set_epoch", None)
        if inner is not None:
            inner(epoch)


class _Collate:
    """Picklable collate (worker processes): src/dataset.py:173-182 via umpr_amd.data.batch_loader."""

    def __init__(self, ignore_photos, rank=0, world=1, store=None):
        self.ignore_photos = ignore_photos
        self.shard = (rank, world) if world > 1 else None
        self.store = store          # a PhotoStore's, FeatureStore's or Pool5Store's index (--photo_store_gb, --feature_store_gb,
                                    # --pool5_store_gb): photos the store holds are not decoded

    def __call__(self, samples):
        from umpr_amd.data import batch_loader
        # photos leave as decoded uint8 and are resized on the device (umpr_amd/photos.py): bit-identical, a fraction of the host work
        return batch_loader(samples, self.ignore_photos, shard=self.shard, resize_on_gpu=not self.ignore_photos,
                            store=None if self.ignore_photos else self.store)


def _agree(value, rank):
    """Rank 0's value on every rank (a timestamped default path must be the same file everywhere)."""
    if parallel.active():
        box = [value if rank == 0 else None]
        torch.distributed.broadcast_object_list(box, src=0)
        return box[0]
    return value


def _averaged_test(config, opt, saved):
    """The context the test phase runs in: with --ema_decay a run that wrote no checkpoint but took a step tests on the moving
    average of the weights, swapped under the model (a checkpoint, when there is one, was loaded with weights="ema" instead)."""
    import contextlib
    if config.ema_decay > 0 and not config.test_only and not saved and opt is not None and opt.ema_ready:
        return opt.swapped_ema()
    return contextlib.nullcontext()


def _unpooled(config):
    """`config` as the validation and test Datasets read it: --review_pool off, so that only the training set builds pools."""
    import copy
    plain = copy.copy(config)
    plain.review_pool = 0
    return plain


def run_real(config, rank, world, log):
    """main.py:64-99 of the reference: Word2vec -> Dataset -> DataLoader(collate) -> training -> test."""
    from torch.utils.data import DataLoader
    from umpr_amd.checkpoint import load_checkpoint
    from umpr_amd.data import Dataset, Word2vec
    d = config.data_dir
    photo_path, photo_json = os.path.join(d, 'photos'), os.path.join(d, 'photos.json')
    # like the reference (main.py:116-119) the default checkpoint name carries the start time, so a run that never
    # saves cannot pick up an older run's file in its test phase
    model_path = config.model_path or _agree(
        f"./model/{os.path.basename(d.strip('/'))}{time.strftime('%Y%m%d_%H%M%S')}.pt", rank)
    if config.test_only and not os.path.exists(model_path):
        log(f'{model_path} is not exist! (--test_only needs --model_path <trained checkpoint>)')
        sys.exit(-1)                                   # the reference exits here too (main.py:89-91)
    w2v = Word2vec(config.word2vec_file)
    # --photo_store_gb X: this rank keeps every resized photo it has decoded in X GB of device memory (150 528 B per photo, no
    # eviction) and decodes it once per run instead of once per epoch and validation pass (umpr_amd/photos.py::PhotoStore)
    # --freeze_vgg True --feature_store_gb X: the store keeps what the frozen VGG makes of a photo instead (4 000 B per photo): a
    # resident photo is neither decoded nor resized nor run through the VGG (umpr_amd/photos.py::FeatureStore)
    # --freeze_conv True --pool5_store_gb X: the store keeps the frozen conv base's pool5 row of a photo (100 352 B): a resident
    # photo is neither decoded nor resized nor run through the 13 conv layers, and the classifier trains on the stored row
    # (umpr_amd/photos.py::Pool5Store)
    store = None
    if config.pool5_store_gb > 0 and not config.review_net_only:
        from umpr_amd.photos import Pool5Store
        store = Pool5Store(config.device, capacity_bytes=int(config.pool5_store_gb * 1e9))
        log(f'Pool5 store: {store.slots} slots of {store.slot_bytes} B ({store.slots * store.slot_bytes / 1e9:.2f} GB) on '
            f'{config.device}' + ('; it replaces the photo store (--photo_store_gb): a photo whose pool5 row is resident is '
                                  'never resized' if config.photo_store_gb > 0 else ''))
    elif config.feature_store_gb > 0 and not config.review_net_only:
        from umpr_amd.photos import FeatureStore
        store = FeatureStore(config.device, capacity_bytes=int(config.feature_store_gb * 1e9))
        log(f'Feature store: {store.slots} slots of {store.slot_bytes} B ({store.slots * store.slot_bytes / 1e9:.2f} GB) on '
            f'{config.device}' + ('; it replaces the photo store (--photo_store_gb): a photo whose features are resident is '
                                  'never resized' if config.photo_store_gb > 0 else ''))
    elif config.photo_store_gb > 0 and not config.review_net_only:
        from umpr_amd.photos import PhotoStore
        store = PhotoStore(config.device, capacity_bytes=int(config.photo_store_gb * 1e9))
        log(f'Photo store: {store.slots} slots of {store.slot_bytes} B ({store.slots * store.slot_bytes / 1e9:.2f} GB) on '
            f'{config.device}')
    store_name = 'Pool5 store' if config.pool5_store_gb > 0 else 'Feature store' if config.feature_store_gb > 0 else 'Photo store'
    known = lambda data: store and store.register(data.photo_paths())
    collate = _Collate(config.review_net_only, rank, world, store.index if store else None)
    # --review_store True: each Dataset's tokenised reviews live on the device (umpr_amd/reviews.py::ReviewStore); the DataLoader
    # runs over (index, photo paths) with the settings it would have, its workers do the photo half of the collate only, and the
    # ids of a batch are written on the device from its indices.  Built for sharded batches, not run on more than one rank.
    if config.review_store:
        from umpr_amd.reviews import IndexView, PhotoCollate, ReviewStore, StoreLoader
        collate = PhotoCollate(config.review_net_only, rank, world, store.index if store else None)
    workers = max(0, int(getattr(config, "loader_workers", 0)))
    # decode + resize + collate in worker processes, pinned staging buffers, batches prefetched ahead of the GPU; with
    # loader_workers = 0 everything runs on the training thread, as in the reference (main.py:70-73)
    dl = dict(collate_fn=collate, num_workers=workers, pin_memory=True)
    if workers:
        dl.update(prefetch_factor=2, persistent_workers=True)

    def loader(data, name, draw=None, **kw):
        """The DataLoader of `data`, cut to this rank's chunks; with --review_store its text half comes from a ReviewStore, and
        with `draw` (the training set under --review_pool / --word_dropout) from a sampled collate"""
        if not config.review_store:
            return ShardedLoader(DataLoader(data, batch_size=config.batch_size, **kw, **dl), rank, world)
        reviews = ReviewStore(data, config.device)
        log(f'Review store ({name}): {reviews!r}')
        if draw is not None:
            wide = (reviews.pool_count["user"] > reviews.draw_keep()) | (reviews.pool_count["item"] > reviews.draw_keep())
            log(f'Sampled collate ({name}): a fresh draw of {reviews.draw_keep()} sentences per user and item pool every epoch'
                + (f' out of up to {config.review_pool}' if config.review_pool else ' (--review_pool 0: the pools are shuffled)')
                + f', word dropout {draw.word_dropout}; {reviews.nbytes} B on the device, {wide.mean():.1%} of the '
                f'{reviews.n_samples} samples have a pool above {reviews.draw_keep()} sentences; validation and test see the '
                'plain batches')
        return ShardedLoader(StoreLoader(DataLoader(IndexView(data), batch_size=config.batch_size, **kw, **dl), reviews, rank, world,
                                         draw=draw), rank, world)

    model = UMPR(config, w2v.embedding).to(config.device)
    os.makedirs(os.path.dirname(model_path) or '.', exist_ok=True)
    logger = None if rank else type('L', (), {'info': staticmethod(log)})
    saved, opt = False, None
    if not config.test_only:
        train_data = Dataset(os.path.join(d, 'train.csv'), photo_json, photo_path, w2v, config)
        valid_data = Dataset(os.path.join(d, 'valid.csv'), photo_json, photo_path, w2v, _unpooled(config))
        log(f'Training dataset contains {len(train_data)} samples.')
        known(train_data), known(valid_data)           # before the loaders exist: their workers copy the path table
        g = torch.Generator().manual_seed(0)  # same shuffle on every rank
        draw = None
        if config.review_pool or config.word_dropout > 0:         # the training loader only
            from umpr_amd.reviews import ReviewDraw
            draw = ReviewDraw(torch.initial_seed(), 0, config.word_dropout, w2v.word2index[w2v.unknown])
        train_dlr = loader(train_data, 'train', draw, shuffle=True, generator=g)
        valid_dlr = loader(valid_data, 'valid')
        opt, saved = training(train_dlr, valid_dlr, model, config, model_path, logger=logger, world=world, rank=rank)
        if store:
            log(f'{store_name} after training: {store.stats()}')
    if config.test_only or saved:
        load_checkpoint(model_path, model, map_location=config.device, weights="ema" if config.ema_decay > 0 else "model")
        log(f'Testing the checkpoint {model_path}' + (' (its moving average of the weights)' if config.ema_decay > 0 else ''))
    else:
        log('No checkpoint was written in this run (validation never improved at a multiple of the validation '
            'interval): testing the model as it stands at the end of training'
            + (' (the moving average of its weights)' if config.ema_decay > 0 and opt.ema_ready else ''))
    test_data = Dataset(os.path.join(d, 'test.csv'), photo_json, photo_path, w2v, _unpooled(config))
    known(test_data)
    test_dlr = loader(test_data, 'test')
    with _averaged_test(config, opt, saved):
        log(f"Test end, test mse is {evaluate_mse(model, test_dlr):.6f}")
    if store:
        log(f'{store_name} after the test: {store.stats()}')


def main():
    try:
        _main()
    except SystemExit:
        raise
    except BaseException:
        # A rank that dies inside a step leaves its peers blocked in the next RCCL collective: report, then leave with a
        # non-zero status at once (no orderly teardown that would itself wait for the peers) so that the launcher
        # (torch.distributed.run) tears the job down.
        import traceback
        traceback.print_exc()
        sys.stderr.flush()
        if parallel.active():
            os._exit(1)
        raise


# options the reference does not have
EXTRA_OPTIONS = {"synthetic_batches": 20, "synthetic_vocab": 400003, "synthetic_emb": 50, "vgg_weights": "", "resume": "",
                 "loader_workers": 0, "valid_every": 500, "dtype": "fp32", "photo_store_gb": 0.0, "grad_clip": 0.0,
                 "freeze_vgg": False, "feature_store_gb": 0.0, "train_embedding": False, "sparse_embedding": False,
                 "freeze_conv": False, "pool5_store_gb": 0.0, "accum_steps": 1, "review_store": False, "ema_decay": 0.0,
                 "lr_scale": "", "wd_scale": "", "decoupled_decay": False, "warmup_steps": 0, "photo_flip": False,
                 "photo_crop": 1.0, "mask_padding": False, "mask_control": False, "unsort_gru": False, "review_pool": 0,
                 "word_dropout": 0.0}


def check_flags(config):
    """Refuses, at start-up, combinations of options that cannot work."""
    if not isinstance(config.freeze_vgg, bool):
        sys.exit(f"--freeze_vgg takes True or False, got {config.freeze_vgg!r}")
    if not isinstance(config.train_embedding, bool):
        sys.exit(f"--train_embedding takes True or False, got {config.train_embedding!r}")
    if not isinstance(config.sparse_embedding, bool):
        sys.exit(f"--sparse_embedding takes True or False, got {config.sparse_embedding!r}")
    if not isinstance(config.review_store, bool):
        sys.exit(f"--review_store takes True or False, got {config.review_store!r}")
    if not isinstance(config.mask_padding, bool):
        sys.exit(f"--mask_padding takes True or False, got {config.mask_padding!r}")
    if not isinstance(config.mask_control, bool):
        sys.exit(f"--mask_control takes True or False, got {config.mask_control!r}")
    if not isinstance(config.unsort_gru, bool):
        sys.exit(f"--unsort_gru takes True or False, got {config.unsort_gru!r}")
    if isinstance(config.review_pool, bool) or not isinstance(config.review_pool, int) or \
            (config.review_pool != 0 and not config.max_sent_count < config.review_pool <= 1024):
        sys.exit(f"--review_pool takes 0 (off) or the sentences kept per user and item pool, max_sent_count = "
                 f"{config.max_sent_count} < N <= 1024, got {config.review_pool!r}")
    if isinstance(config.word_dropout, bool) or not isinstance(config.word_dropout, (int, float)) or \
            not 0 <= config.word_dropout < 1:
        sys.exit(f"--word_dropout takes the share of tokens replaced by <UNK> in a training batch, 0 <= p < 1 (0: off), got "
                 f"{config.word_dropout!r}")
    for option in ("review_pool", "word_dropout"):
        if getattr(config, option) and not config.review_store:
            sys.exit(f"--{option} needs --review_store True: the draw is made by the kernel that collates a batch from the store")
        if getattr(config, option) and config.data_dir == "synthetic":
            sys.exit(f"--{option} needs tokenised reviews (a --data_dir with train.csv): the synthetic batches carry finished id "
                     "tensors, which are not sampled")
    if config.sparse_embedding and not config.train_embedding:
        sys.exit("--sparse_embedding needs --train_embedding True: it chooses how a trainable table is updated (the rows a step "
                 "names only, as torch.optim.SparseAdam would)")
    if isinstance(config.accum_steps, bool) or not isinstance(config.accum_steps, int) or config.accum_steps < 1:
        sys.exit(f"--accum_steps takes a whole number >= 1 (micro-batches per optimiser step), got {config.accum_steps!r}")
    if config.accum_steps > 1 and config.sparse_embedding:
        sys.exit("--accum_steps > 1 and --sparse_embedding True exclude each other: every micro-batch names other rows of the "
                 "table (accumulate with --sparse_embedding False)")
    if isinstance(config.ema_decay, bool) or not isinstance(config.ema_decay, (int, float)):
        sys.exit(f"--ema_decay takes a number, 0 (off) or a decay in (0.5, 1), got {config.ema_decay!r}")
    if config.ema_decay != 0 and not 0.5 < config.ema_decay < 1:
        sys.exit(f"--ema_decay takes 0 (off) or a decay in the open interval (0.5, 1), got {config.ema_decay!r}")
    if config.ema_decay > 0 and config.sparse_embedding:
        sys.exit("--ema_decay > 0 and --sparse_embedding True exclude each other: the sparse table lives outside the arenas the "
                 "average is kept over (average with --sparse_embedding False)")
    for option in ("lr_scale", "wd_scale"):            # the syntax here; the prefixes are checked against the model's names
        try:                                           # by the optimiser (FusedAdam raises ValueError naming the prefix)
            scales = parse_scales(getattr(config, option), option)
        except ValueError as e:
            sys.exit(str(e))
        bad = [p for p, x in scales.items() if not (x > 0 if option == "lr_scale" else x >= 0) or x == float("inf")]
        if bad:
            sys.exit(f"--{option}: the multiplier of the prefix {bad[0]!r} must be finite and "
                     + ("> 0" if option == "lr_scale" else ">= 0") + f", got {scales[bad[0]]}")
    if not isinstance(config.decoupled_decay, bool):
        sys.exit(f"--decoupled_decay takes True or False, got {config.decoupled_decay!r}")
    if isinstance(config.warmup_steps, bool) or not isinstance(config.warmup_steps, int) or config.warmup_steps < 0:
        sys.exit(f"--warmup_steps takes a whole number >= 0 (optimiser steps of linear warm-up, 0: none), got "
                 f"{config.warmup_steps!r}")
    if config.pool5_store_gb > 0 and config.feature_store_gb > 0:
        sys.exit("--pool5_store_gb and --feature_store_gb exclude each other: --feature_store_gb belongs to --freeze_vgg True, "
                 "--pool5_store_gb to --freeze_conv True")
    if config.feature_store_gb < 0:
        sys.exit(f"--feature_store_gb must be >= 0, got {config.feature_store_gb}")
    if config.feature_store_gb > 0 and not config.freeze_vgg:
        sys.exit("--feature_store_gb needs --freeze_vgg True: the store keeps the VGG's output for every photo, which is a constant "
                 "of the run only while the VGG does not train")
    if not isinstance(config.freeze_conv, bool):
        sys.exit(f"--freeze_conv takes True or False, got {config.freeze_conv!r}")
    if config.freeze_conv and config.freeze_vgg:
        sys.exit("--freeze_conv True and --freeze_vgg True exclude each other: --freeze_vgg freezes the whole VGG, --freeze_conv its "
                 "conv base only (the classifier trains)")
    if config.pool5_store_gb < 0:
        sys.exit(f"--pool5_store_gb must be >= 0, got {config.pool5_store_gb}")
    if config.pool5_store_gb > 0 and not config.freeze_conv:
        sys.exit("--pool5_store_gb needs --freeze_conv True: the store keeps the conv base's pool5 for every photo, which is a "
                 "constant of the run only while the conv base does not train")
    if not isinstance(config.photo_flip, bool):
        sys.exit(f"--photo_flip takes True or False, got {config.photo_flip!r}")
    if isinstance(config.photo_crop, bool) or not isinstance(config.photo_crop, (int, float)) or not 0.08 <= config.photo_crop <= 1:
        sys.exit(f"--photo_crop takes the smallest share of the image a random crop keeps, 0.08 <= s <= 1 (1: no crop), got "
                 f"{config.photo_crop!r}")
    if (config.photo_flip or config.photo_crop < 1) and not config.review_net_only:      # UMPR-R has no photos: accepted, ignored
        for option in ("feature_store_gb", "pool5_store_gb"):
            if getattr(config, option) > 0:
                sys.exit(f"--photo_flip / --photo_crop and --{option} > 0 exclude each other: a stored feature would freeze one "
                         "draw of the augmentation (augment with --photo_store_gb, which keeps the plain photo)")
        if config.data_dir == "synthetic":
            sys.exit("--photo_flip / --photo_crop need decoded photos (a --data_dir with train.csv and photos/): the synthetic "
                     "batches carry float photo tensors, which are not augmented")


def _main():
    Config.extend(EXTRA_OPTIONS)
    config = Config()
    check_flags(config)
    rank, local, world = parallel.init_distributed()
    if not torch.cuda.is_available():
        sys.exit("main.py needs an MI355X: the UMPR hot path has no CPU fallback (use the reference for CPU runs)")
    config.device = torch.device("cuda", local)
    torch.cuda.set_device(config.device)
    log = (lambda m: print(time.strftime('%Y-%m-%d %H:%M:%S'), m, flush=True)) if rank == 0 else (lambda m: None)
    log(str(config))
    have_csv = os.path.exists(os.path.join(config.data_dir, 'train.csv'))
    if have_csv:
        return run_real(config, rank, world, log)
    g = torch.Generator().manual_seed(0)
    emb = torch.randn(config.synthetic_vocab, config.synthetic_emb, generator=g) * 0.4
    emb[:3] = 0
    model = UMPR(config, emb.numpy()).to(config.device)
    per_rank = max(1, config.synthetic_batches // world)
    train_dlr = SyntheticLoader(per_rank, config, config.synthetic_vocab, 1000 + 7919 * rank, config.device)
    valid_dlr = SyntheticLoader(max(1, per_rank // 4), config, config.synthetic_vocab, 5000 + 7919 * rank, config.device)
    model_path = config.model_path or './model/umpr_synthetic.pt'
    os.makedirs(os.path.dirname(model_path) or '.', exist_ok=True)
    opt, saved = None, False
    if not config.test_only:
        opt, saved = training(train_dlr, valid_dlr, model, config, model_path,
                              logger=None if rank else type('L', (), {'info': staticmethod(log)}), world=world, rank=rank)
    if config.ema_decay > 0 and (saved or (config.test_only and os.path.exists(model_path))):
        from umpr_amd.checkpoint import load_checkpoint
        load_checkpoint(model_path, model, map_location=config.device, weights="ema")
        log(f'Testing the moving average of the weights in {model_path}')
    with _averaged_test(config, opt, saved):
        mse = evaluate_mse(model, valid_dlr)
    log(f"Test end, test mse is {mse:.6f}")


if __name__ == '__main__':
    main()
