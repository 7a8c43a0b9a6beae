"""The training driver (the role of direct_offset_output.py:243-390): shuffled epochs over format-(B) sequences, a validation loss
every `validation_interval` steps, a checkpoint after each validation, a final validation.

``Schedule`` is the pure-Python event stream of a run; ``fit`` drives a tracker through it: data.InputPrefetcher (decode and pack
on background threads) -> data.upload_staged (three uploads, one ntk_frames_crop_batch launch) -> the tracker's two-stream
pipeline (submit_features / train_on_submitted).  The host reads a loss -- and so synchronises -- only every `log_interval` steps
and after a validation, and calls tracker.check_step() exactly there.

Deviation from the reference.  direct_offset_output.py:308 and :361 assign the index the
validation batcher returns to the TRAINING position ``index`` instead of ``val_index``.  As coded, ``val_index`` stays 0, so every
validation scores the first validation batch `validation_batch` times, and the training position is reset to the second batch of
the epoch, so an epoch longer than `validation_interval` batches never ends.  Schedule walks ``val_index`` through the validation
list and leaves the training position alone: `validation_batch` distinct batches are scored and every epoch ends.
"""
import os
import random

import torch

from . import data, parallel


class Schedule(object):
    """The order of a training run, as an iterable of events:
        ("validate", step, [batch, ...])    before the batch of every step with step % validation_interval == 0 (step 0
                                            included, :300), and once more after the last epoch (:354-386)
        ("train", step, batch)              one optimiser step
    A batch is the list of sequence indices (into the training / validation list) THIS rank runs: every rank draws the same
    global batches of `batch_size` sequences and rank r takes parallel.shard_range(batch_size, r, world) of each.
    Rules of the reference: both lists are truncated to whole batches (:284-287); the training list is reshuffled every epoch
    (:294); the validation list is reshuffled before each validation (:302) and at most `validation_batch` batches of it are
    used (:322), the validation loss being their mean; `step` counts on across epochs (:290, :353).  The two shuffles draw from
    two generators derived from random.Random(seed), so the training order does not depend on how often validation runs.
    The stated deviation -- a validation walks the validation list and does not move the training position -- is described in
    the module's docstring."""

    def __init__(self, n_train, n_val, batch_size, seed=0, validation_interval=100, validation_batch=1, num_epochs=1, rank=0,
                 world=1):
        if batch_size < 1 or validation_interval < 1 or validation_batch < 1 or num_epochs < 0:
            raise ValueError("Schedule: batch_size, validation_interval and validation_batch must be at least 1, num_epochs at least 0")
        self.batch_size, self.seed = int(batch_size), seed
        self.n_train = int(n_train) // self.batch_size * self.batch_size
        self.n_val = int(n_val) // self.batch_size * self.batch_size
        self.validation_interval, self.validation_batch, self.num_epochs = int(validation_interval), int(validation_batch), int(num_epochs)
        self.lo, self.hi = parallel.shard_range(self.batch_size, rank, world)

    def steps(self):
        return self.num_epochs * (self.n_train // self.batch_size)

    def _shard(self, order, index):
        return order[index + self.lo:index + self.hi]

    def __iter__(self):
        base = random.Random(self.seed)
        train_rng, val_rng = random.Random(base.getrandbits(64)), random.Random(base.getrandbits(64))
        train, val = list(range(self.n_train)), list(range(self.n_val))

        def validation(step):
            val_rng.shuffle(val)
            starts = range(0, self.n_val, self.batch_size)[:self.validation_batch]
            return ("validate", step, [self._shard(val, val_index) for val_index in starts])

        step = 0
        for _epoch in range(self.num_epochs):
            train_rng.shuffle(train)
            for index in range(0, self.n_train, self.batch_size):
                if step % self.validation_interval == 0:
                    yield validation(step)
                yield ("train", step, self._shard(train, index))
                step += 1
        yield validation(step)


class FitResult(object):
    """What fit() did: `steps` optimiser steps; `validation` [(step, mean validation loss)]; `training` [(step, loss)] at the
    logged steps; `checkpoints` the paths written, one per validation."""

    def __init__(self):
        self.steps, self.validation, self.training, self.checkpoints = 0, [], [], []


def batch_names(seqs, batch, T):
    """Frame names (without suffix) of the sequences `batch` indexes, sequence-major, as sevenbyseven_get_batch orders them."""
    names = []
    for i in batch:
        folder, stems = seqs[i]
        if len(stems) != T:
            raise ValueError("sequence %s has %d frames; the tracker takes %d" % (folder, len(stems), T))
        names.extend(os.path.join(folder, stem) for stem in stems)
    return names


def tracker_inputs(tracker, batch_img, batch_gt, y_off, x_off):
    """get_input's four tensors -> what the tracker's steps take: (frames, gts0 [B,64] = frame 0's heat-map of each sequence,
    offsets [B,T,2] ordered (y, x))."""
    B, T = tracker.B, tracker.T
    gts0 = batch_gt.reshape(B, T, 64)[:, 0].contiguous()
    offsets = torch.stack([y_off.reshape(B, T), x_off.reshape(B, T)], dim=2).contiguous()
    return batch_img, gts0, offsets


def fit(tracker, train_seqs, val_seqs, *, num_epochs=1, validation_interval=100, validation_batch=1, log_interval=10, ckpt_dir,
        reverse_image=False, image_root=None, seed=0, on_event=None, prefetch=True, workers=None, decode="host"):
    """Train `tracker` (NTMOffsetTracker or DNCOffsetTracker, built with the VGG weights) on format-(B) sequences as
    data.get_valid_sequences returns them, in Schedule's order; each process of a data-parallel run calls it alike.
    Per step: the next training batch's input is taken from the prefetcher, uploaded and cropped in one launch, and its trunk
    pass submitted right after train_on_submitted() of the current batch, so trunk i+1 overlaps core i (across a validation the
    trunk pass is submitted after it).  A validation runs eval_loss over its batches, then tracker.check_step(), reads the mean
    on the host and writes ``<ckpt_dir>/model-<global_step>.pt``.  The training loss is read (after check_step()) at steps with
    step % log_interval == 0 and nowhere else: no other synchronisation.  `on_event`, when given, is called with
    ("validate", step, loss), ("checkpoint", step, path) and ("train", step, loss) -- loss None at a step that is not logged.
    prefetch=False decodes on the calling thread instead (measurements).  To resume, load_checkpoint() first: the checkpoint
    names go on from the tracker's global_step.  decode="device": baseline JPEG frames are decoded by ntk_jpeg_decode_batch on
    the device instead of by the prefetcher's threads (data.stage_batch; same bits, so the same losses and parameters).  The
    decoder's status of every batch since the last look is read where the loop synchronises anyway -- after check_step() at a
    logged step and at a validation -- and a frame it could not decode raises NtkError naming the file.  -> FitResult."""
    rank, world = parallel.world()
    sched = Schedule(len(train_seqs), len(val_seqs), tracker.B * world, seed, validation_interval, validation_batch, num_epochs,
                     rank, world)
    events = list(sched)

    def batches():                      # the frame names of every batch in the order of use, made as the prefetcher asks for them
        for kind, _step, payload in events:
            if kind == "validate":
                for b in payload:
                    yield batch_names(val_seqs, b, tracker.T)
            else:
                yield batch_names(train_seqs, payload, tracker.T)

    os.makedirs(ckpt_dir, exist_ok=True)
    emit = on_event if on_event is not None else (lambda event: None)
    res = FitResult()
    dev = tracker.device
    s_vgg, s_ntm = tracker._streams()
    if prefetch:
        source = data.InputPrefetcher(batches(), depth=2, image_root=image_root, workers=workers, decode=decode)
    else:
        one = data.Staging()
        source = (data.stage_batch(names, image_root, None, "rect", one, decode=decode) for names in batches())
    unchecked = []                      # decode="device": batches whose decoder status has not been read yet

    def check_decoded():
        while unchecked:
            unchecked.pop(0).check_status()

    def next_inputs():
        staged = next(source)
        frames, gts0, offsets = tracker_inputs(tracker, *data.upload_staged(staged, dev, reverse_image))
        if staged.status is not None:
            unchecked.append(staged)
        if not prefetch:
            staged.uploaded.synchronize()           # the one staging set is packed again by the next call
        return frames, gts0, offsets

    def submit():
        frames, gts0, offsets = next_inputs()
        frames.record_stream(s_vgg)                 # read by the trunk pass on the feature stream ...
        gts0.record_stream(s_ntm)                   # ... and by the core pass on its stream, after this function's names are gone
        offsets.record_stream(s_ntm)
        tracker.submit_features(frames)
        return gts0, offsets

    try:
        submitted = None
        for i, (kind, step, payload) in enumerate(events):
            if kind == "validate":
                losses = [tracker.eval_loss(*next_inputs()) for _b in payload]
                tracker.check_step()
                check_decoded()
                val = float(torch.cat(losses).double().mean().item()) if losses else None
                res.validation.append((step, val))
                emit(("validate", step, val))
                path = tracker.save_checkpoint(os.path.join(ckpt_dir, "model-%d.pt" % tracker.opt.global_step))
                res.checkpoints.append(path)
                emit(("checkpoint", step, path))
                continue
            if submitted is None:
                submitted = submit()
            loss = tracker.train_on_submitted(*submitted)
            res.steps += 1
            submitted = submit() if i + 1 < len(events) and events[i + 1][0] == "train" else None
            logged = None
            if step % log_interval == 0:
                tracker.check_step()
                check_decoded()
                logged = float(loss.item())
                res.training.append((step, logged))
            emit(("train", step, logged))
    finally:
        if prefetch:
            source.close()
        tracker.join()
    return res
