"""Online single-frame tracker: the contract of test_tracker.NTMTracker
(test_tracker.py:104-405) -- ``NTMTracker(image, region)`` then ``track(image) -> Rectangle`` -- on the HIP
path.  The reference runs 65 separate ``sess.run`` calls per frame and round-trips the whole NTM state
host<->device through feed_dict at every step (:284-299); here one frame is one crop kernel, one VGG trunk
pass, one serialise kernel and ONE 65-step sequence-kernel launch with the state resident on the device.

Quirk Q8 is kept: inference puts the delimiter row FIRST and reads the output of the LAST feature step
(:400-404, :274-282), although training puts it last and reads the delimiter step.
Box geometry (preprocess.py:73-149, :205-240 for behaviour) lives in ntmtrack.geometry.
"""
import collections
import ctypes
import inspect

import numpy as np
import torch

from . import _lib
from ._lib import upload as _upload         # host array -> device tensor through a pinned asynchronous copy: no synchronisation
from .ntm import NTMCell, _P, _np, gemm_nt
from .regions import as_round_truth         # a round's ground truth by kind: rectangles, polygons or masks
from .regions import MASK_OVERLAP_DOUBLES, POLY_DOUBLES     # noqa: F401  (not used here any more; callers read them as online.X)
from .tracker import GRID_N, GRID_START, GRID_STEP, NUM_FEATURES
from .vgg import VGG16Conv43

Rectangle = collections.namedtuple("Rectangle", ["x", "y", "width", "height"])     # vot.py:23-25

VGG_MEAN = (123.68, 116.78, 103.94)


# ---- box geometry lives in ntmtrack.geometry (one implementation); re-exported here for callers of this module
from .geometry import (normalize_bbox, calculate_cropbox, calculate_transformation, apply_transformation,   # noqa: E402,F401
                       offset_bbox, discrete_gauss, generate_gt)


def crop_and_resize(image, box, crop=224, mean=VGG_MEAN, out=None):
    """(image [H,W,3] fp32 device tensor - mean) cropped to `box` (normalised y1,x1,y2,x2) and resized bilinearly."""
    H, W, C = image.shape
    if out is None:
        out = torch.empty((crop, crop, C), device=image.device, dtype=torch.float32)
    m = torch.tensor(mean, device=image.device, dtype=torch.float32) if mean is not None else None
    y1, x1, y2, x2 = [float(v) for v in box]
    _lib.check(_lib.lib().ntk_crop_and_resize(_P(image.contiguous()), H, W, C, _np(m), y1, x1, y2, x2, _P(out), crop, crop, 0.0,
                                              _lib.stream()), "ntk_crop_and_resize")
    return out


class NTMTracker(object):
    """test_tracker.NTMTracker on the HIP path.  `image`: [H,W,3] RGB array (uint8 or float), `region`: (x, y, w, h)
    in pixels (or normalised if all < 1, :306-309).  `cell`: an ntmtrack.ntm.NTMCell with loaded parameters;
    `vgg`: a VGG16Conv43."""

    def __init__(self, image, region, cell, vgg, cropbox_grid=8, bbox_grid=6, device="cuda"):
        self.cell, self.vgg = cell, vgg
        self.device = torch.device(device)
        self.cropbox_grid, self.bbox_grid = cropbox_grid, bbox_grid
        self.frame = 0
        self.init_region = region
        img = self._to_device(image)
        h, w, _ = img.shape
        self.image_size = (w, h)
        self._update_bbox(self.image_size, region)
        self.state = self.cell.zero_state(1)
        feats = self._preprocess_image(img, True)
        self._run_tracker(feats)                    # this output is discarded (test_tracker.py:146-148)

    def _to_device(self, image):
        t = torch.as_tensor(np.asarray(image), dtype=torch.float32) if not torch.is_tensor(image) else image.float()
        return t.to(self.device).contiguous()

    def _update_bbox(self, image_size, region):     # test_tracker.py:300-329
        x1, y1, w, h = region
        normalized = x1 < 1 and y1 < 1 and w < 1 and h < 1
        bbox = (y1, x1, y1 + h, x1 + w)
        self.normalized_bbox = list(bbox) if normalized else normalize_bbox(image_size, bbox)
        self.cropbox = calculate_cropbox(self.normalized_bbox, self.cropbox_grid, self.bbox_grid)
        self.transformation = calculate_transformation(self.cropbox)

    def _preprocess_image(self, img, is_first_frame):
        """-> serialised block [1, 65, ldx] on the device: delimiter row first, then the 64 feature rows (:370-405)."""
        crop = crop_and_resize(img, self.cropbox)
        self.cropped_input_image = crop
        try:
            fmap = self.vgg(crop.unsqueeze(0), latency=True)             # one frame per call: the trunk form with the shorter critical path
        except TypeError:                                                # (a caller's own trunk object without the flag)
            fmap = self.vgg(crop.unsqueeze(0))
        gts0 = None
        if is_first_frame:
            gt = generate_gt(apply_transformation(self.normalized_bbox, self.transformation), self.cropbox_grid, self.bbox_grid)
            gts0 = torch.as_tensor(gt.reshape(1, -1), dtype=torch.float32).to(self.device).contiguous()
        ldx = self.cell.input_ldx
        X = torch.empty((1, NUM_FEATURES + 1, ldx), device=self.device)
        _lib.check(_lib.lib().ntk_gather_serialize_online(_P(fmap), _np(gts0), _P(X), 1, 1, fmap.shape[1], fmap.shape[2],
                                                          fmap.shape[3], ldx, GRID_START, GRID_STEP, GRID_N, _lib.stream()),
                   "ntk_gather_serialize_online")
        return X

    def _run_tracker(self, X):
        logits, _o, self.state, _rec = self.cell.run_sequence(X, self.state, record=False, want_outputs=False)
        return logits

    def _initial_normal_bbox(self):
        width = self.bbox_grid / float(self.cropbox_grid)
        return [.5 - width / 2, .5 - width / 2, .5 + width / 2, .5 + width / 2]

    def _decode_bbox(self, normalized_bbox):
        y1, x1, y2, x2 = apply_transformation(normalized_bbox, np.linalg.inv(self.transformation))
        w, h = self.image_size
        y1, x1, y2, x2 = y1 * h, x1 * w, y2 * h, x2 * w
        return Rectangle(x1, y1, x2 - x1, y2 - y1)

    def track(self, image):
        """One frame: returns the new region as Rectangle(x, y, width, height) in image coordinates."""
        self.frame += 1
        img = self._to_device(image)
        logits = self._run_tracker(self._preprocess_image(img, False))
        offsets = torch.tanh(logits[0, -1]).cpu().numpy()          # output of the LAST step (:274-282); 2 values -> host
        self.offsets = offsets
        self.output_bbox = offset_bbox(self._initial_normal_bbox(), offsets)
        region = self._decode_bbox(self.output_bbox)
        self._update_bbox(self.image_size, region)
        return region


# ---- batched online tracker: boxes, crops and state stay on the device ---------------------------------------------------

STATE_DOUBLES = 10           # include/ntmtrack.h NTK_TRACK_STATE_*: [w, h, object box y1 x1 y2 x2, crop box y1 x1 y2 x2]


def crop_and_resize_batch(images, frame_of, boxes, crop=224, mean=None, out=None):
    """images [F,H,W,C] fp32 or uint8 device tensor; frame_of int32 [B] and boxes fp32 [B,4] (normalised y1,x1,y2,x2) on the
    device; mean fp32 [C] device tensor or None -> (images[frame_of[b]] - mean) cropped to boxes[b], [B,crop,crop,C] fp32.
    One launch; a frame index outside [0,F) gives the extrapolation value (0) for that tracker."""
    F, H, W, C = images.shape
    B = boxes.shape[0]
    if images.dtype not in (torch.float32, torch.uint8):
        raise _lib.NtkError("crop_and_resize_batch: images must be fp32 or uint8, not %s" % images.dtype)
    if frame_of.dtype != torch.int32 or boxes.dtype != torch.float32 or frame_of.shape[0] != B:
        raise _lib.NtkError("crop_and_resize_batch: frame_of must be int32 [B] and boxes fp32 [B,4]")
    if out is None:
        out = torch.empty((B, crop, crop, C), device=images.device, dtype=torch.float32)
    _lib.check(_lib.lib().ntk_crop_and_resize_batch(_P(images.contiguous()), 1 if images.dtype == torch.uint8 else 0, F, H, W, C,
                                                    _P(frame_of), _P(boxes), _np(mean), _P(out), B, crop, crop, 0.0, _lib.stream()),
               "ntk_crop_and_resize_batch")
    return out


def select_rows(mask, a, b, out=None):
    """out[i] = mask[i] ? a[i] : b[i] over the leading dimension (mask uint8 [B] on the device; out may be a or b)."""
    B = a.shape[0]
    out = torch.empty_like(a) if out is None else out
    _lib.check(_lib.lib().ntk_select_rows(_P(mask), _P(a), _P(b), _P(out), B, a.numel() // B, _lib.stream()), "ntk_select_rows")
    return out


class BatchNTMTracker(object):
    """B online trackers in one pass per frame, with nothing read back to the host: NTMTracker's contract (same first-frame
    pass, same per-frame arithmetic) for several objects in one video (``images`` [1,H,W,3]) or one object in each of several
    clips of equal size (``images`` [B,H,W,3]); ``frame_of`` [B] says which image a tracker reads, in general.

    ``images``: [F,H,W,3], uint8 (kept as uint8 on the device) or float; host array or device tensor.  ``regions``: [B,4]
    (x, y, w, h) in pixels (normalised if all four < 1).  ``cell``: an NTMCell / StackedNTMCell with output_dim 2.
    ``track`` returns the regions as a [B,4] float64 DEVICE tensor; ``offsets`` [B,2], ``frame`` [B] (frames tracked since
    the slot was started) and ``state`` (the cell's state dict at batch B) live on the device too.  A host synchronisation
    happens only when the caller reads one of them."""

    def __init__(self, images, regions, cell, vgg, frame_of=None, cropbox_grid=8, bbox_grid=6, device="cuda"):
        if cell.dims is None or cell.dims.O != 2:
            raise _lib.NtkError("BatchNTMTracker: the cell must have parameters and output_dim 2 (dy, dx), not %s"
                                % (None if cell.dims is None else cell.dims.O))
        self.cell = cell
        self._setup(images, regions, vgg, cell.input_ldx, frame_of, cropbox_grid, bbox_grid, device)

    def _setup(self, images, regions, vgg, ldx, frame_of, cropbox_grid, bbox_grid, device):
        """Everything of the constructor that does not depend on the kind of core: fields, the first-frame pass (_first_frame),
        the per-frame buffers.  ldx: padded width of a serialised row."""
        self.vgg, self._ldx = vgg, ldx
        self.device = torch.device(device)
        self.cropbox_grid, self.bbox_grid = cropbox_grid, bbox_grid
        self.crop = 224
        # asked once, not with a try/except around every frame's trunk pass: a caller's own trunk object may not know the flag
        try:
            takes = inspect.signature(vgg).parameters
        except (TypeError, ValueError):
            takes = {}
        self._vgg_kw = {"latency": True} if "latency" in takes else {}
        self._vgg_takes_out = "out" in takes
        regions = np.asarray(regions, dtype=np.float64).reshape(-1, 4)
        B = self.B = regions.shape[0]
        if B < 1:
            raise _lib.NtkError("%s: no regions" % type(self).__name__)
        self.mean = torch.tensor(VGG_MEAN, device=self.device, dtype=torch.float32)
        imgs = self._images(images)
        self.frame_of = self._frame_table(frame_of, imgs.shape[0], B)
        self.box_state, self.cropbox32, self.state = self._first_frame(imgs, self.frame_of, regions)
        self.regions = _upload(regions, torch.float64, self.device)
        self.offsets = torch.zeros((B, 2), device=self.device, dtype=torch.float32)
        self.frame = torch.zeros((B,), device=self.device, dtype=torch.int32)
        # per-frame buffers, made once (each is consumed on the same stream before the next frame overwrites it)
        self._crops = torch.empty((B, self.crop, self.crop, 3), device=self.device, dtype=torch.float32)
        self._X = torch.empty((B, NUM_FEATURES + 1, ldx), device=self.device, dtype=torch.float32)
        self._gts0 = self._zero = None                  # made by the first frame that carries a restart mask

    # ---- host -> device plumbing (no synchronising call)
    def _images(self, images):
        if torch.is_tensor(images):
            t = images if images.dtype == torch.uint8 else images.to(torch.float32)
            t = t if t.device == self.device else (t.pin_memory() if not t.is_cuda else t).to(self.device, non_blocking=True)
        else:
            a = np.asarray(images)
            t = _upload(a, torch.uint8 if a.dtype == np.uint8 else torch.float32, self.device)
        if t.dim() == 3:
            t = t.unsqueeze(0)
        if t.dim() != 4:
            raise _lib.NtkError("images must be [F,H,W,3]")
        return t.contiguous()

    def _frame_table(self, frame_of, F, n):
        if frame_of is None:
            if F != 1 and F != n:
                raise _lib.NtkError("%d images for %d trackers: pass frame_of" % (F, n))
            return (torch.zeros((n,), device=self.device, dtype=torch.int32) if F == 1 else
                    torch.arange(n, device=self.device, dtype=torch.int32))
        if torch.is_tensor(frame_of) and frame_of.is_cuda:
            t = frame_of.to(torch.int32).contiguous()
        else:
            t = _upload(np.asarray(frame_of).reshape(-1), torch.int32, self.device)
        if t.shape[0] != n:
            raise _lib.NtkError("frame_of has %d entries for %d trackers" % (t.shape[0], n))
        return t

    def _mask(self, active, shape):
        if torch.is_tensor(active) and active.is_cuda:
            t = active.to(torch.uint8).contiguous()
        else:
            t = _upload(np.asarray(active).astype(bool), torch.uint8, self.device)
        if tuple(t.shape) != tuple(shape):
            raise _lib.NtkError("active has shape %s, expected %s" % (tuple(t.shape), tuple(shape)))
        return t

    # ---- the pieces of one pass (scripts/dev_online_batch_timing.py puts events between them)
    def _crop(self, imgs, frame_of, cropbox32, out=None):
        return crop_and_resize_batch(imgs, frame_of, cropbox32, self.crop, self.mean, out=out)

    def _trunk(self, crops):
        return self.vgg(crops, **self._vgg_kw)

    def _serialize(self, fmap, gts0, X=None):
        """Q8 serialisation (delimiter row first): [n, 65, ldx] on the device."""
        n, ldx = fmap.shape[0], self._ldx
        if X is None:
            X = torch.empty((n, NUM_FEATURES + 1, ldx), device=self.device, dtype=torch.float32)
        _lib.check(_lib.lib().ntk_gather_serialize_online(_P(fmap), _np(gts0), _P(X), n, 1, fmap.shape[1], fmap.shape[2],
                                                          fmap.shape[3], ldx, GRID_START, GRID_STEP, GRID_N, _lib.stream()),
                   "ntk_gather_serialize_online")
        return X

    def _sequence(self, X, mask):
        """65 steps from self.state; with a mask, an inactive tracker's rows of the new state are its old ones."""
        logits, _o, new, _rec = self.cell.run_sequence(X, self.state, record=False, want_outputs=False)
        if mask is not None:
            for k, v in new.items():
                select_rows(mask, v, self.state[k], out=v)
        self.state = new
        return logits

    def _update_boxes(self, logits, mask):
        _lib.check(_lib.lib().ntk_track_boxes_update(_P(logits), self.B, logits.shape[1], float(self.cropbox_grid),
                                                     float(self.bbox_grid), _np(mask), _P(self.box_state), _P(self.cropbox32),
                                                     _P(self.regions), _P(self.offsets), _P(self.frame), _lib.stream()),
                   "ntk_track_boxes_update")

    def _first_frame_inputs(self, imgs, frame_of, regions):
        """-> (box state [n,10] f64, crop boxes [n,4] fp32, serialised first frame X [n,65,ldx] with its heat-map rows)."""
        n = regions.shape[0]
        H, W = imgs.shape[1], imgs.shape[2]
        rows, gts = np.empty((n, STATE_DOUBLES), dtype=np.float64), np.empty((n, NUM_FEATURES), dtype=np.float32)
        for i, (x1, y1, w, h) in enumerate(regions.tolist()):
            bbox = (y1, x1, y1 + h, x1 + w)
            nb = list(bbox) if (x1 < 1 and y1 < 1 and w < 1 and h < 1) else normalize_bbox((W, H), bbox)
            cb = calculate_cropbox(nb, self.cropbox_grid, self.bbox_grid)
            rows[i] = [W, H] + list(nb) + list(cb)
            gts[i] = generate_gt(apply_transformation(nb, calculate_transformation(cb)), self.cropbox_grid, self.bbox_grid).reshape(-1)
        box_state = _upload(rows, torch.float64, self.device)
        cropbox32 = box_state[:, 6:10].to(torch.float32).contiguous()
        X = self._serialize(self._trunk(self._crop(imgs, frame_of, cropbox32)), _upload(gts, torch.float32, self.device))
        return box_state, cropbox32, X

    def _first_frame(self, imgs, frame_of, regions):
        """NTMTracker.__init__ over the given trackers: box state from the regions (host geometry: the regions arrive from the
        host anyway), heat-map rows, zero state, one pass whose output is discarded.  -> (box state [n,10] f64, crop boxes
        [n,4] fp32, cell state at batch n), all on the device."""
        box_state, cropbox32, X = self._first_frame_inputs(imgs, frame_of, regions)
        n = regions.shape[0]
        _logits, _o, state, _rec = self.cell.run_sequence(X, self.cell.zero_state(n), record=False, want_outputs=False)
        return box_state, cropbox32, state                      # this output is discarded (test_tracker.py:146-148)

    def _scatter_state(self, idx, state):
        for k, v in state.items():
            self.state[k].index_copy_(0, idx, v)

    # ---- public
    def reset(self, slots, images, regions, frame_of=None):
        """Start new objects in the given slots (the first-frame pass on a sub-batch of len(slots) trackers, scattered into
        the slots); every other slot is untouched.  ``frame_of`` indexes ``images`` for this pass only (default: one image
        for all, or one per slot in order); the table ``track`` reads is not changed."""
        slots = [int(s) for s in slots]
        regions = np.asarray(regions, dtype=np.float64).reshape(-1, 4)
        if len(slots) != regions.shape[0] or len(set(slots)) != len(slots) or not all(0 <= s < self.B for s in slots):
            raise _lib.NtkError("reset: slots %s (distinct, in [0,%d)) for %d regions" % (slots, self.B, regions.shape[0]))
        imgs = self._images(images)
        box_state, cropbox32, state = self._first_frame(imgs, self._frame_table(frame_of, imgs.shape[0], len(slots)), regions)
        idx = _upload(np.asarray(slots), torch.int64, self.device)
        self.box_state.index_copy_(0, idx, box_state)
        self.cropbox32.index_copy_(0, idx, cropbox32)
        self._scatter_state(idx, state)
        self.regions.index_copy_(0, idx, _upload(regions, torch.float64, self.device))
        self.offsets.index_fill_(0, idx, 0)
        self.frame.index_fill_(0, idx, 0)

    def track(self, images, frame_of=None, active=None, restart=None, restart_regions=None):
        """One frame for every (active) tracker -> regions [B,4] (x, y, width, height) float64 on the device; an inactive
        tracker keeps its state, box, frame count and last region.  Everything is enqueued on the current stream.

        ``restart`` (uint8 [B]) with ``restart_regions`` (float64 [B,4], pixels or normalised), both on the device: a slot with
        restart[b] != 0 is STARTED on this frame's image from restart_regions[b] -- what ``reset([b], image, region)`` means --
        inside the same pass (one crop launch, one trunk pass, one sequence launch, whatever the masks hold); its region is the
        one given.  Every other slot is tracked or, with ``active``, left alone."""
        imgs = self._images(images)
        if frame_of is not None:
            self.frame_of = self._frame_table(frame_of, imgs.shape[0], self.B)
        mask = None if active is None else self._mask(active, (self.B,))
        if (restart is None) != (restart_regions is None):
            raise _lib.NtkError("track: restart and restart_regions come together")
        if restart is None:
            self._step(imgs, mask)
        else:
            self._step_restart(imgs, mask, *self._restart_args(restart, restart_regions))
        return self.regions.clone()

    def _step(self, imgs, mask):
        crops = self._crop(imgs, self.frame_of, self.cropbox32, out=self._crops)
        X = self._serialize(self._trunk(crops), None, X=self._X)
        self._update_boxes(self._sequence(X, mask), mask)

    # ---- a frame on which some slots are started instead of tracked
    def _restart_args(self, restart, regions):
        if not (torch.is_tensor(restart) and restart.is_cuda and restart.dtype == torch.uint8 and tuple(restart.shape) == (self.B,)
                and torch.is_tensor(regions) and regions.is_cuda and regions.dtype == torch.float64
                and tuple(regions.shape) == (self.B, 4)):
            raise _lib.NtkError("track: restart must be a uint8 [%d] and restart_regions a float64 [%d,4] device tensor" % (self.B, self.B))
        return restart.contiguous(), regions.contiguous()

    def _restart_boxes(self, restart, regions, mask):
        """ntk_track_restart_boxes: the restarted slots' box state, crop boxes, regions and heat-map rows -> (heat-map rows
        [B,64], the mask of the slots the sequence advances, the mask of the slots whose output moves their box)."""
        if self._gts0 is None:
            self._gts0 = torch.empty((self.B, NUM_FEATURES), device=self.device, dtype=torch.float32)
            self._run_mask = torch.empty((self.B,), device=self.device, dtype=torch.uint8)
            self._move_mask = torch.empty((self.B,), device=self.device, dtype=torch.uint8)
        both_int = isinstance(self.bbox_grid, int)
        sigma = float(self.bbox_grid // 3 if both_int else self.bbox_grid / 3)          # generate_gt's, focus = 3
        _lib.check(_lib.lib().ntk_track_restart_boxes(_P(regions), _P(restart), _np(mask), self.B, float(self.cropbox_grid),
                                                      float(self.bbox_grid), sigma, NUM_FEATURES, _P(self.box_state),
                                                      _P(self.cropbox32), _P(self.regions), _P(self.offsets), _P(self.frame),
                                                      _P(self._gts0), _P(self._run_mask), _P(self._move_mask), _lib.stream()),
                   "ntk_track_restart_boxes")
        return self._gts0, self._run_mask, self._move_mask

    def _features(self, imgs):
        return self._trunk(self._crop(imgs, self.frame_of, self.cropbox32, out=self._crops))

    def _zero_rows(self, restart):
        """The restarted slots' rows of the recurrent state become rows of the zero state (made once), in one launch."""
        if self._zero is None:
            self._zero = self.cell.zero_state(self.B)
            self._zero_keys = sorted(self._zero)
            rows = [self._zero[k].numel() // self.B for k in self._zero_keys]
            self._zero_rows_c = (ctypes.c_longlong * len(rows))(*rows)
            self._zero_table = _upload(np.array([self._zero[k].data_ptr() for k in self._zero_keys], dtype=np.int64), torch.int64,
                                       self.device)
            self._state_tables = {}
        # the cell returns its new state in fresh tensors: one pointer table per set of addresses the allocator hands out
        ptrs = tuple(self.state[k].data_ptr() for k in self._zero_keys)
        table = self._state_tables.get(ptrs)
        if table is None:
            if len(self._state_tables) >= 64:
                self._state_tables.clear()
            table = self._state_tables[ptrs] = _upload(np.array(ptrs, dtype=np.int64), torch.int64, self.device)
        state_keep(restart, 1, self.B, self._zero_table, table, self._zero_rows_c)

    def _step_restart(self, imgs, mask, restart, regions):
        gts0, run, move = self._restart_boxes(restart, regions, mask)
        X = self._serialize(self._features(imgs), gts0, X=self._X)
        self._zero_rows(restart)
        self._update_boxes(self._sequence(X, None if mask is None else run), move)

    def track_clip(self, frames, active=None, supervisor=None, gt=None, clip_of=None):
        """frames [T,F,H,W,3] -> regions [T,B,4] float64 on the device: T calls of track on one stream, no synchronisation.
        active: [T,B] (nullable).  With a ``supervisor`` (evaluate.Supervisor), the round's ground truth ``gt`` [T,B,4] float64
        and ``clip_of`` int32 [B] on the device, every frame is plan -> the pass with the planned masks -> judge: a slot that
        lost its object is restarted from the ground truth inside the pass.  ``gt`` may be [T,B,16] polygons (include/ntmtrack.h,
        NTK_POLY_*): plan and judge take the polygons, a restart starts from the polygon's bounding rectangle, which one
        ntk_track_poly_bounds launch computes for the whole round.  ``gt`` may be an evaluate.MaskRound (segmentation masks,
        NTK_MASK_*): per frame plan on the masks' rects[t], the pass with restarts from rects[t], one ntk_track_mask_overlaps
        of the frame's B masks against the tracked regions, judge; the round's ``gt.overlap`` [T,B,3] holds them afterwards.
        The loop is one for the three kinds (regions.as_round_truth: ``rects``, ``after_pass``).  The supervisor's ``codes``
        [T,B] int8 then say what each slot did on each frame; a slot that sat a frame out repeats its last region."""
        T = len(frames)
        if not torch.is_tensor(frames) and not isinstance(frames, (list, tuple)):
            a = np.asarray(frames)
            frames = _upload(a, torch.uint8 if a.dtype == np.uint8 else torch.float32, self.device)
        masks = None if active is None else self._mask(active, (T, self.B))
        out = torch.empty((T, self.B, 4), device=self.device, dtype=torch.float64)
        if supervisor is not None:
            if clip_of is None:
                raise _lib.NtkError("track_clip: a supervisor needs gt and clip_of")
            truth = as_round_truth(gt, self.device, "track_clip with a supervisor", shape=(T, self.B))
            rects = truth.rects                         # what a restart starts from, for the whole round
            codes = torch.empty((T, self.B), device=self.device, dtype=torch.int8)
            for t in range(T):
                frame = truth[t]
                track, restart = supervisor.plan(frame, None if masks is None else masks[t], clip_of, codes=codes[t])
                self._step_restart(self._images(frames[t]), track, restart, rects[t])
                frame.after_pass(self.regions)
                supervisor.judge(self.regions, frame, clip_of, codes=codes[t])
                out[t].copy_(self.regions)
            supervisor.codes = codes
            return out
        for t in range(T):
            self._step(self._images(frames[t]), None if masks is None else masks[t])
            out[t].copy_(self.regions)
        return out


# ---- online DNC trackers: the recurrent state stays in the kernels' own layout and is advanced in place ----------------------

def state_keep(mask, keep_where, B, src_table, dst_table, row_floats):
    """For every b with (mask[b] != 0) == keep_where: row b of every tensor of the source table -> the same row of the
    destination table, one launch (ntk_dnc_state_keep).  mask uint8 [B] and the tables (int64 [n] tensors of data
    pointers) on the device; row_floats a ctypes c_longlong array of n row sizes."""
    _lib.check(_lib.lib().ntk_dnc_state_keep(_P(mask), int(keep_where), B, len(row_floats), _P(src_table), _P(dst_table), row_floats,
                                             _lib.stream()), "ntk_dnc_state_keep")


class BatchDNCTracker(BatchNTMTracker):
    """BatchNTMTracker's contract on a DNC core: B online trackers in one pass per frame, nothing read back to the host.  The
    reference has no online DNC tracker (its DNC script only trains and validates), so this contract is the project's own: the
    NTM online tracker's, serialisation included (delimiter row first, heat-map rows on the first frame only, the output of the
    LAST step read: quirk Q8 applies here as it does there).

    ``core``: a built ntmtrack.dnc.DNC (input 514, output 2), or a tracker.DNCOffsetTracker, whose core is taken: that tracker
    wires the core's two outputs straight to the offsets, so there is no projection outside the core and ``head`` must stay None.
    ``state`` is the core's serving state (dnc.DNCServingState: the eight buffers as the kernels take them, advanced in place by
    one launch per frame); ``state.to_state()`` gives the logical DNCState.  A frame with an ``active`` mask saves the inactive
    trackers' rows, runs the same launch, and puts them back (ntk_dnc_state_keep): an active tracker's state is never copied.
    The unmasked per-frame path allocates nothing and synchronises nothing; ``check()`` synchronises and raises if a cluster
    launch failed since the last check."""

    def __init__(self, images, regions, core, vgg, head=None, frame_of=None, cropbox_grid=8, bbox_grid=6, device="cuda"):
        core = getattr(core, "core", core)
        if head is not None:
            raise _lib.NtkError("BatchDNCTracker: the DNC trackers have no projection outside the core; head must be None")
        if core.D is None or core.O != 2:
            raise _lib.NtkError("BatchDNCTracker: the core must have parameters and output_size 2 (dy, dx), not %s"
                                % (None if core.D is None else core.O))
        self.core = core
        self._save = None
        self._setup(images, regions, vgg, core.ldx, frame_of, cropbox_grid, bbox_grid, device)
        B, S = self.B, NUM_FEATURES + 1
        # the serialise kernel writes every column of every row on every frame, the padding columns (as zeros) included
        self._fmap = None
        self._xproj = torch.empty((B * S, 4 * core.hid), device=self.device, dtype=torch.float32)
        self._logits = torch.empty((B, S, 2), device=self.device, dtype=torch.float32)

    @classmethod
    def from_tracker(cls, tracker, images, regions, vgg=None, **kw):
        """Serve a trained or checkpointed tracker.DNCOffsetTracker: its core, and its trunk unless ``vgg`` is given."""
        return cls(images, regions, tracker.core, vgg if vgg is not None else tracker.vgg, **kw)

    def _trunk(self, crops, out=None):
        if out is not None and self._vgg_takes_out:
            return self.vgg(crops, out=out, **self._vgg_kw)
        return self.vgg(crops, **self._vgg_kw)

    def _project(self, X, out=None):
        n = X.shape[0]
        return gemm_nt(X.view(n * X.shape[1], self._ldx), self.core.WxT, out=out)

    def _first_frame(self, imgs, frame_of, regions):
        """The first-frame pass over the given trackers from zero serving state; its output is discarded.
        -> (box state, crop boxes, serving state at batch n)."""
        box_state, cropbox32, X = self._first_frame_inputs(imgs, frame_of, regions)
        n = regions.shape[0]
        sub = self.core.serving_state(n)
        self.core.serve_projected(self._project(X), n, X.shape[1], sub)
        return box_state, cropbox32, sub

    def _scatter_state(self, idx, state):
        self.state.load(state.to_state(), rows=idx)

    def _keep_tables(self):
        """The second serving state and the device pointer tables of both, made on the first masked frame."""
        if self._save is None:
            self._save = self.core.serving_state(self.B)
            table = lambda st: _upload(np.array([t.data_ptr() for t in st.tensors()], dtype=np.int64), torch.int64, self.device)
            rows = self.state.row_floats()
            self._tables = (table(self.state), table(self._save), (ctypes.c_longlong * len(rows))(*rows))
        return self._tables

    def _sequence(self, X, mask):
        """65 steps in place on self.state.  With a mask: the inactive trackers' rows are saved first and put back after."""
        core = self.core
        xproj = self._project(X, out=self._xproj)
        if mask is None:
            return core.serve_projected(xproj, self.B, X.shape[1], self.state, out=self._logits)
        cur, save, rows = self._keep_tables()
        state_keep(mask, 0, self.B, cur, save, rows)
        logits = core.serve_projected(xproj, self.B, X.shape[1], self.state, out=self._logits)
        state_keep(mask, 0, self.B, save, cur, rows)
        return logits

    def _step(self, imgs, mask):
        crops = self._crop(imgs, self.frame_of, self.cropbox32, out=self._crops)
        if self._fmap is None:
            self._fmap = torch.empty((self.B, self.crop // 8, self.crop // 8, 512), device=self.device, dtype=torch.float32)
        X = self._serialize(self._trunk(crops, out=self._fmap), None, X=self._X)
        self._update_boxes(self._sequence(X, mask), mask)

    def _features(self, imgs):
        crops = self._crop(imgs, self.frame_of, self.cropbox32, out=self._crops)
        if self._fmap is None:
            self._fmap = torch.empty((self.B, self.crop // 8, self.crop // 8, 512), device=self.device, dtype=torch.float32)
        return self._trunk(crops, out=self._fmap)

    def _zero_rows(self, restart):
        """The restarted slots' rows of the serving state become rows of a fresh one (made on first use), in one launch."""
        if self._zero is None:
            self._zero = self.core.serving_state(self.B)
            self._zero_table = _upload(np.array([t.data_ptr() for t in self._zero.tensors()], dtype=np.int64), torch.int64, self.device)
        cur, _save, rows = self._keep_tables()
        state_keep(restart, 1, self.B, self._zero_table, cur, rows)

    def check(self):
        """Synchronises; raises NtkError if a cluster launch of the core failed since the last check (DNC.check_cluster)."""
        self.core.check_cluster()


class DNCTracker(object):
    """NTMTracker's contract on a DNC core: ``DNCTracker(image, region, core, vgg)`` then ``track(image) -> Rectangle``.  A
    BatchDNCTracker of one object (``batch``) whose region is read back to the host after every frame -- the one
    synchronisation of the online DNC path."""

    def __init__(self, image, region, core, vgg, cropbox_grid=8, bbox_grid=6, device="cuda"):
        self.batch = BatchDNCTracker(image, [region], core, vgg, cropbox_grid=cropbox_grid, bbox_grid=bbox_grid, device=device)
        self.frame = 0

    def track(self, image):
        self.batch._step(self.batch._images(image), None)
        self.frame += 1
        self.offsets = self.batch.offsets[0].cpu().numpy()
        return Rectangle(*self.batch.regions[0].tolist())
