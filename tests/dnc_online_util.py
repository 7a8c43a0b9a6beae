"""NumPy restatement of the online DNC loop for ONE object: what online.DNCTracker computes, from the oracles alone.  Box
geometry from ntmtrack.geometry, the crop from oracle.online_oracle.crop_and_resize, the trunk from oracle.ntm_oracle, the
online serialisation (delimiter row first, heat-map rows on the first frame only) from oracle.online_oracle.frame_block, the
core from oracle.dnc_oracle.dnc_step.  The reference has no online DNC tracker: the loop is the NTM online tracker's
(test_tracker.py:104-405) with the DNC core in the cell's place.

Crop and trunk run in float64.  The core runs in `core_dtype`: float32 by default, because the DNC's allocation weighting sorts
usages that are exact ties in float32 and differ at 1e-12 in float64 (tests/test_dnc_gpu.py:93-96) -- a float64 core orders them
differently from any float32 implementation; float64 is there to measure the float32 oracle's own error on a clip."""
import numpy as np

from ntmtrack import geometry as G
from oracle import dnc_oracle as D
from oracle import ntm_oracle as O
from oracle import online_oracle as OO

VGG_MEAN = np.array((123.68, 116.78, 103.94))
CROPBOX_GRID, BBOX_GRID, CROP = 8, 6, 224


def _boxes(size, region):
    """(normalised box, crop box, transformation) of a region (x, y, w, h), as NTMTracker._update_bbox."""
    w, h = size
    x1, y1, rw, rh = region
    bbox = (y1, x1, y1 + rh, x1 + rw)
    nb = list(bbox) if (x1 < 1 and y1 < 1 and rw < 1 and rh < 1) else G.normalize_bbox(size, bbox)
    cb = G.calculate_cropbox(nb, CROPBOX_GRID, BBOX_GRID)
    return nb, cb, G.calculate_transformation(cb)


def online_dnc_loop(cfg, params, vgg_weights, first_image, region, images, core_dtype=np.float32):
    """first_image, images[t]: [H,W,3] arrays (any dtype); region (x, y, w, h) in pixels.
    -> (offsets [T,2] (dy, dx), regions [T,4] (x, y, w, h) float64, final oracle DNCState)."""
    ws64 = {k: (w.astype(np.float64), b.astype(np.float64)) for k, (w, b) in vgg_weights.items()}
    p = {k: np.asarray(v).astype(core_dtype) for k, v in params.items()}
    H, W = first_image.shape[:2]
    size = (W, H)
    st = D.dnc_initial_state(cfg, 1, core_dtype)

    def frame(img, nb, cb, tr, first, st):
        crop = OO.crop_and_resize(np.asarray(img, dtype=np.float64) - VGG_MEAN, cb, CROP, CROP)
        fmap = O.vgg16_conv43(crop[None], ws64)
        gt = G.generate_gt(G.apply_transformation(nb, tr), CROPBOX_GRID, BBOX_GRID) if first else None
        blk = OO.frame_block(None, fmap, gt).astype(core_dtype)              # [65, 514]
        y = None
        for s in range(blk.shape[0]):
            y, st, _ = D.dnc_step(cfg, p, blk[s][None], st)
        return np.tanh(y[0].astype(np.float64)), st                          # the LAST step's output (quirk Q8)

    nb, cb, tr = _boxes(size, region)
    _, st = frame(first_image, nb, cb, tr, True, st)                         # the first frame's output is discarded
    width = BBOX_GRID / float(CROPBOX_GRID)
    init = [.5 - width / 2, .5 - width / 2, .5 + width / 2, .5 + width / 2]
    offsets, regions = [], []
    for img in images:
        off, st = frame(img, nb, cb, tr, False, st)
        y1, x1, y2, x2 = G.apply_transformation(G.offset_bbox(init, off), np.linalg.inv(tr))
        region = (x1 * W, y1 * H, (x2 - x1) * W, (y2 - y1) * H)
        offsets.append(off)
        regions.append(region)
        nb, cb, tr = _boxes(size, region)
    return np.array(offsets), np.array(regions, dtype=np.float64), st
