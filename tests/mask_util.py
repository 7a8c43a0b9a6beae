"""NumPy restatement of the mask rules of include/ntmtrack.h (NTK_MASK_*) through DENSE RASTERS, written from the rules in plain
Python, one mask at a time: the counts are decoded into a bool image of the box, the pixel set of a rectangle is built by testing
pixel centres, and everything is counted with ``&`` and ``sum`` -- no closed form is shared with the kernels.  On top of that the
score table (accumulate_mask, on the model of poly_util.accumulate_poly) and the supervised walk (walk_mask, on the model of
poly_util.walk_poly: supervised_util.plan as it is, judge restated with the mask overlap).

A set of masks is (cells int [..., 6], rle int [n_rle]) as the entries take it; ``n_rle`` is len(rle) unless given."""
import numpy as np

import evaluate_util as U
import supervised_util as S

CELL_INTS, OVERLAP_DOUBLES, MAX_PIXELS = 6, 3, 1 << 30


def decode(cell, rle, n_rle=None):
    """-> (x0, y0, bool [h,w]) of a present mask, None of an absent one."""
    x0, y0, w, h, first, count = [int(v) for v in cell]
    n_rle = len(rle) if n_rle is None else n_rle
    if not (w > 0 and h > 0 and w * h <= MAX_PIXELS and first >= 0 and count >= 0 and first + count <= n_rle):
        return None
    counts = [int(c) for c in rle[first:first + count]]
    if any(c < 0 for c in counts):
        return None
    flat, pos = np.zeros(w * h, dtype=bool), 0
    for k, c in enumerate(counts):
        if k % 2:
            flat[pos:pos + c] = True                    # NumPy drops what runs past the end
        pos += c
    if not flat.any():
        return None
    return x0, y0, flat.reshape(h, w)


def bounds(cell, rle, n_rle=None):
    """-> ((min col, min row, max col + 1 - min col, max row + 1 - min row) in frame pixels, |M|), or None for an absent mask."""
    m = decode(cell, rle, n_rle)
    if m is None:
        return None
    x0, y0, img = m
    cols, rows = np.nonzero(img.any(axis=0))[0], np.nonzero(img.any(axis=1))[0]
    rect = np.array([x0 + cols[0], y0 + rows[0], cols[-1] + 1 - cols[0], rows[-1] + 1 - rows[0]], dtype=np.float64)
    return rect, np.float64(img.sum())


def bounds_arrays(cells, rle, n_rle=None):
    """cells [..., 6] -> (rects [..., 4], area [...]), NaN for an absent mask."""
    cells = np.asarray(cells)
    rects, area = np.full(cells.shape[:-1] + (4,), np.nan), np.full(cells.shape[:-1], np.nan)
    for idx in np.ndindex(*cells.shape[:-1]):
        r = bounds(cells[idx], rle, n_rle)
        if r is not None:
            rects[idx], area[idx] = r
    return rects, area


def rect_pixels(p, x_lo, y_lo, width, height):
    """The pixel set of the rectangle p = (x, y, w, h) on the window of columns [x_lo, x_lo + width) and rows [y_lo, y_lo + height):
    negative sizes clamped to 0, corners first, pixel (c, r) inside when its centre lies in [x, x2) x [y, y2).  All False for a
    rectangle that is not finite."""
    p = np.asarray(p, dtype=np.float64)
    if not np.isfinite(p).all():
        return np.zeros((height, width), dtype=bool)
    x, y = p[0], p[1]
    x2, y2 = x + max(p[2], 0.0), y + max(p[3], 0.0)
    cc, rc = np.arange(x_lo, x_lo + width) + 0.5, np.arange(y_lo, y_lo + height) + 0.5
    return ((rc >= y) & (rc < y2))[:, None] & ((cc >= x) & (cc < x2))[None, :]


def overlap_counts(p, cell, rle, n_rle=None):
    """-> (|M n R|, |R|, |M|) as float64 [3]; NaNs for an absent mask.  Counted on a window that holds the mask's box and, with a
    margin, the whole rectangle (which is not clipped to any frame)."""
    m = decode(cell, rle, n_rle)
    if m is None:
        return np.full(3, np.nan)
    x0, y0, img = m
    h, w = img.shape
    p = np.asarray(p, dtype=np.float64)
    xa, ya, xb, yb = x0, y0, x0 + w, y0 + h
    if np.isfinite(p).all():
        xa, ya = min(xa, int(np.floor(p[0])) - 2), min(ya, int(np.floor(p[1])) - 2)
        xb, yb = max(xb, int(np.ceil(p[0] + max(p[2], 0.0))) + 2), max(yb, int(np.ceil(p[1] + max(p[3], 0.0))) + 2)
    assert (xb - xa) * (yb - ya) <= 1 << 24, "the test's raster window is %d x %d" % (xb - xa, yb - ya)
    frame = np.zeros((yb - ya, xb - xa), dtype=bool)
    frame[y0 - ya:y0 - ya + h, x0 - xa:x0 - xa + w] = img
    R = rect_pixels(p, xa, ya, xb - xa, yb - ya)
    assert not (R[0].any() or R[-1].any() or R[:, 0].any() or R[:, -1].any())       # the window does hold the whole rectangle
    return np.array([(frame & R).sum(), R.sum(), frame.sum()], dtype=np.float64)


def mask_iou(ov):
    """I / ((R + M) - I), one float64 division; 0.0 when I == 0."""
    i, r, m = [np.float64(v) for v in ov]
    if i == 0:
        return np.float64(0.0)
    return i / ((r + m) - i)


def frame_score(p, cell, rle, active=True, n_rle=None):
    """evaluate_util.frame_score for mask ground truth: None where the frame is not scored, else (iou, distance to the centre of
    the mask's bounds)."""
    b = bounds(cell, rle, n_rle)
    if not active or b is None:
        return None
    r = b[0]
    p = np.asarray(p, dtype=np.float64)
    if not np.isfinite(p).all():
        return np.float64(0.0), np.float64(np.inf)
    q = np.array([p[0], p[1], max(p[2], 0.0), max(p[3], 0.0)])
    dx, dy = (q[0] + q[2] / 2) - (r[0] + r[2] / 2), (q[1] + q[3] / 2) - (r[1] + r[3] / 2)
    return mask_iou(overlap_counts(p, cell, rle, n_rle)), np.sqrt(dx * dx + dy * dy)


def accumulate_mask(table, regions, cells, rle, clip_of, iou_thr, dist_thr, active=None):
    """evaluate_util.accumulate with the masks cells [T,B,6] / rle as ground truth: adds to the table in place, each slot's frames
    in order.  -> (frame_iou [T,B], centre distances [T,B]), NaN where a frame was not scored."""
    regions = np.asarray(regions, dtype=np.float64)
    T, B = regions.shape[:2]
    n_iou = len(iou_thr)
    ious, dists = np.full((T, B), np.nan), np.full((T, B), np.nan)
    for b in range(B):
        c = int(clip_of[b])
        if c < 0 or c >= table.shape[0]:
            continue
        row = table[c]
        for t in range(T):
            s = frame_score(regions[t, b], cells[t, b], rle, True if active is None else bool(active[t, b]))
            if s is None:
                continue
            iou, dist = s
            ious[t, b], dists[t, b] = iou, dist
            if np.isfinite(dist):
                row[U.SUM_DIST] += dist
            for k, thr in enumerate(dist_thr):
                row[U.HEAD + n_iou + k] += 1.0 if dist <= thr else 0.0
            if iou == 0.0:
                if row[U.FIRST_LOST] < 0:
                    row[U.FIRST_LOST] = row[U.FRAMES]
                row[U.LOST] += 1
            for k, thr in enumerate(iou_thr):
                row[U.HEAD + k] += 1.0 if iou > thr else 0.0
            row[U.SUM_IOU] += iou
            row[U.FRAMES] += 1
    return ious, dists


def clip_masks(regions):
    """A clip's ground truth (x0, y0, w, h, counts) per frame, row 0 left out -> (cells [L-1,1,6], rle) for the replays."""
    cells, rle = [], []
    for x0, y0, w, h, counts in regions[1:]:
        cells.append((x0, y0, w, h, len(rle), len(counts)))
        rle.extend(int(c) for c in counts)
    return np.asarray(cells, dtype=np.int64).reshape(-1, 1, CELL_INTS), np.asarray(rle, dtype=np.int64)


def score_clips_mask(regions_per_clip, frames_per_clip, iou_thr, dist_thr):
    """evaluate_util.score_clips for mask ground truth; frames_per_clip[i]: (x0, y0, w, h, counts) per frame of clip i."""
    table = U.new_table(len(regions_per_clip), len(iou_thr), len(dist_thr))
    for i, (r, frames) in enumerate(zip(regions_per_clip, frames_per_clip)):
        cells, rle = clip_masks(frames)
        accumulate_mask(table[i:i + 1], np.asarray(r)[:, None], cells, rle, [0], iou_thr, dist_thr)
    return table


def judge_mask(state, table, regions, cells, rle, track, clip_of, codes, skip, burn_in, failure_overlap):
    """supervised_util.judge with the mask overlap; cells [B,6]."""
    B = state.shape[0]
    ious = np.full(B, np.nan)
    for b in range(B):
        c = int(clip_of[b])
        if c < 0 or c >= table.shape[0] or not track[b]:
            continue
        st, row = state[b], table[c]
        s = frame_score(regions[b], cells[b], rle)
        if s is None:                                                # tracked, the object absent
            st[S.SINCE] += 1
            codes[b] = S.TRACKED_CODE
            continue
        o = s[0]
        ious[b] = o
        tracked = row[S.TRACKED]
        row[S.TRACKED] += 1
        if o <= failure_overlap:
            row[S.FAILURES] += 1
            if row[S.FIRST_FAILURE] < 0:
                row[S.FIRST_FAILURE] = tracked
            st[S.MODE], st[S.COUNTDOWN] = S.WAIT, skip
            codes[b] = S.FAILURE
            continue
        st[S.SINCE] += 1
        if st[S.SINCE] > burn_in:
            row[S.VALID] += 1
            row[S.SUM_IOU] += o
        codes[b] = S.TRACKED_CODE
    return ious


def walk_mask(pred, cells, rle, clip_of, n_clips, active=None, skip=5, burn_in=10, failure_overlap=0.0):
    """supervised_util.walk over the masks cells [T,B,6] / rle: plan sees the masks' bounds (NaN for an absent mask, so its "valid"
    is "present"), judge the masks.  A restart frame's prediction is ignored.
    -> (codes [T,B] int8, frame_iou [T,B], table, state, restart [T,B] uint8)."""
    T, B = pred.shape[:2]
    state, table = S.new_state(B), S.new_table(n_clips)
    codes, ious, restarts = np.zeros((T, B), np.int8), np.full((T, B), np.nan), np.zeros((T, B), np.uint8)
    rects, _area = bounds_arrays(cells, rle)
    for t in range(T):
        track, restarts[t], codes[t] = S.plan(state, table, rects[t], None if active is None else active[t], clip_of)
        ious[t] = judge_mask(state, table, pred[t], cells[t], rle, track, clip_of, codes[t], skip, burn_in, failure_overlap)
    return codes, ious, table, state, restarts
