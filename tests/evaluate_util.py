"""NumPy float64 restatement of the scoring rules of ntk_track_overlap_scores (include/ntmtrack.h), written from the rules, one
frame at a time in plain Python: the per-frame IoU with its skip, lost and clamp rules, the centre distance, and the table."""
import numpy as np

FRAMES, SUM_IOU, SUM_DIST, LOST, FIRST_LOST, HEAD = 0, 1, 2, 3, 4, 5


def rect_iou(p, g):
    """VOT / OTB overlap of two rectangles (x, y, w, h), w, h >= 0, on real coordinates.  Corners first, sides as differences of
    corners, so a box against itself is exactly 1 and boxes that only touch exactly 0."""
    p, g = [np.float64(v) for v in p], [np.float64(v) for v in g]
    px2, py2, gx2, gy2 = p[0] + p[2], p[1] + p[3], g[0] + g[2], g[1] + g[3]
    ix, iy = min(px2, gx2) - max(p[0], g[0]), min(py2, gy2) - max(p[1], g[1])
    if not (ix > 0 and iy > 0):
        return np.float64(0.0)
    with np.errstate(all="ignore"):
        inter = ix * iy
        union = ((px2 - p[0]) * (py2 - p[1]) + (gx2 - g[0]) * (gy2 - g[1])) - inter
        iou = inter / union
    if not (iou > 0):
        return np.float64(0.0)
    return np.float64(min(iou, 1.0))


def frame_score(p, g, active=True):
    """-> (iou, centre distance) of one frame, or None where the frame is not scored (inactive; ground truth not finite or with
    w <= 0 or h <= 0).  A prediction that is not finite: IoU 0, distance inf.  Negative predicted sizes count as 0."""
    g = np.asarray(g, dtype=np.float64)
    if not active or not np.isfinite(g).all() or g[2] <= 0 or g[3] <= 0:
        return None
    p = np.asarray(p, dtype=np.float64)
    if not np.isfinite(p).all():
        return np.float64(0.0), np.float64(np.inf)
    p = np.array([p[0], p[1], max(p[2], 0.0), max(p[3], 0.0)])
    dx, dy = (p[0] + p[2] / 2) - (g[0] + g[2] / 2), (p[1] + p[3] / 2) - (g[1] + g[3] / 2)
    return rect_iou(p, g), np.sqrt(dx * dx + dy * dy)


def new_table(n_clips, n_iou, n_dist):
    table = np.zeros((n_clips, HEAD + n_iou + n_dist), dtype=np.float64)
    table[:, FIRST_LOST] = -1
    return table


def accumulate(table, regions, gt, clip_of, iou_thr, dist_thr, active=None):
    """Adds regions / gt [T,B,4] to the table in place, each slot's frames in order.  -> (frame_iou [T,B] with NaN where a frame
    was not scored, the centre distances [T,B] likewise)."""
    regions, gt = np.asarray(regions, dtype=np.float64), np.asarray(gt, dtype=np.float64)
    T, B = regions.shape[:2]
    n_iou = len(iou_thr)
    ious, dists = np.full((T, B), np.nan), np.full((T, B), np.nan)
    for b in range(B):
        c = int(clip_of[b])
        if c < 0 or c >= table.shape[0]:
            continue
        row = table[c]
        for t in range(T):
            s = frame_score(regions[t, b], gt[t, b], True if active is None else bool(active[t, b]))
            if s is None:
                continue
            iou, dist = s
            ious[t, b], dists[t, b] = iou, dist
            if np.isfinite(dist):
                row[SUM_DIST] += dist
            for k, thr in enumerate(dist_thr):
                row[HEAD + n_iou + k] += 1.0 if dist <= thr else 0.0
            if iou == 0.0:
                if row[FIRST_LOST] < 0:
                    row[FIRST_LOST] = row[FRAMES]
                row[LOST] += 1
            for k, thr in enumerate(iou_thr):
                row[HEAD + k] += 1.0 if iou > thr else 0.0
            row[SUM_IOU] += iou
            row[FRAMES] += 1
    return ious, dists


def score_clips(regions_per_clip, gt_per_clip, iou_thr, dist_thr):
    """The table of whole clips: regions_per_clip[i] [L-1,4] against gt_per_clip[i][1:] (row 0 of the ground truth starts the
    tracker and is not scored)."""
    table = new_table(len(regions_per_clip), len(iou_thr), len(dist_thr))
    for i, (r, g) in enumerate(zip(regions_per_clip, gt_per_clip)):
        accumulate(table[i:i + 1], np.asarray(r)[:, None], np.asarray(g)[1:, None], [0], iou_thr, dist_thr)
    return table
