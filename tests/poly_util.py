"""NumPy float64 restatement of the polygon rules of include/ntmtrack.h (NTK_POLY_*), written from the rules in plain Python, one
region at a time: which pairs are vertices, when a region is present, its bounding rectangle, the overlap of a rectangle with a
polygon (Sutherland-Hodgman clipping against the four sides, then the shoelace area), the score table (accumulate_poly, on the
model of evaluate_util.accumulate) and the supervised walk (supervised_util.plan as it is, judge restated with the polygon
overlap)."""
import numpy as np

import evaluate_util as U
import supervised_util as S

MAX_POINTS, DOUBLES = 8, 16


def pad(points):
    """A list of (x, y) -> the 16-double region, NaN after the vertices."""
    out = np.full(DOUBLES, np.nan)
    flat = np.asarray(points, dtype=np.float64).reshape(-1)
    out[:len(flat)] = flat
    return out


def rect_points(r):
    x, y, w, h = [float(v) for v in r]
    return [(x, y), (x + w, y), (x + w, y + h), (x, y + h)]


def rotated_rect(cx, cy, w, h, theta):
    c, s = np.cos(theta), np.sin(theta)
    return [(cx + dx * c - dy * s, cy + dx * s + dy * c) for dx, dy in ((-w / 2, -h / 2), (w / 2, -h / 2), (w / 2, h / 2), (-w / 2, h / 2))]


def vertices(g):
    """The leading pairs whose two numbers are both finite."""
    g = np.asarray(g, dtype=np.float64).reshape(-1)
    pts = []
    for i in range(min(MAX_POINTS, len(g) // 2)):
        if not (np.isfinite(g[2 * i]) and np.isfinite(g[2 * i + 1])):
            break
        pts.append((np.float64(g[2 * i]), np.float64(g[2 * i + 1])))
    return pts


def area(pts):
    """Shoelace area about the first point, either orientation."""
    if len(pts) < 3:
        return np.float64(0.0)
    ox, oy = pts[0]
    s = np.float64(0.0)
    with np.errstate(all="ignore"):
        for i in range(len(pts)):
            a, b = pts[i], pts[(i + 1) % len(pts)]
            s = s + ((a[0] - ox) * (b[1] - oy) - (b[0] - ox) * (a[1] - oy))
    return abs(s) / 2


def bounds(g):
    """-> (min x, min y, max x - min x, max y - min y) of a present region, None of an absent one (fewer than 3 vertices, an empty
    bounding rectangle, a shoelace area of 0)."""
    pts = vertices(g)
    if len(pts) < 3:
        return None
    xs, ys = [p[0] for p in pts], [p[1] for p in pts]
    x, y, w, h = min(xs), min(ys), max(xs) - min(xs), max(ys) - min(ys)
    if not (w > 0 and h > 0 and area(pts) > 0):
        return None
    return np.array([x, y, w, h], dtype=np.float64)


def bounds_array(polys):
    """[..., 16] -> [..., 4], NaN for an absent region."""
    polys = np.asarray(polys, dtype=np.float64)
    out = np.full(polys.shape[:-1] + (4,), np.nan)
    for idx in np.ndindex(*polys.shape[:-1]):
        r = bounds(polys[idx])
        if r is not None:
            out[idx] = r
    return out


def clip(pts, x0, y0, x1, y1):
    """The polygon inside the open rectangle: one half-plane after the other, strict inside tests, a crossing point with the
    side's own coordinate."""
    def half(pts, axis, c, above):
        o, out = 1 - axis, []
        inside = (lambda p: p[axis] > c) if above else (lambda p: p[axis] < c)
        for i in range(len(pts)):
            a, b = pts[i], pts[(i + 1) % len(pts)]
            ia, ib = inside(a), inside(b)
            if ia != ib:
                q = [None, None]
                q[axis], q[o] = c, a[o] + (b[o] - a[o]) * ((c - a[axis]) / (b[axis] - a[axis]))
                out.append(tuple(q))
            if ib:
                out.append(b)
        return out
    for axis, c, above in ((0, x0, True), (0, x1, False), (1, y0, True), (1, y1, False)):
        if not pts:
            break
        pts = half(pts, axis, np.float64(c), above)
    return pts


def poly_iou(p, g):
    """|P n R| / (|P| + |R| - |P n R|) of the rectangle p = (x, y, w, h), w, h >= 0, and the present polygon g, clamped to [0,1]."""
    p = [np.float64(v) for v in p]
    pts = vertices(g)
    x1, y1 = p[0] + p[2], p[1] + p[3]
    left = clip(pts, p[0], p[1], x1, y1)
    if len(left) < 3:
        return np.float64(0.0)
    with np.errstate(all="ignore"):
        inter = area(left)
        union = ((x1 - p[0]) * (y1 - p[1]) + area(pts)) - inter
        iou = inter / union
    if not (iou > 0):
        return np.float64(0.0)
    return np.float64(min(iou, 1.0))


def frame_score(p, g, active=True):
    """evaluate_util.frame_score for a polygon ground truth: None where the frame is not scored, else (iou, distance to the centre
    of the polygon's bounding rectangle)."""
    r = bounds(g)
    if not active or r is None:
        return None
    p = np.asarray(p, dtype=np.float64)
    if not np.isfinite(p).all():
        return np.float64(0.0), np.float64(np.inf)
    p = np.array([p[0], p[1], max(p[2], 0.0), max(p[3], 0.0)])
    dx, dy = (p[0] + p[2] / 2) - (r[0] + r[2] / 2), (p[1] + p[3] / 2) - (r[1] + r[3] / 2)
    return poly_iou(p, g), np.sqrt(dx * dx + dy * dy)


def accumulate_poly(table, regions, gt, clip_of, iou_thr, dist_thr, active=None):
    """evaluate_util.accumulate with gt [T,B,16]: adds to the table in place, each slot's frames in order.
    -> (frame_iou [T,B], centre distances [T,B]), NaN where a frame was not scored."""
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


def score_clips_poly(regions_per_clip, gt_per_clip, iou_thr, dist_thr):
    """evaluate_util.score_clips for polygon ground truth [L,16] per clip."""
    table = U.new_table(len(regions_per_clip), len(iou_thr), len(dist_thr))
    for i, (r, g) in enumerate(zip(regions_per_clip, gt_per_clip)):
        accumulate_poly(table[i:i + 1], np.asarray(r)[:, None], np.asarray(g)[1:, None], [0], iou_thr, dist_thr)
    return table


def judge_poly(state, table, regions, gt, track, clip_of, codes, skip, burn_in, failure_overlap):
    """supervised_util.judge with the polygon overlap; gt [B,16]."""
    B = state.shape[0]
    ious = np.full(B, np.nan)
    for b in range(B):
        c = int(clip_of[b])
        if c < 0 or c >= table.shape[0] or not track[b]:
            continue
        st, row = state[b], table[c]
        s = frame_score(regions[b], gt[b])
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


def walk_poly(pred, gt, clip_of, n_clips, active=None, skip=5, burn_in=10, failure_overlap=0.0):
    """supervised_util.walk over gt [T,B,16]: plan sees the bounding rectangles (NaN for an absent region, so its "valid" is
    "present"), judge the polygons.  A restart frame's prediction is ignored.
    -> (codes [T,B] int8, frame_iou [T,B], table, state, restart [T,B] uint8)."""
    T, B = pred.shape[:2]
    state, table = S.new_state(B), S.new_table(n_clips)
    codes, ious, restarts = np.zeros((T, B), np.int8), np.full((T, B), np.nan), np.zeros((T, B), np.uint8)
    rects = bounds_array(gt)
    for t in range(T):
        track, restarts[t], codes[t] = S.plan(state, table, rects[t], None if active is None else active[t], clip_of)
        ious[t] = judge_poly(state, table, pred[t], gt[t], track, clip_of, codes[t], skip, burn_in, failure_overlap)
    return codes, ious, table, state, restarts
