"""NumPy restatement of the supervised protocol's rules (include/ntmtrack.h, ntk_track_supervise) and of the first-frame geometry
of ntk_track_restart_boxes, written from the rules, one frame at a time in plain Python on top of evaluate_util.frame_score and the
ntmtrack.geometry functions; and run_supervised, the reference run the validator is compared with: one B = 1 tracker per clip
driven from the host, which restarts through the existing reset."""
import numpy as np

import evaluate_util as U

VALID, SUM_IOU, FAILURES, RESTARTS, TRACKED, SKIPPED, FIRST_FAILURE, HEAD = 0, 1, 2, 3, 4, 5, 6, 7
MODE, COUNTDOWN, SINCE, STATE_INTS = 0, 1, 2, 3
TRACK, WAIT = 0, 1
INACTIVE, TRACKED_CODE, RESTART, FAILURE, SKIP = -1, 0, 1, 2, 3


def new_state(B):
    return np.zeros((B, STATE_INTS), dtype=np.int32)                # (TRACK, 0, 0)


def new_table(n_clips):
    table = np.zeros((n_clips, HEAD), dtype=np.float64)
    table[:, FIRST_FAILURE] = -1
    return table


def gt_valid(g):
    g = np.asarray(g, dtype=np.float64)
    return bool(np.isfinite(g).all() and g[2] > 0 and g[3] > 0)


def plan(state, table, gt, active, clip_of):
    """Before the pass: -> (track [B], restart [B], codes [B]); state and table change in place."""
    B = state.shape[0]
    track, restart, codes = np.zeros(B, np.uint8), np.zeros(B, np.uint8), np.full(B, INACTIVE, np.int8)
    for b in range(B):
        c = int(clip_of[b])
        if c < 0 or c >= table.shape[0] or (active is not None and not active[b]):
            continue
        st, row = state[b], table[c]
        if st[MODE] == TRACK:
            track[b], codes[b] = 1, TRACKED_CODE
            continue
        st[COUNTDOWN] = max(st[COUNTDOWN] - 1, 0)
        if st[COUNTDOWN] == 0 and gt_valid(gt[b]):
            restart[b], codes[b] = 1, RESTART
            row[RESTARTS] += 1
            st[MODE], st[SINCE] = TRACK, 0
        else:
            codes[b] = SKIP
            row[SKIPPED] += 1
    return track, restart, codes


def judge(state, table, regions, gt, track, clip_of, codes, skip, burn_in, failure_overlap):
    """After the pass: the tracked slots are scored; -> frame_iou [B] (NaN where the frame was not judged); codes completed in place."""
    B = state.shape[0]
    ious = np.full(B, np.nan)
    for b in range(B):
        c = int(clip_of[b])
        if c < 0 or c >= table.shape[0] or not track[b]:
            continue
        st, row = state[b], table[c]
        s = U.frame_score(regions[b], gt[b])
        if s is None:                                                # tracked, the object absent
            st[SINCE] += 1
            codes[b] = TRACKED_CODE
            continue
        o = s[0]
        ious[b] = o
        tracked = row[TRACKED]
        row[TRACKED] += 1
        if o <= failure_overlap:
            row[FAILURES] += 1
            if row[FIRST_FAILURE] < 0:
                row[FIRST_FAILURE] = tracked
            st[MODE], st[COUNTDOWN] = WAIT, skip
            codes[b] = FAILURE
            continue
        st[SINCE] += 1
        if st[SINCE] > burn_in:
            row[VALID] += 1
            row[SUM_IOU] += o
        codes[b] = TRACKED_CODE
    return ious


def walk(pred, gt, clip_of, n_clips, active=None, skip=5, burn_in=10, failure_overlap=0.0):
    """T frames of plan and judge over predictions that do not depend on the plan (a restart frame's prediction is ignored).
    -> (codes [T,B] int8, frame_iou [T,B], table, state)."""
    T, B = pred.shape[:2]
    state, table = new_state(B), new_table(n_clips)
    codes, ious = np.zeros((T, B), np.int8), np.full((T, B), np.nan)
    for t in range(T):
        track, _restart, codes[t] = plan(state, table, gt[t], None if active is None else active[t], clip_of)
        ious[t] = judge(state, table, pred[t], gt[t], track, clip_of, codes[t], skip, burn_in, failure_overlap)
    return codes, ious, table, state


def first_frame_geometry(regions, W, H, cropbox_grid=8, bbox_grid=6):
    """BatchNTMTracker._first_frame_inputs' host arithmetic through the ntmtrack.geometry functions.
    -> (state rows [n,10] float64, crop boxes [n,4] fp32, heat-map rows [n, g*g] fp32)."""
    from ntmtrack import geometry as G
    regions = np.asarray(regions, dtype=np.float64).reshape(-1, 4)
    rows = np.empty((len(regions), 10), dtype=np.float64)
    gts = np.empty((len(regions), cropbox_grid * cropbox_grid), dtype=np.float32)
    for i, (x1, y1, w, h) in enumerate(regions.tolist()):
        bbox = (y1, x1, y1 + h, x1 + w)
        nb = list(bbox) if (x1 < 1 and y1 < 1 and w < 1 and h < 1) else G.normalize_bbox((W, H), bbox)
        cb = G.calculate_cropbox(nb, cropbox_grid, bbox_grid)
        rows[i] = [W, H] + list(nb) + list(cb)
        gts[i] = G.generate_gt(G.apply_transformation(nb, G.calculate_transformation(cb)), cropbox_grid, bbox_grid).reshape(-1)
    return rows, rows[:, 6:10].astype(np.float32), gts


def run_supervised(make_single, clip, skip=5, burn_in=10, failure_overlap=0.0):
    """The protocol over one clip with one tracker of B = 1 (``make_single(first_images [1,H,W,3], regions [1,4])``), driven from
    the host: a tracked frame's region is read back and judged, a restart frame calls the tracker's reset([0], frame, gt).
    -> (regions [L-1,4] with NaN where the slot sat out and the ground truth on a restart frame, codes [L-1] int8, the clip's
    table row [HEAD], frame_iou [L-1])."""
    frames, gt = np.asarray(clip.frames), np.asarray(clip.regions, dtype=np.float64)
    L = len(gt)
    trk = make_single(frames[:1], gt[:1])
    state, table, clip_of = new_state(1), new_table(1), [0]
    regions, codes, ious = np.full((L - 1, 4), np.nan), np.zeros(L - 1, np.int8), np.full(L - 1, np.nan)
    for t in range(1, L):
        track, restart, c = plan(state, table, gt[t:t + 1], None, clip_of)
        if track[0]:
            regions[t - 1] = trk.track(frames[t:t + 1]).cpu().numpy()[0]
        elif restart[0]:
            trk.reset([0], frames[t:t + 1], gt[t:t + 1])
            regions[t - 1] = gt[t]
        ious[t - 1] = judge(state, table, regions[t - 1:t], gt[t:t + 1], track, clip_of, c, skip, burn_in, failure_overlap)[0]
        codes[t - 1] = c[0]
    return regions, codes, table[0], ious
