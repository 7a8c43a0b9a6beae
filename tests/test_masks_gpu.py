"""GPU: segmentation-mask ground truth on the device -- ntk_track_mask_bounds and ntk_track_mask_overlaps against the dense-raster
restatement of their rules (tests/mask_util.py) bit for bit, ntk_track_overlap_scores_mask and ntk_track_supervise_mask against
the restated table and walk, and evaluate.Validation over mask clips in both protocols, replayed on the host from the regions and
codes the device returned.

Model shapes, world and makers: those of tests/test_evaluate_gpu.py; the frames here are 64 x 96."""
import os

import numpy as np
import pytest
import torch

import evaluate_util as U
import mask_util as M
import supervised_util as S
import test_evaluate_gpu as TE
import test_polygon_gpu as TP
import test_supervised_gpu as TS
from test_evaluate_gpu import world                                  # noqa: F401  (the module-scoped fixture: cell, trunk, clips)

pytestmark = pytest.mark.gpu

same_bits = TE.same_bits
dev = TS.dev
H, W = 64, 96
SENT = -777.25
# The overlap of a frame is ONE float64 division of whole numbers below 2^53 on both sides, so it agrees bit for bit and so do
# the sums, which both sides form in frame order.  The centre distance goes through a square root and products that the host
# and the device may round differently in the last place: the bound tests/test_polygon_gpu.py holds it to, per scored frame.
DIST_ATOL = 1e-12


# ------------------------------------------------------------------------------------------------- the planted masks and rectangles
def chunk_counts(rng, k):
    """k counts of 1 .. 20 (about 10 k pixels of the 96 x 64 box: runs cross row ends)."""
    return rng.integers(1, 21, k).tolist()


def planted_masks():
    """-> list of (name, x0, y0, w, h, counts, present)."""
    rng = np.random.default_rng(41)
    masks = [("w = 1", 5, 3, 1, 7, [2, 3], True),
             ("h = 1", 4, 6, 9, 1, [3, 4], True),
             ("a single pixel", 7, 8, 1, 1, [0, 1], True),
             ("a first count of 0", 2, 2, 5, 4, [0, 3, 4, 2], True),
             ("zero-length runs in the middle", 3, 1, 6, 5, [2, 3, 0, 4, 5, 0, 0, 2], True),
             ("a run that ends exactly at a row end", 10, 4, 6, 4, [2, 4, 3, 2], True),
             ("a run that crosses three rows", 12, 20, 5, 5, [3, 10, 4, 1], True),
             ("counts that run past w h", 1, 1, 4, 3, [5, 20], True),
             ("a run that starts past w h", 30, 30, 4, 3, [2, 3, 10, 4], True),
             ("counts that stop short of w h", 0, 0, 8, 6, [4, 5], True),
             ("a filled box", 10, 5, 6, 4, [0, 24], True),
             ("a filled column", 20, 9, 1, 5, [0, 5], True),
             ("a filled row", 30, 2, 7, 1, [0, 7], True),
             ("a filled box, counts past w h", 0, 0, 3, 3, [0, 100], True),
             ("a filled box in two runs", 40, 30, 8, 8, [0, 30, 0, 34], True),
             ("a filled box partly outside the frame", -4, -2, 8, 6, [0, 48], True),
             ("a box that ends outside the frame", 90, 60, 10, 8, [7, 50], True),
             ("an all-zero mask", 3, 3, 4, 4, [16], False),
             ("no counts", 3, 3, 4, 4, [], False),
             ("only zero-length runs of ones", 3, 3, 4, 4, [2, 0, 5, 0], False),
             ("a negative count", 3, 3, 4, 4, [2, 3, -1, 4], False),
             ("a negative count past w h", 3, 3, 2, 2, [0, 9, 3, -2], False),
             ("w = 0", 3, 3, 0, 4, [0, 4], False),
             ("h < 0", 3, 3, 4, -1, [0, 4], False),
             ("more than 2^30 pixels", 0, 0, 65536, 32768, [0, 5], False)]
    for k in (63, 64, 65, 128, 129):
        masks.append(("%d counts" % k, 0, 0, 96, 64, chunk_counts(rng, k), True))
    masks.append(("129 counts, a negative one in the third chunk", 0, 0, 96, 64, chunk_counts(rng, 128) + [-1], False))
    masks.append(("200 counts that pass w h in the second chunk", 2, 1, 30, 20, chunk_counts(rng, 200), True))
    for i in range(12):                                              # random boxes and counts
        w, h = int(rng.integers(1, 40)), int(rng.integers(1, 30))
        k = int(rng.integers(1, 40))
        counts = rng.integers(0, max(2, 3 * w * h // (2 * k)), k).tolist()
        present = sum(min(sum(counts[:j + 1]), w * h) - min(sum(counts[:j]), w * h) for j in range(1, k, 2)) > 0
        masks.append(("random %d" % i, int(rng.integers(-5, 60)), int(rng.integers(-5, 35)), w, h, counts, present))
    return masks


def rectangles_for(b, box):
    """The predicted rectangles a mask is met with, from its bounds b = (x, y, w, h) (its box where it is absent)."""
    x, y, w, h = [float(v) for v in b]
    bx, by, bw, bh = [float(v) for v in box]
    return [("the bounds themselves", (x, y, w, h)),
            ("inside", (x + np.floor(w / 4), y + np.floor(h / 4), max(np.floor(w / 2), 1.0), max(np.floor(h / 2), 1.0))),
            ("covering", (x - 3.0, y - 2.0, w + 7.0, h + 5.0)),
            ("partial", (x + np.ceil(w / 2), y - 1.0, w + 2.0, h + 1.0)),
            ("disjoint", (x + w + 25.0, y + h + 13.0, 9.0, 6.0)),
            ("touching the box's right side", (bx + bw, by, 5.0, bh)),
            ("touching the box's top side", (bx, by - 4.0, bw, 4.0)),
            ("corners at k + 0.5", (x + 0.5, y - 0.5, w, h + 1.0)),
            ("corners at k + 0.5, one pixel less", (x - 1.5, y + 0.5, w + 1.0, max(h - 1.0, 0.0))),
            ("negative coordinates", (-20.5, -30.25, x + w + 20.5, y + h + 29.0)),
            ("partly outside the frame", (x + 1.0, y + 1.0, 200.0, 150.0)),
            ("fractional", (x - 0.3, y + 0.7, w * 0.61 + 0.9, h * 0.83 + 0.45)),
            ("fractional, just under the centres", (x + 0.4999, y + 0.5001, w, h)),
            ("a negative width", (x + 1.0, y, -4.0, h)),
            ("a negative height", (x, y + 1.0, w, -0.5)),
            ("NaN", (np.nan, y, w, h)),
            ("inf", (x, y, np.inf, h)),
            ("-inf", (x, -np.inf, w, h))]


def planted_cases():
    """Every planted mask against every rectangle -> (names, cells [n,6] int32, rle int32, n_rle, regions [n,4])."""
    names, cells, rle, regions = [], [], [], []
    for name, x0, y0, w, h, counts, present in planted_masks():
        first = len(rle)
        rle.extend(counts)
        cell = (x0, y0, w, h, first, len(counts))
        b = M.bounds(cell, rle)
        assert (b is not None) == present, name
        for kind, rect in rectangles_for(b[0] if present else (x0, y0, max(w, 1), max(h, 1)), (x0, y0, max(w, 0), max(h, 0))):
            names.append("%s / %s" % (name, kind))
            cells.append(cell)
            regions.append(rect)
    rle.extend([7, 7, 7])                                            # counts that belong to no mask
    n_rle = len(rle)
    for what, cell in (("first + count > n_rle", (3, 3, 4, 4, n_rle - 2, 3)), ("first < 0", (3, 3, 4, 4, -1, 2)),
                       ("count < 0", (3, 3, 4, 4, 0, -2)), ("first past n_rle", (3, 3, 4, 4, n_rle + 5, 0)),
                       ("first + count overflows 32 bits", (3, 3, 4, 4, 2 ** 31 - 1, 2 ** 31 - 1))):
        assert M.bounds(cell, rle) is None
        for kind, rect in rectangles_for((3, 3, 4, 4), (3, 3, 4, 4))[:3]:
            names.append("%s / %s" % (what, kind))
            cells.append(cell)
            regions.append(rect)
    return names, np.asarray(cells, dtype=np.int32), np.asarray(rle, dtype=np.int32), n_rle, np.asarray(regions, dtype=np.float64)


@pytest.fixture(scope="module")
def planted():
    """The planted cases and their raster restatement, computed once and left unchanged."""
    names, cells, rle, n_rle, regions = planted_cases()
    rects, area = M.bounds_arrays(cells, rle, n_rle)
    overlap = np.stack([M.overlap_counts(p, c, rle, n_rle) for p, c in zip(regions, cells)])
    for a in (cells, rle, regions, rects, area, overlap):
        a.setflags(write=False)
    return {"names": names, "cells": cells, "rle": rle, "n_rle": n_rle, "regions": regions, "rects": rects, "area": area,
            "overlap": overlap}


def run_masks(cuda, cells, rle, n_rle, regions):
    """One ntk_track_mask_bounds and one ntk_track_mask_overlaps over n masks; the outputs have a row more than the entries are
    told of and the inputs are compared with what went up -> (rects [n,4], area [n], overlap [n,3])."""
    from ntmtrack import _lib
    n = len(cells)
    d_cells, d_rle = dev(np.array(cells), cuda, torch.int32), dev(np.array(rle), cuda, torch.int32)       # copies: the fixture's
    d_regions = dev(np.array(regions), cuda)                                                            # arrays are read-only
    d_rects = torch.full((n + 1, 4), SENT, device=cuda, dtype=torch.float64)
    d_area = torch.full((n + 1,), SENT, device=cuda, dtype=torch.float64)
    d_overlap = torch.full((n + 1, 3), SENT, device=cuda, dtype=torch.float64)
    P = _lib.ptr
    _lib.check(_lib.lib().ntk_track_mask_bounds(P(d_cells), P(d_rle), n_rle, n, P(d_rects), P(d_area), _lib.stream()),
               "ntk_track_mask_bounds")
    _lib.check(_lib.lib().ntk_track_mask_overlaps(P(d_regions), P(d_cells), P(d_rle), n_rle, n, P(d_overlap), _lib.stream()),
               "ntk_track_mask_overlaps")
    torch.cuda.synchronize()
    rects, area, overlap = d_rects.cpu().numpy(), d_area.cpu().numpy(), d_overlap.cpu().numpy()
    assert (rects[n] == SENT).all() and area[n] == SENT and (overlap[n] == SENT).all()
    assert same_bits(d_cells.cpu().numpy(), np.ascontiguousarray(cells)) and same_bits(d_rle.cpu().numpy(), np.ascontiguousarray(rle))
    assert same_bits(d_regions.cpu().numpy(), np.ascontiguousarray(regions))
    return rects[:n], area[:n], overlap[:n]


def differing(got, want, names):
    bad = [i for i in range(len(want)) if got[i].tobytes() != want[i].tobytes()]
    return ["%s: got %s, want %s" % (names[i], got[i].tolist(), want[i].tolist()) for i in bad[:8]]


# ------------------------------------------------------------------------------------------- 1. bounds, area and overlaps, bit for bit
def test_the_input_mix_of_the_planted_cases(planted):
    """On the restatement alone: the comparison below cannot pass on an empty case."""
    ov = planted["overlap"]
    present = ~np.isnan(ov[:, 0])
    iou = np.array([M.mask_iou(o) if ok else np.nan for o, ok in zip(ov, present)])
    n = len(ov)
    print("%d cases: %d absent, %d with 0 < IoU < 1, %d with IoU 0, %d with IoU 1" % (
        n, (~present).sum(), ((iou > 0) & (iou < 1)).sum(), (iou == 0).sum(), (iou == 1).sum()))
    assert ((iou > 0) & (iou < 1)).sum() * 4 >= n and (iou == 0).sum() >= 5 and (iou == 1).sum() >= 5
    assert (~present).sum() >= 3 * 18 and np.isnan(planted["rects"][~present]).all() and np.isnan(planted["area"][~present]).all()
    # every value is a whole number, |M n R| <= min(|R|, |M|), and the area is |M|
    assert (ov[present] == np.floor(ov[present])).all() and (ov[present, 0] <= np.minimum(ov[present, 1], ov[present, 2])).all()
    assert same_bits(ov[present, 2], planted["area"][present])


def test_planted_masks_equal_the_raster_restatement_bit_for_bit(cuda, planted):
    rects, area, overlap = run_masks(cuda, planted["cells"], planted["rle"], planted["n_rle"], planted["regions"])
    names = planted["names"]
    assert same_bits(rects, planted["rects"]), differing(rects, planted["rects"], names)
    assert same_bits(area, planted["area"]), differing(area, planted["area"], names)
    assert same_bits(overlap, planted["overlap"]), differing(overlap, planted["overlap"], names)


def random_cases(n, seed):
    """n random masks in a 96 x 64 frame (speckle, blobs and stripes coded by MaskRegions.from_arrays, every fifth one raw random
    counts) against rectangles about their bounds."""
    from ntmtrack.evaluate import MaskRegions
    rng = np.random.default_rng(seed)
    cells, rle, regions = [], [], []
    for i in range(n):
        if i % 5 == 4:
            w, h = int(rng.integers(1, 97)), int(rng.integers(1, 65))
            counts = rng.integers(0, 30, int(rng.integers(2, 150))).tolist()
            x0, y0 = int(rng.integers(-10, 20)), int(rng.integers(-10, 20))
        else:
            m = np.zeros((H, W), dtype=bool)
            y, x = np.mgrid[:H, :W]
            cy, cx, ry, rx = rng.uniform(10, 54), rng.uniform(10, 86), rng.uniform(1, 25), rng.uniform(1, 35)
            m |= ((y + 0.5 - cy) / ry) ** 2 + ((x + 0.5 - cx) / rx) ** 2 <= 1
            if i % 5 == 1:
                m &= rng.random((H, W)) < 0.5
            if i % 5 == 2:
                m[:, ::3] = False
            x0, y0, w, h, counts = MaskRegions.from_arrays(m[None]).frame(0)
            counts = counts.tolist()
        cell = (x0, y0, w, h, len(rle), len(counts))
        rle.extend(counts)
        b = M.bounds(cell, rle)
        b = (x0, y0, w, h) if b is None else b[0]
        pw, ph = b[2] * rng.uniform(0.5, 1.4), b[3] * rng.uniform(0.5, 1.4)
        regions.append((b[0] + rng.uniform(-0.3, 0.5) * b[2], b[1] + rng.uniform(-0.3, 0.5) * b[3], pw, ph))
        cells.append(cell)
    return np.asarray(cells, dtype=np.int32), np.asarray(rle, dtype=np.int32), np.asarray(regions, dtype=np.float64)


@pytest.mark.parametrize("n", [1, 3, 64, 65])
def test_random_masks_equal_the_raster_restatement_bit_for_bit(cuda, n):
    cells, rle, regions = random_cases(n, 500 + n)
    w_rects, w_area = M.bounds_arrays(cells, rle)
    w_overlap = np.stack([M.overlap_counts(p, c, rle) for p, c in zip(regions, cells)])
    iou = np.array([M.mask_iou(o) for o in w_overlap if not np.isnan(o[0])])
    assert len(iou) >= n - n // 8 and ((iou > 0) & (iou < 1)).sum() * 2 >= n
    rects, area, overlap = run_masks(cuda, cells, rle, len(rle), regions)
    names = ["mask %d" % i for i in range(n)]
    assert same_bits(rects, w_rects), differing(rects, w_rects, names)
    assert same_bits(area, w_area), differing(area, w_area, names)
    assert same_bits(overlap, w_overlap), differing(overlap, w_overlap, names)


# ------------------------------------------------------------------------------------------------------------------ 2. the table
def mask_round(cuda, cells, rle):
    """cells [T,B,6] (``first`` into rle) -> evaluate.MaskRound [T,B] through evaluate.upload_masks (one block: the T B masks in a
    row, then seen as [T,B])."""
    from ntmtrack import evaluate as E
    T, B = cells.shape[:2]
    flat = E.upload_masks([((), np.ascontiguousarray(cells, dtype=np.int32).reshape(-1, 6), np.asarray(rle, dtype=np.int32))], (T * B,), cuda)
    return E.MaskRound(flat.cells.view(T, B, 6), flat.rle, flat.n_rle, flat.rects.view(T, B, 4), flat.area.view(T, B))


def run_scores(cuda, pred, rnd, clip_of, n_clips, active=None, table=None):
    """OverlapScores.add with a MaskRound -> (table, frame_iou, the scores object)."""
    from ntmtrack import evaluate as E
    s = table if table is not None else E.OverlapScores(n_clips, device=cuda)
    fi = s.add(dev(np.ascontiguousarray(pred), cuda), rnd, torch.tensor(clip_of, dtype=torch.int32, device=cuda),
               None if active is None else dev(np.ascontiguousarray(active), cuda, torch.uint8), frame_iou=True)
    torch.cuda.synchronize()
    return s.table.cpu().numpy(), fi.cpu().numpy(), s


def assert_mask_table(got, want, what):
    """Every count and SUM_IOU exact; SUM_DIST within DIST_ATOL per scored frame of the row."""
    exact = [c for c in range(want.shape[1]) if c != U.SUM_DIST]
    e_dist = np.abs(got[:, U.SUM_DIST] - want[:, U.SUM_DIST]) / np.maximum(want[:, U.FRAMES], 1)
    print("%s: max |SUM_IOU err| %.3g, max |SUM_DIST err| per frame %.3g px" % (
        what, np.abs(got[:, U.SUM_IOU] - want[:, U.SUM_IOU]).max(), e_dist.max()))
    np.testing.assert_array_equal(got[:, exact], want[:, exact])
    assert e_dist.max() <= DIST_ATOL


TABLE_T = 4


def w_dists_to_thresholds(d):
    return d[:, None] - TE.DIST_THR[None] if len(d) else np.ones((1, 1))


def table_data(B, seed=77):
    """-> (pred [T,B,4], cells [T,B,6], rle, active [T,B]): random masks against rectangles about their bounds, every fourth far
    away; with B >= 3 an inactive frame, an absent mask, a prediction that is not finite and one of negative width."""
    cells, rle, pred = random_cases(TABLE_T * B, seed + B)
    cells, pred = cells.reshape(TABLE_T, B, 6).copy(), pred.reshape(TABLE_T, B, 4).copy()
    pred[1::4, :, 0] += 300.0
    active = np.ones((TABLE_T, B), dtype=np.uint8)
    if B >= 3:
        active[1, 2] = 0
        cells[2, 0, 2] = 0                                           # w = 0: an absent object
        pred[0, 1, 0], pred[3, 2, 2] = np.nan, -7.0
    return pred, cells, rle, active


@pytest.mark.parametrize("B", [1, 3, 64, 65])
def test_scores_match_the_restated_table(cuda, B):
    pred, cells, rle, active = table_data(B)
    n_clips = B + 1
    clip_of = [B - b for b in range(B)]                              # rows B .. 1; row 0 belongs to nobody
    want = U.new_table(n_clips, 21, 51)
    w_iou, w_dist = M.accumulate_mask(want, pred, cells, rle, clip_of, TE.IOU_THR, TE.DIST_THR, active)
    scored = ~np.isnan(w_iou)
    finite = scored & np.isfinite(w_dist)
    assert np.abs(w_dists_to_thresholds(w_dist[finite])).min() >= 1e-9            # no precision count hinges on a last bit
    assert (w_iou[scored] > 0).sum() * 3 >= scored.sum() and (w_iou[scored] == 0).sum() >= 1
    rnd = mask_round(cuda, cells, rle)
    got, g_iou, _s = run_scores(cuda, pred, rnd, clip_of, n_clips, active)
    assert_mask_table(got, want, "B = %d: kernel against the restatement" % B)
    assert same_bits(g_iou, w_iou), np.argwhere(~((g_iou == w_iou) | (np.isnan(g_iou) & np.isnan(w_iou)))).tolist()[:8]
    if B >= 3:
        assert (~scored).sum() == 2 and g_iou[0, 1] == 0.0 and g_iou[3, 2] == 0.0
    assert (got[0] == U.new_table(1, 21, 51)[0]).all()
    # the round's bounds and areas are the restated ones
    w_rects, w_area = M.bounds_arrays(cells, rle)
    assert same_bits(rnd.rects.cpu().numpy(), w_rects) and same_bits(rnd.area.cpu().numpy(), w_area)


def test_a_filled_integer_rectangle_as_a_mask_leaves_the_rectangle_entrys_bits(cuda):
    rng = np.random.default_rng(9)
    T, B = 3, 65
    boxes = np.concatenate([rng.integers(0, 50, (T, B, 1)), rng.integers(0, 30, (T, B, 1)), rng.integers(1, 41, (T, B, 1)),
                            rng.integers(1, 31, (T, B, 1))], axis=2)
    pred = (boxes + rng.integers(-12, 13, (T, B, 4))).astype(np.float64)
    pred[..., 2:] = np.maximum(pred[..., 2:], 1.0)
    pred[0, :5] = boxes[0, :5]                                       # five boxes against themselves: exactly 1
    pred[1, :5, 0] = boxes[1, :5, 0] + boxes[1, :5, 2]               # five that touch: exactly 0
    cells = np.zeros((T, B, 6), dtype=np.int32)
    cells[..., :4] = boxes
    cells[..., 4] = 2 * np.arange(T * B).reshape(T, B)
    cells[..., 5] = 2
    rle = np.stack([np.zeros(T * B, dtype=np.int64), (boxes[..., 2] * boxes[..., 3]).reshape(-1)], axis=1).reshape(-1)
    clip_of = list(range(B))
    by_rect, rect_iou, _s = TE.run_kernel(cuda, pred, boxes.astype(np.float64), clip_of, B)
    by_mask, mask_iou, _s = run_scores(cuda, pred, mask_round(cuda, cells, rle), clip_of, B)
    assert ((rect_iou > 0) & (rect_iou < 1)).sum() >= 50 and (rect_iou == 0).sum() >= 5 and (rect_iou == 1).sum() >= 5
    assert same_bits(mask_iou, rect_iou), "differ at %s" % np.argwhere(mask_iou != rect_iou).tolist()[:8]
    assert same_bits(by_mask, by_rect)


def test_one_frame_calls_leave_the_bits_of_one_call(cuda):
    B = 3
    pred, cells, rle, active = table_data(B)
    clip_of = [3, 0, 1]
    rnd = mask_round(cuda, cells, rle)
    whole, whole_iou, _s = run_scores(cuda, pred, rnd, clip_of, B + 1, active)
    s, ious = None, []
    for t in range(TABLE_T):
        one, iou, s = run_scores(cuda, pred[t], rnd[t], clip_of, B + 1, active[t], table=s)         # the [B,4] form of add
        ious.append(iou[0])
    assert same_bits(one, whole) and same_bits(np.stack(ious), whole_iou) and whole[:, U.FRAMES].sum() == TABLE_T * B - 2


# -------------------------------------------------------------------------------------------------------------- 3. supervise
SUP_T, SUP_B, SUP_CLIPS = 6, 3, 5
SUP_CLIP_OF = [3, 0, 4]


def blob(cx, cy, rx, ry):
    y, x = np.mgrid[:H, :W]
    return ((y + 0.5 - cy) / ry) ** 2 + ((x + 0.5 - cx) / rx) ** 2 <= 1


def supervise_data():
    """Blobs that drift; a prediction is the blob's bounds with a little noise, moved 60 px away where a failure is planted.
    Slot 1 never fails."""
    from ntmtrack.evaluate import MaskRegions
    rng = np.random.default_rng(12)
    frames, pred = [], np.zeros((SUP_T, SUP_B, 4))
    centre, size = rng.uniform(25, 40, (SUP_B, 2)), rng.uniform(6, 14, (SUP_B, 2))
    for t in range(SUP_T):
        for b in range(SUP_B):
            frames.append(blob(centre[b, 0] + 2.0 * t, centre[b, 1] - 1.5 * t, size[b, 0], size[b, 1]))
    regions = MaskRegions.from_arrays(np.stack(frames))
    cells, rle = regions.cells(0, SUP_T * SUP_B)
    cells = cells.reshape(SUP_T, SUP_B, 6).copy()
    rects, _a = M.bounds_arrays(cells, rle)
    pred[:] = rects + rng.standard_normal((SUP_T, SUP_B, 4)) * 1.2
    for t, b in ((1, 0), (4, 0), (0, 2)):
        pred[t, b, 0] += 60.0
    cells[1, 2, 3] = cells[2, 2, 3] = 0 # slot 2 failed on 0: with skip 1 and with skip 2 its restart frame has no object
    cells[3, 1, 2] = 0                  # an absent object while tracking
    pred[5, 2, 1] = np.inf              # a prediction that is not finite: overlap 0, a failure
    active = np.ones((SUP_T, SUP_B), dtype=np.uint8)
    active[2, 1] = 0
    return pred, cells, rle, active


@pytest.mark.parametrize("skip,burn_in", [(1, 0), (2, 1)])
def test_supervise_matches_the_restated_walk(cuda, skip, burn_in):
    from ntmtrack import evaluate as E
    pred, cells, rle, active = supervise_data()
    w_codes, w_iou, w_table, w_state, _r = M.walk_mask(pred, cells, rle, SUP_CLIP_OF, SUP_CLIPS, active, skip=skip, burn_in=burn_in)
    judged = ~np.isnan(w_iou)
    print("skip %d burn_in %d: codes per slot %s" % (skip, burn_in, w_codes.T.tolist()))
    assert w_table[:, S.FAILURES].sum() >= 3 and w_table[:, S.RESTARTS].sum() >= 2 and w_table[SUP_CLIP_OF[1], S.FAILURES] == 0
    assert (w_codes[:, 2] == S.SKIP).sum() > skip - 1               # the restart that had no object slipped
    assert w_table[:, S.VALID].sum() >= 3 and ((w_iou[judged] == 0) | (w_iou[judged] > 0.05)).all()

    sup = E.Supervisor(SUP_B, SUP_CLIPS, skip=skip, burn_in=burn_in, device=cuda)
    rnd = mask_round(cuda, cells, rle)
    d_pred, d_act = dev(pred, cuda), dev(active, cuda, torch.uint8)
    d_clip = dev(np.asarray(SUP_CLIP_OF), cuda, torch.int32)
    codes = torch.zeros((SUP_T, SUP_B), dtype=torch.int8, device=cuda)
    ious = torch.zeros((SUP_T, SUP_B), dtype=torch.float64, device=cuda)
    for t in range(SUP_T):
        frame = rnd[t]
        sup.plan(frame, d_act[t], d_clip, codes=codes[t], frame_iou=ious[t])
        frame.overlaps(d_pred[t])
        sup.judge(d_pred[t], frame, d_clip, codes=codes[t], frame_iou=ious[t])
    torch.cuda.synchronize()
    codes, ious, table, state = codes.cpu().numpy(), ious.cpu().numpy(), sup.table.cpu().numpy(), sup.state.cpu().numpy()
    np.testing.assert_array_equal(codes, w_codes)
    np.testing.assert_array_equal(state, w_state)
    assert same_bits(ious, w_iou)
    assert same_bits(table, w_table), (table.tolist(), w_table.tolist())
    for row in (1, 2):                                               # rows no slot named stay as the owner made them
        assert (table[row] == S.new_table(1)[0]).all()


# ---------------------------------------------------------------------------------------------------- 4. through the trackers
SKIP, BURN_IN = TS.SKIP, TS.BURN_IN
LENGTHS = [9, 4, 6, 4, 7]
CLIP_SEED = 36


def mask_clips(seed=CLIP_SEED):
    """Five clips of 64 x 96 on the model of tests/test_supervised_gpu.py's: the object is a blob inscribed in a box; clips 0 and 2
    carry planted failures (the box, about a tenth of the frame wide, jumps three box widths along x: the box update moves a box
    by less than 8/6 of its side per frame, so the prediction cannot overlap the ground truth on that frame, whatever the weights
    are), the others drift a few pixels per frame; clip 4 has an absent object."""
    from ntmtrack.evaluate import Clip, MaskRegions
    drifting = TE.make_clips(seed, LENGTHS, H, W)
    rng = np.random.default_rng(seed + 1)

    def planted(n, jumps):
        box = np.array([8.0, 28.0, 10.0, 8.0])
        regions = np.tile(box, (n, 1)) + np.cumsum(rng.uniform(-0.25, 0.25, size=(n, 4)), axis=0)
        for frame, widths in jumps:
            regions[frame:, 0] += widths * 10.0
        return regions
    boxes = [np.asarray(c.regions) for c in drifting]
    boxes[0], boxes[2] = planted(LENGTHS[0], [(1, 3), (4, 3)]), planted(LENGTHS[2], [(1, 3)])
    clips = []
    for i, (c, b) in enumerate(zip(drifting, boxes)):
        masks = np.stack([blob(r[0] + r[2] / 2, r[1] + r[3] / 2, r[2] / 2, r[3] / 2) for r in b])
        if i == 4:
            masks[3] = False
        clips.append(Clip(c.frames, MaskRegions.from_arrays(masks)))
    return clips


def clip_frames(clip):
    return [clip.regions.frame(i) for i in range(len(clip.regions))]


def raster_bounds(clip, i):
    cells, counts = clip.regions.cells(i, i + 1)
    b = M.bounds(cells[0], counts)
    return None if b is None else b[0]


def assert_starts(seen, clips):
    """Clips are handed out in index order: the start regions, in the order they were given, are the raster bounds of the clips'
    first masks, bit for bit."""
    starts = np.concatenate(seen)
    assert same_bits(starts, np.stack([raster_bounds(c, 0) for c in clips]))


recording, family_maker, CountingLib = TP.recording, TP.family_maker, TP.CountingLib


@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_validate_one_pass_over_mask_clips(world, cuda, family):                                    # noqa: F811
    from ntmtrack import evaluate as E
    clips, cores, seen = mask_clips(), [], []
    v = E.Validation(recording(family_maker(family, world, cuda, cores), seen), clips, 2, 2, return_regions=True, device=cuda).finish()
    assert v.masks and not v.polygons and v.supervisor is None
    assert_starts(seen, clips)
    regions = v.regions()
    assert all(np.isfinite(r).all() and r.shape == (len(c.regions) - 1, 4) for r, c in zip(regions, clips))
    want = M.score_clips_mask(regions, [clip_frames(c) for c in clips], TE.IOU_THR, TE.DIST_THR)    # rows in the caller's clip order
    assert want[:, U.FRAMES].tolist() == [8, 3, 5, 3, 5] and want[:, U.SUM_IOU].sum() > 0 and want[:, U.LOST].sum() >= 2
    assert_mask_table(v.scores.table.cpu().numpy(), want, "%s: one pass over mask clips, replayed" % family)


def replay_supervised(regions, codes, clips, table):
    """The device's regions and codes through the host restatement, clip by clip -> the replayed table [n_clips, HEAD]."""
    rows = []
    for i, c in enumerate(clips):
        cells, rle = M.clip_masks(clip_frames(c))
        w_codes, w_iou, w_table, _state, w_restart = M.walk_mask(regions[i][:, None], cells, rle, [0], 1, skip=SKIP, burn_in=BURN_IN)
        assert codes[i].tolist() == w_codes[:, 0].tolist(), "clip %d" % i
        assert (np.isnan(regions[i]).all(axis=1) == (w_codes[:, 0] == S.SKIP)).all() and np.isfinite(regions[i][w_codes[:, 0] != S.SKIP]).all()
        for t in np.nonzero(w_restart[:, 0])[0]:                     # a restart starts from the mask's bounds
            assert same_bits(regions[i][t], raster_bounds(c, t + 1)), "clip %d frame %d" % (i, t + 1)
        assert same_bits(table[i], w_table[0]), "clip %d: %s, replayed %s" % (i, table[i].tolist(), w_table[0].tolist())
        rows.append(w_table[0])
    return np.stack(rows)


@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_validate_supervised_over_mask_clips(world, cuda, family):                                  # noqa: F811
    from ntmtrack import evaluate as E
    clips, cores, seen = mask_clips(), [], []
    v = E.Validation(recording(family_maker(family, world, cuda, cores), seen), clips, 2, 2, return_regions=True, device=cuda,
                     protocol="supervised", skip=SKIP, burn_in=BURN_IN).finish()
    if family == "dnc":
        TE.assert_one_workgroup_family(cores)
    assert_starts(seen, clips)
    regions, codes, table = v.regions(), v.codes(), v.supervisor.table.cpu().numpy()
    want = replay_supervised(regions, codes, clips, table)
    print("%s: replayed codes %s" % (family, [c.tolist() for c in codes]))
    assert want[:, S.FAILURES].sum() >= 2 and want[:, S.RESTARTS].sum() >= 2 and want[:, S.VALID].sum() > 0
    res = v.supervisor.result()
    assert res["failures"] == int(want[:, S.FAILURES].sum()) and res["restarts"] == int(want[:, S.RESTARTS].sum())


@pytest.mark.parametrize("family", ["ntm", "dnc"])
@pytest.mark.parametrize("protocol", ["one_pass", "supervised"])
def test_mask_rounds_after_the_first_do_not_synchronise(world, cuda, family, protocol):             # noqa: F811
    from ntmtrack import evaluate as E
    cores = []
    v = E.Validation(family_maker(family, world, cuda, cores), mask_clips(), 2, 2, device=cuda, protocol=protocol, skip=SKIP,
                     burn_in=BURN_IN)
    assert v.masks and v.step()                                     # builds the tracker, its plans and workspaces
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    rounds = 0
    try:
        while v.step():
            rounds += 1
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert rounds >= 4
    if family == "dnc":
        TE.assert_one_workgroup_family(cores)
    v.finish()
    if protocol == "supervised":
        res = v.supervisor.result()
        assert res["failures"] >= 2 and res["restarts"] >= 2      # the planted failures ran inside the unsynchronised rounds
    else:
        assert v.scores.result()["frames"] == 24


# ------------------------------------------------------------------------------------------------------- 5. unchanged path
def mask_entries(calls):
    """The entries of this feature (ntk_track_decode_mask, which masks FRAMES of file clips, is not one of them)."""
    return sorted(name for name in calls if "_mask" in name and name != "ntk_track_decode_mask")


def test_rectangle_clips_make_no_mask_call(world, cuda, monkeypatch):                               # noqa: F811
    from ntmtrack import _lib, evaluate as E
    rect_clips = TE.make_clips(CLIP_SEED, LENGTHS, H, W)
    maker = TE.ntm_maker(world, cuda)
    lib = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    E.Validation(maker, rect_clips, 2, 2, device=cuda).finish()
    assert mask_entries(lib.calls) == [] and lib.calls["ntk_track_overlap_scores"] >= 4
    lib.calls.clear()
    E.Validation(maker, rect_clips, 2, 2, device=cuda, protocol="supervised", skip=SKIP, burn_in=BURN_IN).finish()
    assert mask_entries(lib.calls) == [] and lib.calls["ntk_track_supervise"] >= 8
    # the wrapper does see the mask calls when there are some: per round one bounds, one overlaps and one scoring launch ...
    lib.calls.clear()
    v = E.Validation(maker, mask_clips(), 2, 2, device=cuda).finish()
    rounds = lib.calls["ntk_track_mask_bounds"]
    assert rounds >= 5 and mask_entries(lib.calls) == ["ntk_track_mask_bounds", "ntk_track_mask_overlaps", "ntk_track_overlap_scores_mask"]
    assert lib.calls["ntk_track_mask_overlaps"] == rounds and lib.calls["ntk_track_overlap_scores_mask"] == rounds
    assert lib.calls["ntk_track_overlap_scores"] == 0 and v.scores.result()["frames"] == 24
    # ... and in the supervised protocol one bounds launch per round, one overlaps launch and two phases per frame
    lib.calls.clear()
    E.Validation(maker, mask_clips(), 2, 2, device=cuda, protocol="supervised", skip=SKIP, burn_in=BURN_IN).finish()
    assert lib.calls["ntk_track_mask_bounds"] == rounds and lib.calls["ntk_track_mask_overlaps"] == 2 * rounds
    assert lib.calls["ntk_track_supervise_mask"] == 4 * rounds and lib.calls["ntk_track_supervise"] == 0


# ------------------------------------------------------------------------------------------------- 6. a VOT directory, end to end
def test_validate_supervised_on_a_vot_mask_directory(world, cuda, tmp_path):                        # noqa: F811
    """data.vot_clips -> evaluate.validate(protocol="supervised") -> evaluate.write_trajectory on a tree written here: two sequences
    whose groundtruth.txt holds ``m`` lines (one with an absent object), JPEG frames decoded when scheduled."""
    from ntmtrack import data, evaluate as E
    from test_masks_host import write_mask_directory
    rng = np.random.default_rng(4)
    source = mask_clips()
    for name, sub, clip in (("a", "color", source[2]), ("b", "", source[4])):
        write_mask_directory(str(tmp_path), name, clip.regions, rng.integers(0, 256, size=(len(clip.regions), H, W, 3), dtype=np.uint8), sub)
    with open(os.path.join(str(tmp_path), "list.txt"), "w") as f:
        f.write("a\nb\n")
    clips = data.vot_clips(str(tmp_path))
    assert all(isinstance(c.regions, E.MaskRegions) and c.size == (H, W) for c in clips) and [len(c.regions) for c in clips] == [6, 7]
    assert np.isnan(E.mask_bounds(clips[1].regions, 3)).all()
    res, regions, codes = E.validate(TE.ntm_maker(world, cuda), clips, 2, 2, return_regions=True, device=cuda, protocol="supervised",
                                     skip=SKIP, burn_in=BURN_IN)
    table = np.zeros((2, S.HEAD))
    for k, col in (("valid", S.VALID), ("failures", S.FAILURES), ("restarts", S.RESTARTS), ("tracked", S.TRACKED), ("skipped", S.SKIPPED),
                   ("first_failure", S.FIRST_FAILURE)):
        table[:, col] = res["clips"][k]
    want = []
    for i, c in enumerate(clips):                                    # the result holds the accuracy, not the sum: the counts exactly
        cells, rle = M.clip_masks(clip_frames(c))
        w_codes, _iou, w_table, _state, _r = M.walk_mask(regions[i][:, None], cells, rle, [0], 1, skip=SKIP, burn_in=BURN_IN)
        assert codes[i].tolist() == w_codes[:, 0].tolist()
        exact = [k for k in range(S.HEAD) if k != S.SUM_IOU]
        np.testing.assert_array_equal(table[i, exact], w_table[0, exact])
        if w_table[0, S.VALID] > 0:
            assert res["clips"]["accuracy"][i] == w_table[0, S.SUM_IOU] / w_table[0, S.VALID]
        want.append(w_table[0])
    want = np.stack(want)
    assert want[0, S.FAILURES] >= 1 and want[0, S.RESTARTS] >= 1 and res["tracked"] >= 2
    assert res["tracked"] + res["skipped"] + res["restarts"] in (10, 11)     # every frame but, where it was tracked, the absent one
    for i, c in enumerate(clips):
        path = str(tmp_path / ("%s_001.txt" % "ab"[i]))
        E.write_trajectory(path, E.mask_bounds(c.regions, 0), regions[i], codes[i])
        lines = open(path).read().splitlines()
        assert len(lines) == len(c.regions) and lines[0] == "1"
        assert all((line in ("0", "1", "2")) == (code != S.TRACKED_CODE) for line, code in zip(lines[1:], codes[i]))


def test_a_mask_clip_beside_a_rectangle_clip_is_refused(world, cuda):                               # noqa: F811
    from ntmtrack import evaluate as E
    clips = [mask_clips()[1], TE.make_clips(CLIP_SEED, LENGTHS, H, W)[3]]
    with pytest.raises(ValueError, match=r"clips \[0\] have mask regions and clips \[1\] have not"):
        E.Validation(TE.ntm_maker(world, cuda), clips, 2, 2, device=cuda)
