"""GPU: polygon ground truth on the device -- ntk_track_poly_bounds, ntk_track_overlap_scores_poly and ntk_track_supervise_poly
against the NumPy restatement of their rules (tests/poly_util.py), the values the header pins, and evaluate.Validation over
polygon clips in both protocols, replayed on the host from the regions and codes the device returned.

Model shapes, world, makers and frame size: those of tests/test_evaluate_gpu.py; the clips: tests/test_supervised_gpu.py's, with
every ground-truth box turned by 20 degrees about its centre."""
import collections

import numpy as np
import pytest
import torch

import evaluate_util as U
import poly_util as P
import supervised_util as S
import test_evaluate_gpu as TE
import test_supervised_gpu as TS
from test_evaluate_gpu import world                                  # noqa: F401  (the module-scoped fixture: cell, trunk, clips)

pytestmark = pytest.mark.gpu

# Two float64 evaluations of the same overlap by different routes (clipping against splitting every edge) differ by 4.4e-16 on
# 23 000 random polygons on the CPU; 1e-12 per frame leaves four decades for the order of operations and the absence of FMA.
ATOL = 1e-12
same_bits = TE.same_bits
dev = TS.dev
L_SHAPE = [(0, 0), (40, 0), (40, 10), (10, 10), (10, 40), (0, 40)]


def flat(points):
    return np.asarray(points, dtype=np.float64).reshape(-1)


def random_polygon(rng, i):
    """A region by its index: rotated rectangles, 3- to 8-gons about a centre (simple: the angles go once round), the L-shape moved
    and scaled; every other one in the opposite orientation."""
    cx, cy = rng.uniform(60, 300, 2)
    kind = i % 3
    if kind == 0:
        pts = P.rotated_rect(cx, cy, rng.uniform(10, 120), rng.uniform(10, 120), rng.uniform(0, np.pi))
    elif kind == 1:
        k = (3, 8, 4, 5, 6, 7)[(i // 3) % 6]
        ang = 2 * np.pi * (np.arange(k) + rng.uniform(0, 0.8, k)) / k
        rad = rng.uniform(15, 90, k)
        pts = [(cx + r * np.cos(a), cy + r * np.sin(a)) for r, a in zip(rad, ang)]
    else:
        s = rng.uniform(0.5, 2.0)
        pts = [(cx + s * (x - 20), cy + s * (y - 20)) for x, y in L_SHAPE]
    return P.pad(pts[::-1] if (i // 2) % 2 else pts)


# ---------------------------------------------------------------------------------------------------------------- 1. bounds
ABSENT = {"two vertices": P.pad([(3.0, 4.0), (50.0, 60.0)]),
          "collinear": P.pad([(0.0, 0.0), (10.0, 10.0), (20.0, 20.0), (35.0, 35.0)]),
          "first pair NaN": np.concatenate([[np.nan], flat(P.rotated_rect(50, 50, 20, 10, 0.3))[1:], [np.nan] * 8])}
SENT = -777.25


def run_bounds(cuda, polys):
    from ntmtrack import _lib
    n = len(polys)
    d_poly = dev(polys, cuda)
    d_rects = torch.full((n + 1, 4), SENT, device=cuda, dtype=torch.float64)      # one row more than the kernel is told of
    _lib.check(_lib.lib().ntk_track_poly_bounds(_lib.ptr(d_poly), n, _lib.ptr(d_rects), _lib.stream()), "ntk_track_poly_bounds")
    torch.cuda.synchronize()
    out = d_rects.cpu().numpy()
    assert (out[n] == SENT).all()
    return out[:n]


@pytest.mark.parametrize("n", [1, 5, 70])
def test_bounds_equal_the_restatement_bit_for_bit(cuda, n):
    rng = np.random.default_rng(200 + n)
    polys = np.stack([random_polygon(rng, i) for i in range(n)])
    polys[::4, :] -= 400.0                                           # every fourth region has all its coordinates negative
    absent_at = {1: [], 5: [1, 2, 3], 70: [1, 2, 3, 63, 64, 69]}[n]
    for j, i in enumerate(absent_at):
        polys[i] = list(ABSENT.values())[j % 3]
    want = P.bounds_array(polys)
    counts = collections.Counter(len(P.vertices(g)) for g in polys)
    assert counts[4] and (n < 5 or counts[8]) and (n < 70 or counts[3])
    assert np.isnan(want[absent_at]).all() and np.isfinite(np.delete(want, absent_at, 0)).all()
    assert (want[0, 0] + want[0, 2] < 0) and (want[0, 1] + want[0, 3] < 0)     # where the reference's seed of the maximum is wrong
    got = run_bounds(cuda, polys)
    assert same_bits(got, want), "differ in rows %s" % np.nonzero((got != want).any(axis=1) & ~np.isnan(want).all(axis=1))[0].tolist()


@pytest.mark.parametrize("kind", sorted(ABSENT))
def test_bounds_of_an_absent_region_are_nan(cuda, kind):
    assert P.bounds(ABSENT[kind]) is None
    assert np.isnan(run_bounds(cuda, ABSENT[kind][None])).all()


# --------------------------------------------------------------------------------------------------------------- 2. overlap
T = 3
OVERLAP_SEED = 31


def overlap_data(B, seed=OVERLAP_SEED):
    """-> (pred [T,B,4], gt [T,B,16], active [T,B], planted [T,B]).  A prediction is a rectangle about the polygon's bounding
    rectangle, moved and resized; every fourth one lies 400 px away.  With B >= 5: an inactive frame, two absent objects, two
    predictions that are not finite and one of negative width (``planted``: their overlap is 0 by rule, not by geometry)."""
    rng = np.random.default_rng(seed + B)
    gt, pred = np.full((T, B, 16), np.nan), np.zeros((T, B, 4))
    for t in range(T):
        for b in range(B):
            i = t * B + b
            gt[t, b] = random_polygon(rng, i)
            x, y, w, h = P.bounds(gt[t, b])
            pw, ph = w * rng.uniform(0.7, 1.3), h * rng.uniform(0.7, 1.3)
            cx, cy = x + w / 2 + rng.uniform(-0.25, 0.25) * w, y + h / 2 + rng.uniform(-0.25, 0.25) * h
            if i % 4 == 1:
                cx += 400.0
            pred[t, b] = (cx - pw / 2, cy - ph / 2, pw, ph)
    active, planted = np.ones((T, B), dtype=np.uint8), np.zeros((T, B), dtype=bool)
    if B >= 5:
        active[1, 2] = 0
        gt[2, 0], gt[0, 3] = ABSENT["two vertices"], ABSENT["first pair NaN"]
        pred[1, 1, 0], pred[0, 4, 1], pred[2, 4, 2] = np.nan, np.inf, -7.0
        planted[1, 1] = planted[0, 4] = planted[2, 4] = True
    return pred, gt, active, planted


def check_overlap_inputs(pred, gt, planted, ious, dists):
    """The conditions on the inputs, on the restatement alone: no count may hinge on a last bit, and the comparison may not pass
    on an empty case."""
    scored = ~np.isnan(ious)
    for t, b in zip(*np.nonzero(scored & ~planted)):
        if ious[t, b] == 0:
            p, g = pred[t, b], P.bounds(gt[t, b])
            gap = max(max(p[0], g[0]) - min(p[0] + p[2], g[0] + g[2]), max(p[1], g[1]) - min(p[1] + p[3], g[1] + g[3]))
            assert gap > 1.0, "frame (%d, %d): overlap 0 with a gap of %.3g px between the bounding rectangles" % (t, b, gap)
        else:
            assert np.abs(ious[t, b] - TE.IOU_THR).min() >= 1e-6, "frame (%d, %d): overlap %.17g" % (t, b, ious[t, b])
    finite = scored & np.isfinite(dists)
    assert np.abs(dists[finite][:, None] - TE.DIST_THR[None]).min() >= 1e-9
    assert (ious[scored] > 0).sum() * 3 >= scored.sum() and (ious[scored & ~planted] == 0).sum() >= 1


def assert_poly_table(got, want, what):
    """Every count exact; SUM_IOU and SUM_DIST within ATOL per scored frame of the row."""
    sums = [U.SUM_IOU, U.SUM_DIST]
    exact = [c for c in range(want.shape[1]) if c not in sums]
    np.testing.assert_array_equal(got[:, exact], want[:, exact])
    frames = np.maximum(want[:, U.FRAMES], 1)
    e_iou, e_dist = np.abs(got[:, U.SUM_IOU] - want[:, U.SUM_IOU]) / frames, np.abs(got[:, U.SUM_DIST] - want[:, U.SUM_DIST]) / frames
    print("%s: max |SUM_IOU err| per frame %.3g, max |SUM_DIST err| per frame %.3g px" % (what, e_iou.max(), e_dist.max()))
    assert e_iou.max() <= ATOL and e_dist.max() <= ATOL


@pytest.mark.parametrize("B", [1, 5, 70])
def test_overlap_matches_the_restatement(cuda, B):
    pred, gt, active, planted = overlap_data(B)
    n_clips = B + 1
    clip_of = [B - b for b in range(B)]                              # rows B .. 1; row 0 belongs to nobody
    want = U.new_table(n_clips, 21, 51)
    w_iou, w_dist = P.accumulate_poly(want, pred, gt, clip_of, TE.IOU_THR, TE.DIST_THR, active)
    check_overlap_inputs(pred, gt, planted, w_iou, w_dist)
    got, g_iou, _s = TE.run_kernel(cuda, pred, gt, clip_of, n_clips, active)
    assert_poly_table(got, want, "B = %d: kernel against the restatement" % B)
    unscored = np.isnan(w_iou)
    assert (np.isnan(g_iou) == unscored).all()
    if B >= 5:
        assert unscored.sum() == 3 and g_iou[1, 1] == 0.0 and g_iou[0, 4] == 0.0 and g_iou[2, 4] == 0.0
    e = np.abs(g_iou - w_iou)[~unscored].max()
    print("B = %d: frame_iou: max |err| %.3g over %d frames, %d of them with overlap 0" % (B, e, (~unscored).sum(), (w_iou == 0).sum()))
    assert e <= ATOL
    assert same_bits(g_iou == 0, w_iou == 0)                         # the exact zeros are exact on both sides
    assert (got[0] == U.new_table(1, 21, 51)[0]).all()


# ------------------------------------------------------------------------------------------------- 3. the pinned exact values
def one_frame(cuda, pred, gt):
    """B frames in one call, one clip each -> frame_iou [B]."""
    B = len(pred)
    _t, iou, _s = TE.run_kernel(cuda, np.asarray(pred, dtype=np.float64)[None], np.asarray(gt, dtype=np.float64)[None], list(range(B)), B)
    return iou[0]


def test_pinned_exact_values(cuda):
    box = (20.0, 31.0, 40.0, 17.0)
    diamond = P.pad([(42.0, -12.0), (62.0, 8.0), (82.0, -12.0), (62.0, -32.0)])
    cases = [(box, P.pad(P.rect_points(box)), 1.0),                                          # an integer 4-gon against itself
             (box, P.pad(P.rect_points(box)[::-1]), 1.0),                                    # and in the other orientation
             ((20.0, 60.0, 30.0, 20.0), P.pad(P.rect_points((50.0, 60.0, 30.0, 20.0))), 0.0),  # touching along x = 50
             ((60.0, 40.0, 10.0, 20.0), P.pad(P.rect_points((50.0, 60.0, 30.0, 20.0))), 0.0),  # touching along y = 60
             ((20.0, 40.0, 30.0, 20.0), P.pad(P.rect_points((50.0, 60.0, 30.0, 20.0))), 0.0),  # touching in a corner
             ((50.0, 0.0, 30.0, 30.0), P.pad([(50.0, 10.0), (30.0, 20.0), (30.0, 0.0)]), 0.0),  # a triangle's vertex on a side
             ((0.0, 0.0, 50.0, 50.0), diamond, 0.0),                  # a turned square by the corner (50, 0): bounding boxes overlap
             ((15.0, 15.0, 20.0, 20.0), P.pad(L_SHAPE), 0.0),         # the rectangle in the L's notch
             ((5.0, 5.0, 30.0, 30.0), P.pad(L_SHAPE), 275.0 / 1325.0),
             ((0.0, 0.0, 20.0, 20.0), P.pad([(10.0, 0.0), (20.0, 10.0), (10.0, 20.0), (0.0, 10.0)]), 0.5)]
    db = P.bounds(diamond)
    assert db[0] < 50.0 and db[1] + db[3] > 0.0                      # the diamond's bounding rectangle does reach into the rectangle
    got = one_frame(cuda, [c[0] for c in cases], [c[1] for c in cases])
    for (p, g, want), value in zip(cases, got):
        assert P.poly_iou(p, g) == want                              # the restatement agrees on what is pinned
        assert value == want, "rectangle %s against %s: %.17g, expected %.17g" % (p, P.vertices(g), value, want)


def test_integer_four_gons_give_the_rectangle_kernels_bits(cuda):
    rng = np.random.default_rng(9)
    n = 200
    boxes = np.concatenate([rng.integers(0, 300, (n, 2)), rng.integers(1, 150, (n, 2))], axis=1).astype(np.float64)
    pred = boxes + rng.integers(-40, 41, (n, 4))
    pred[:, 2:] = np.maximum(pred[:, 2:], 1.0)
    gons = np.stack([P.pad(P.rect_points(b) if i % 2 else P.rect_points(b)[::-1]) for i, b in enumerate(boxes)])
    rect = one_frame(cuda, pred, boxes)
    poly = one_frame(cuda, pred, gons)
    assert ((rect > 0) & (rect < 1)).sum() >= 50 and (rect == 0).sum() >= 1
    assert same_bits(poly, rect), "differ at %s" % np.nonzero(poly != rect)[0].tolist()


# ------------------------------------------------------------------------------------------------------------- 4. splitting
def test_one_frame_calls_leave_the_bits_of_one_call(cuda):
    B = 5
    pred, gt, active, _planted = overlap_data(B)
    clip_of = [3, 0, 5, 1, 4]
    whole, whole_iou, _s = TE.run_kernel(cuda, pred, gt, clip_of, B + 1, active)
    s, ious = None, []
    for t in range(T):
        one, iou, s = TE.run_kernel(cuda, pred[t], gt[t], clip_of, B + 1, active[t], table=s)       # the [B,4] / [B,16] form of add
        ious.append(iou[0])
    assert same_bits(one, whole) and same_bits(np.stack(ious), whole_iou) and whole[:, U.FRAMES].sum() == T * B - 3


# -------------------------------------------------------------------------------------------------------------- 5. supervise
SUP_T, SUP_B, SUP_CLIPS = 12, 5, 7
SUP_CLIP_OF = [3, 0, 6, 1, 4]


def supervise_data():
    """Rotated rectangles that drift and turn; a prediction is the polygon's bounding rectangle with a little noise (an overlap
    near the ratio of the two areas), moved 300 px away where a failure is planted.  Slot 3 never fails."""
    rng = np.random.default_rng(12)
    gt, pred = np.full((SUP_T, SUP_B, 16), np.nan), np.zeros((SUP_T, SUP_B, 4))
    centre, size = rng.uniform(80, 200, (SUP_B, 2)), rng.uniform(30, 80, (SUP_B, 2))
    for t in range(SUP_T):
        for b in range(SUP_B):
            pts = P.rotated_rect(centre[b, 0] + 2.0 * t, centre[b, 1] - 1.5 * t, size[b, 0], size[b, 1], 0.2 + 0.05 * t + b)
            gt[t, b] = P.pad(pts if b % 2 else pts[::-1])
            pred[t, b] = P.bounds(gt[t, b]) + rng.standard_normal(4) * 1.5
    for t, b in ((2, 0), (6, 0), (3, 1), (9, 2), (4, 4), (11, 4)):
        pred[t, b, 0] += 300.0
    gt[4, 1] = np.nan                   # skip 1: slot 1 failed on 3, its restart frame 4 has no object
    gt[6, 1] = ABSENT["two vertices"]   # skip 3: slot 1 failed on 3, its restart frame 6 has no object
    gt[1, 3] = ABSENT["collinear"]      # an absent object while tracking
    pred[1, 2, 1] = np.inf              # a prediction that is not finite: overlap 0, a failure of slot 2
    pred[5, 2, 3] = -3.0                # a negative height: clamped, overlap 0, slot 2 fails again after its restart
    active = np.ones((SUP_T, SUP_B), dtype=np.uint8)
    active[5, 3] = active[7, 0] = 0
    return pred, gt, active


@pytest.mark.parametrize("skip", [1, 3])
@pytest.mark.parametrize("burn_in", [0, 2])
def test_supervise_matches_the_restated_walk(cuda, skip, burn_in):
    from ntmtrack import evaluate as E
    pred, gt, active = supervise_data()
    w_codes, w_iou, w_table, w_state, _r = P.walk_poly(pred, gt, SUP_CLIP_OF, SUP_CLIPS, active, skip=skip, burn_in=burn_in)
    judged = ~np.isnan(w_iou)
    print("skip %d burn_in %d: codes per slot %s" % (skip, burn_in, w_codes.T.tolist()))
    assert w_table[:, S.FAILURES].sum() >= 4 and w_table[:, S.RESTARTS].sum() >= 3 and w_table[SUP_CLIP_OF[3], S.FAILURES] == 0
    assert (w_codes[:, 1] == S.SKIP).sum() > skip - 1               # the restart that had no object slipped
    assert ((w_iou[judged] == 0) | (w_iou[judged] > 0.05)).all()      # no decision hinges on a last bit

    sup = E.Supervisor(SUP_B, SUP_CLIPS, skip=skip, burn_in=burn_in, device=cuda)
    d_pred, d_gt, d_act = dev(pred, cuda), dev(gt, cuda), dev(active, cuda)
    d_clip = dev(np.asarray(SUP_CLIP_OF), cuda, torch.int32)
    codes = torch.zeros((SUP_T, SUP_B), dtype=torch.int8, device=cuda)
    ious = torch.zeros((SUP_T, SUP_B), dtype=torch.float64, device=cuda)
    for t in range(SUP_T):
        sup.plan(d_gt[t], d_act[t], d_clip, codes=codes[t], frame_iou=ious[t])
        sup.judge(d_pred[t], d_gt[t], d_clip, codes=codes[t], frame_iou=ious[t])
    torch.cuda.synchronize()
    codes, ious, table, state = codes.cpu().numpy(), ious.cpu().numpy(), sup.table.cpu().numpy(), sup.state.cpu().numpy()
    np.testing.assert_array_equal(codes, w_codes)
    np.testing.assert_array_equal(state, w_state)
    exact = [c for c in range(S.HEAD) if c != S.SUM_IOU]
    np.testing.assert_array_equal(table[:, exact], w_table[:, exact])
    e_sum = np.abs(table[:, S.SUM_IOU] - w_table[:, S.SUM_IOU]) / np.maximum(w_table[:, S.VALID], 1)
    e_iou = np.abs(ious - w_iou)[judged].max()
    print("max |SUM_IOU err| per added frame %.3g, max |frame_iou err| %.3g" % (e_sum.max(), e_iou))
    assert (np.isnan(ious) == ~judged).all() and e_sum.max() <= ATOL and e_iou <= ATOL
    for row in (2, 5):                                               # rows no slot named stay as the owner made them
        assert (table[row] == S.new_table(1)[0]).all()


# ---------------------------------------------------------------------------------------------------- 6. through the trackers
SKIP, BURN_IN = TS.SKIP, TS.BURN_IN
TURN = np.radians(20.0)
POLY_SEED = 36                                                       # the first seed from 31 on whose turned clips leave, for both families, a clip
                                                                     # that never fails beside the planted failures (the trackers are untrained)


def turned(regions):
    """[L,4] boxes -> [L,16]: every box turned by 20 degrees about its centre (its bounding rectangle is larger than the box); an
    absent object stays absent."""
    out = np.full((len(regions), 16), np.nan)
    for i, r in enumerate(np.asarray(regions, dtype=np.float64)):
        if np.isfinite(r).all():
            out[i, :8] = flat(P.rotated_rect(r[0] + r[2] / 2, r[1] + r[3] / 2, r[2], r[3], TURN))
    return out


def polygon_clips(seed=POLY_SEED):
    from ntmtrack.evaluate import Clip
    return [Clip(c.frames, turned(c.regions)) for c in TS.supervised_clips(seed)]


def recording(maker, seen):
    """The maker behind a record of every region a tracker is started with, at its making and at every reset, in order."""
    def make(images, regions):
        seen.append(np.array(regions, dtype=np.float64, copy=True))
        trk = maker(images, regions)
        reset = trk.reset

        def recorded(slots, images, regions, *a, **k):
            seen.append(np.array(regions, dtype=np.float64, copy=True))
            return reset(slots, images, regions, *a, **k)
        trk.reset = recorded
        return trk
    return make


def family_maker(family, world_, cuda, cores):
    return TE.ntm_maker(world_, cuda) if family == "ntm" else TE.dnc_maker(world_, cuda, cores)


def assert_starts(seen, clips):
    """Clips are handed out in index order: the start regions, in the order they were given, are the bounds of the clips' first
    polygons, bit for bit."""
    starts = np.concatenate(seen)
    want = np.stack([P.bounds(c.regions[0]) for c in clips])
    assert same_bits(starts, want)
    box = TS.supervised_clips(POLY_SEED)[0].regions[0]
    assert want[0, 2] > box[2] and want[0, 3] > box[3]               # larger than the box that was turned


@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_validate_one_pass_over_polygon_clips(world, cuda, family):                                 # noqa: F811
    from ntmtrack import evaluate as E
    clips, cores, seen = polygon_clips(), [], []
    v = E.Validation(recording(family_maker(family, world, cuda, cores), seen), clips, 2, 2, return_regions=True, device=cuda).finish()
    assert v.polygons and v.supervisor is None
    assert_starts(seen, clips)
    regions = v.regions()
    assert all(np.isfinite(r).all() and r.shape == (len(c.regions) - 1, 4) for r, c in zip(regions, clips))
    want = P.score_clips_poly(regions, [c.regions for c in clips], TE.IOU_THR, TE.DIST_THR)        # rows in the caller's clip order
    assert want[:, U.FRAMES].tolist() == [8, 3, 5, 3, 5] and want[:, U.SUM_IOU].sum() > 0
    assert_poly_table(v.scores.table.cpu().numpy(), want, "%s: one pass over polygon clips, replayed" % family)


def replay_supervised(regions, codes, clips, table):
    """The device's regions and codes through the host restatement, clip by clip -> the replayed table [n_clips, HEAD]."""
    rows = []
    exact = [c for c in range(S.HEAD) if c != S.SUM_IOU]
    for i, c in enumerate(clips):
        w_codes, w_iou, w_table, _state, w_restart = P.walk_poly(regions[i][:, None], c.regions[1:, None], [0], 1, skip=SKIP, burn_in=BURN_IN)
        judged = ~np.isnan(w_iou[:, 0])
        assert ((w_iou[judged, 0] == 0) | (w_iou[judged, 0] > 1e-6)).all(), w_iou[:, 0].tolist()     # no decision hinges on a last bit
        assert codes[i].tolist() == w_codes[:, 0].tolist(), "clip %d" % i
        assert (np.isnan(regions[i]).all(axis=1) == (w_codes[:, 0] == S.SKIP)).all() and np.isfinite(regions[i][w_codes[:, 0] != S.SKIP]).all()
        for t in np.nonzero(w_restart[:, 0])[0]:                     # a restart starts from the polygon's bounds
            assert same_bits(regions[i][t], P.bounds(c.regions[t + 1])), "clip %d frame %d" % (i, t + 1)
        np.testing.assert_array_equal(table[i, exact], w_table[0, exact], "clip %d" % i)
        err = abs(table[i, S.SUM_IOU] - w_table[0, S.SUM_IOU])
        assert err <= ATOL * max(w_table[0, S.VALID], 1), "clip %d: |SUM_IOU err| %.3g over %d frames" % (i, err, w_table[0, S.VALID])
        rows.append(w_table[0])
    return np.stack(rows)


@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_validate_supervised_over_polygon_clips(world, cuda, family):                               # noqa: F811
    from ntmtrack import evaluate as E
    clips, cores, seen = polygon_clips(), [], []
    v = E.Validation(recording(family_maker(family, world, cuda, cores), seen), clips, 2, 2, return_regions=True, device=cuda,
                     protocol="supervised", skip=SKIP, burn_in=BURN_IN).finish()
    if family == "dnc":
        TE.assert_one_workgroup_family(cores)
    assert_starts(seen, clips)
    regions, codes, table = v.regions(), v.codes(), v.supervisor.table.cpu().numpy()
    want = replay_supervised(regions, codes, clips, table)
    print("%s: replayed codes %s" % (family, [c.tolist() for c in codes]))
    assert want[:, S.FAILURES].sum() >= 2 and want[:, S.RESTARTS].sum() >= 2
    assert ((want[:, S.FAILURES] == 0) & (want[:, S.VALID] > 0)).any()
    res = v.supervisor.result()
    assert res["failures"] == int(want[:, S.FAILURES].sum()) and res["restarts"] == int(want[:, S.RESTARTS].sum())


@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_polygon_rounds_after_the_first_do_not_synchronise(world, cuda, family):                    # noqa: F811
    from ntmtrack import evaluate as E
    cores = []
    v = E.Validation(family_maker(family, world, cuda, cores), polygon_clips(), 2, 2, device=cuda, protocol="supervised", skip=SKIP,
                     burn_in=BURN_IN)
    assert v.polygons and v.step()                                 # builds the tracker, its plans and workspaces
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
    res = v.finish().supervisor.result()
    assert res["failures"] >= 2 and res["restarts"] >= 2          # the planted failures ran inside the unsynchronised rounds


@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_a_rectangle_clip_beside_a_polygon_clip(world, cuda, family):                               # noqa: F811
    """The polygon clip first, the rectangle clip (with its planted failure) second: the rows come back in that order, and the
    rectangle clip's row, scored as a 4-gon, is the row the rectangle entry points give for the same regions."""
    from ntmtrack import evaluate as E
    rect_clips = TS.supervised_clips(POLY_SEED)
    poly_clip, rect_clip = polygon_clips()[1], rect_clips[2]
    clips = [poly_clip, rect_clip]
    maker = family_maker(family, world, cuda, [])
    gt = np.asarray(rect_clip.regions, dtype=np.float64)

    # one pass
    v = E.Validation(maker, clips, 2, 2, return_regions=True, device=cuda).finish()
    regions, table = v.regions(), v.scores.table.cpu().numpy()
    assert v.polygons and [len(r) for r in regions] == [len(poly_clip.regions) - 1, len(rect_clip.regions) - 1]
    assert_poly_table(table[:1], P.score_clips_poly(regions[:1], [poly_clip.regions], TE.IOU_THR, TE.DIST_THR), "the polygon clip's row")
    by_rect, _iou, _s = TE.run_kernel(cuda, regions[1][:, None], gt[1:, None], [0], 1)
    assert_poly_table(table[1:], by_rect, "%s: the rectangle clip's row against ntk_track_overlap_scores" % family)

    # supervised
    v = E.Validation(maker, clips, 2, 2, return_regions=True, device=cuda, protocol="supervised", skip=SKIP, burn_in=BURN_IN).finish()
    regions, codes, table = v.regions(), v.codes(), v.supervisor.table.cpu().numpy()
    replay_supervised(regions[:1], codes[:1], [poly_clip], table[:1])
    sup = E.Supervisor(1, 1, skip=SKIP, burn_in=BURN_IN, device=cuda)
    d_regions, d_gt, d_clip = dev(regions[1][:, None], cuda), dev(gt[1:, None], cuda), dev(np.zeros(1), cuda, torch.int32)
    r_codes = torch.zeros((len(regions[1]), 1), dtype=torch.int8, device=cuda)
    for t in range(len(regions[1])):
        sup.plan(d_gt[t], None, d_clip, codes=r_codes[t])
        sup.judge(d_regions[t], d_gt[t], d_clip, codes=r_codes[t])
    by_rect = sup.table.cpu().numpy()[0]
    assert codes[1].tolist() == r_codes.cpu().numpy()[:, 0].tolist() and by_rect[S.FAILURES] >= 1 and by_rect[S.RESTARTS] >= 1
    exact = [c for c in range(S.HEAD) if c != S.SUM_IOU]
    np.testing.assert_array_equal(table[1, exact], by_rect[exact])
    err = abs(table[1, S.SUM_IOU] - by_rect[S.SUM_IOU])
    print("%s: the rectangle clip's supervised row against ntk_track_supervise: |SUM_IOU err| %.3g" % (family, err))
    assert err <= ATOL * max(by_rect[S.VALID], 1)


# ------------------------------------------------------------------------------------------------------- 7. unchanged path
class CountingLib(object):
    """The library behind a count of the calls of each entry."""

    def __init__(self, real):
        self._real, self.calls = real, collections.Counter()

    def __getattr__(self, name):
        fn = getattr(self._real, name)

        def call(*args):
            self.calls[name] += 1
            return fn(*args)
        return call


def polygon_entries(calls):
    return sorted(name for name in calls if name.endswith("_poly") or name == "ntk_track_poly_bounds")


def test_rectangle_clips_make_no_polygon_call(world, cuda, monkeypatch):                            # noqa: F811
    from ntmtrack import _lib, evaluate as E
    clips = TS.supervised_clips()
    maker = TE.ntm_maker(world, cuda)
    lib = CountingLib(_lib.lib())
    monkeypatch.setattr(_lib, "lib", lambda: lib)
    v = E.Validation(maker, clips, 2, 2, return_regions=True, device=cuda).finish()
    assert not v.polygons and polygon_entries(lib.calls) == [] and lib.calls["ntk_track_overlap_scores"] >= 4
    regions, table = v.regions(), v.scores.table.cpu().numpy()
    lib.calls.clear()
    s = E.Validation(maker, clips, 2, 2, device=cuda, protocol="supervised", skip=SKIP, burn_in=BURN_IN).finish()
    assert polygon_entries(lib.calls) == [] and lib.calls["ntk_track_supervise"] >= 8 and s.supervisor.result()["failures"] >= 2
    # the wrapper does see a polygon call when there is one
    lib.calls.clear()
    E.OverlapScores(1, device=cuda).add(dev(regions[0][:1], cuda), dev(turned(clips[0].regions[1:2]), cuda), dev(np.zeros(1), cuda, torch.int32))
    assert polygon_entries(lib.calls) == ["ntk_track_overlap_scores_poly"]
    # the table: the regions are those of one tracker per clip (code this feature does not touch), and the rows are the bits
    # ntk_track_overlap_scores leaves when it is called on them directly, one clip per call
    monkeypatch.undo()
    assert all(same_bits(g, w_) for g, w_ in zip(regions, TE.singles(maker, clips)))
    direct = E.OverlapScores(len(clips), device=cuda)
    P_ = _lib.ptr
    for i, c in enumerate(clips):
        d_r, d_g = dev(regions[i], cuda), dev(np.asarray(c.regions, dtype=np.float64)[1:], cuda)
        d_c = dev(np.array([i]), cuda, torch.int32)
        _lib.check(_lib.lib().ntk_track_overlap_scores(P_(d_r), P_(d_g), None, P_(d_c), len(regions[i]), 1, len(clips), P_(direct._iou), 21,
                                                       P_(direct._dist), 51, P_(direct.table), None, _lib.stream()), "ntk_track_overlap_scores")
    assert same_bits(table, direct.table.cpu().numpy())
    TE.assert_table(table, U.score_clips(regions, [c.regions for c in clips], TE.IOU_THR, TE.DIST_THR), "rectangle clips, one pass")


# ------------------------------------------------------------------------------------------------- 8. a VOT directory, end to end
def test_validate_supervised_on_a_vot_directory(world, cuda, tmp_path):                             # noqa: F811
    """data.vot_clips -> evaluate.validate(protocol="supervised") -> evaluate.write_trajectory on a tree written here: one sequence
    of rectangles under color/, one of turned rectangles beside its groundtruth.txt, JPEG frames decoded when scheduled."""
    import os
    from PIL import Image
    from ntmtrack import data, evaluate as E
    rng = np.random.default_rng(4)
    H, W = TE.H, TE.W
    boxes = np.array([30.0, 25.0, 36.0, 28.0]) + np.cumsum(rng.uniform(-1, 1, size=(5, 4)), axis=0)
    quads = turned(np.array([50.0, 30.0, 30.0, 24.0]) + np.cumsum(rng.uniform(-1, 1, size=(4, 4)), axis=0))[:, :8]
    for name, sub, rows in (("a", "color", boxes), ("b", "", quads)):
        os.makedirs(os.path.join(str(tmp_path), name, sub))
        with open(os.path.join(str(tmp_path), name, "groundtruth.txt"), "w") as f:
            f.write("".join(",".join(repr(float(v)) for v in r) + "\n" for r in rows))
        for i in range(len(rows)):
            Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(
                os.path.join(str(tmp_path), name, sub, "%08d.jpg" % (i + 1)))
    with open(os.path.join(str(tmp_path), "list.txt"), "w") as f:
        f.write("a\nb\n")
    clips = data.vot_clips(str(tmp_path))
    assert [c.regions.shape for c in clips] == [(5, 4), (4, 16)] and all(c.size == (H, W) for c in clips)
    res, regions, codes = E.validate(TE.ntm_maker(world, cuda), clips, 2, 2, return_regions=True, device=cuda, protocol="supervised",
                                     skip=SKIP, burn_in=BURN_IN)
    as_polygons = [E.Clip(None, E.rect_polygons(clips[0].regions)), E.Clip(None, clips[1].regions)]
    table = np.zeros((2, S.HEAD))
    for k, col in (("valid", S.VALID), ("failures", S.FAILURES), ("restarts", S.RESTARTS), ("tracked", S.TRACKED), ("skipped", S.SKIPPED),
                   ("first_failure", S.FIRST_FAILURE)):
        table[:, col] = res["clips"][k]
    table[:, S.SUM_IOU] = np.where(table[:, S.VALID] > 0, res["clips"]["accuracy"] * table[:, S.VALID], 0.0)
    replay_supervised(regions, codes, as_polygons, table)
    assert res["tracked"] >= 2 and res["tracked"] + res["skipped"] + res["restarts"] == 7
    for i, c in enumerate(clips):
        path = str(tmp_path / ("%s_001.txt" % "ab"[i]))
        E.write_trajectory(path, E.polygon_bounds(as_polygons[i].regions[0]), regions[i], codes[i])
        lines = open(path).read().splitlines()
        assert len(lines) == len(c.regions) and lines[0] == "1"
        assert all((line in ("0", "1", "2")) == (code != S.TRACKED_CODE) for line, code in zip(lines[1:], codes[i]))
