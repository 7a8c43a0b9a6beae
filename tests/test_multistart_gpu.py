"""GPU: the multi-start protocol on the device -- ntk_track_multistart (rectangle, polygon and mask ground truth) against the NumPy
restatement of its rules (tests/multistart_util.py) to the bits, ntk_track_eao_curve against the curve in exact rational
arithmetic, and evaluate.Validation(protocol="multistart") against the one-pass validation of the same runs and the restatement.

Model shapes, makers and bounds: those of tests/test_evaluate_gpu.py and tests/test_supervised_gpu.py."""
import numpy as np
import pytest
import torch

import evaluate_util as U
import mask_util as K
import multistart_util as M
import poly_util as P
import test_evaluate_gpu as TE
from test_evaluate_gpu import world                                  # noqa: F401  (the module-scoped fixture: cell, trunk, clips)
from test_supervised_gpu import iou_bound

pytestmark = pytest.mark.gpu

same_bits = TE.same_bits
REGION_ATOL = TE.REGION_ATOL
POLY_ATOL = 1e-12                                                    # what tests/test_polygon_gpu.py holds a polygon overlap to
H, W = TE.H, TE.W


# ------------------------------------------------------------------------------- 1. the state machine against the restatement
THETA, PATIENCE, T, B, N_RUNS, ROUNDS = 0.1, 2, 3, 5, 9, 4
RUN_OF = [[3, 0, 6, 1, 4], [3, 0, 6, 1, 4], [3, 0, 6, 1, 7], [3, 0, 6, 1, 7]]          # slot 4 changes its run after round 1
TRACE_FIRST = np.arange(N_RUNS + 1) * (T * ROUNDS)
# One letter per frame, a group per round.  H: overlaps well; l: overlaps a little (low); L: beside the ground truth (0, low);
# E: overlap == failure_overlap exactly (low); A: the ground truth is absent; I: the frame is inactive.
PATTERNS = ["HHl LlH HHH HHH",      # run 3: a streak that crosses a round boundary and fails at ordinal 2
            "HlL HHH HEl HLl",      # run 0: exactly `patience` low frames, twice, forgiven; a streak open at the run's end
            "HHH ElL HHH HHH",      # run 6: patience + 1 low frames, the first of them ON the threshold: fails at ordinal 3
            "HlA LIl HHH HAH",      # run 1: an absent and an inactive frame inside the streak that fails at ordinal 1
            "LlL HHH HlH HIl"]      # run 4 fails at ordinal 0; then run 7: a forgiven streak and one open at its end


def machine_case(kind):
    """-> (pred [R,T,B,4], gt per round, active [R,T,B] uint8).  gt: [R,T,B,4] rectangles, [R,T,B,16] polygons (the rectangle
    turned by 0.2 rad about its centre) or dense masks bool [R,T,B,64,96] (the rectangle's pixels without a hole of 2 x 2)."""
    rng = np.random.default_rng(5)
    letters = np.array([list(p.replace(" ", "")) for p in PATTERNS]).T.reshape(ROUNDS, T, B)
    rect = np.concatenate([rng.integers(8, 24, (ROUNDS, T, B, 2)), rng.integers(30, 44, (ROUNDS, T, B, 1)),
                           rng.integers(20, 28, (ROUNDS, T, B, 1))], axis=3).astype(np.float64)
    pred = rect + rng.integers(-12, 13, rect.shape) / 8.0                            # H, and what A and I are never scored with
    active = (letters != "I").astype(np.uint8)
    poly = np.full(rect.shape[:3] + (16,), np.nan)
    dense = np.zeros(rect.shape[:3] + (64, 96), dtype=bool)
    for idx in np.ndindex(ROUNDS, T, B):
        c = letters[idx]
        if c == "E":
            rect[idx], pred[idx] = (0, 0, 10, 10), (0, 0, 10, 1)                     # 10 / ((10 + 100) - 10) = 0.1, one rounding
        x, y, w, h = rect[idx]
        if c == "l":
            pred[idx] = (x + w - 3.5, y + 0.25, w, h)
        if c == "L":
            pred[idx] = (x + w + 40, y, w, h)
        poly[idx] = P.pad(P.rect_points(rect[idx]) if c == "E" else P.rotated_rect(x + w / 2, y + h / 2, w, h, 0.2))
        dense[idx][int(y):int(y + h), int(x):int(x + w)] = True
        if c != "E":
            dense[idx][int(y + h / 2):int(y + h / 2) + 2, int(x + w / 2):int(x + w / 2) + 2] = False
        if c == "A":
            rect[idx], poly[idx], dense[idx] = np.nan, np.nan, False
    return pred, {"rect": rect, "poly": poly, "mask": dense}[kind], active


def dev(a, cuda, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(cuda)


def round_truth(kind, gt_r, cuda):
    """The ground truth of one round on the device, as the scoring entries take it."""
    from ntmtrack import evaluate as E
    if kind != "mask":
        return dev(gt_r, cuda)
    blocks = [((b,),) + E.MaskRegions.from_arrays(gt_r[:, b]).cells(0, gt_r.shape[0]) for b in range(gt_r.shape[1])]
    return E.upload_masks(blocks, gt_r.shape[:2], cuda)


def run_machine(cuda, kind, pred, gt, active, run_of, every=1):
    """The rounds through one MultiStart -> (table, trace, frame_iou [R,T,B], the overlap kernel's own frame_iou [R,T,B]).
    every=2: a frame on which every slot is inactive goes behind every frame."""
    from ntmtrack import evaluate as E
    ms = E.MultiStart(N_RUNS, TRACE_FIRST, THETA, PATIENCE, device=cuda)
    scores = E.OverlapScores(N_RUNS, device=cuda)
    ious, own = [], []
    for r in range(ROUNDS):
        p, g, a = pred[r], gt[r], active[r]
        if every == 2:
            p, g = np.repeat(p, 2, axis=0), np.repeat(g, 2, axis=0)
            a = np.repeat(a, 2, axis=0)
            a[1::2] = 0
        truth, d_run = round_truth(kind, g, cuda), dev(np.asarray(run_of[r]), cuda, torch.int32)
        ious.append(ms.add(dev(p, cuda), truth, d_run, active=dev(a, cuda), frame_iou=True))
        own.append(scores.add(dev(p, cuda), truth, d_run, active=dev(a, cuda), frame_iou=True))
    torch.cuda.synchronize()
    return (ms.table.cpu().numpy(), ms.trace.cpu().numpy(), np.stack([i.cpu().numpy() for i in ious]),
            np.stack([i.cpu().numpy() for i in own]))


def restated_overlaps(kind, pred, gt, active):
    """[R,T,B]: the restatement's overlap of every scored frame through evaluate_util / poly_util / mask_util, NaN elsewhere."""
    from ntmtrack import evaluate as E
    out = np.full(pred.shape[:3], np.nan)
    for r in range(ROUNDS):
        if kind == "mask":
            for b in range(B):
                cells, rle = E.MaskRegions.from_arrays(gt[r][:, b]).cells(0, T)
                for t in range(T):
                    s = K.frame_score(pred[r, t, b], cells[t], rle, bool(active[r, t, b]))
                    out[r, t, b] = np.nan if s is None else s[0]
        else:
            out[r] = M.frame_overlaps(pred[r], gt[r], active[r], U.frame_score if kind == "rect" else P.frame_score)
    return out


@pytest.mark.parametrize("kind", ["rect", "poly", "mask"])
def test_state_machine_matches_the_restatement(cuda, kind):
    pred, gt, active = machine_case(kind)
    want_iou = restated_overlaps(kind, pred, gt, active)
    rounds = [(want_iou[r], RUN_OF[r]) for r in range(ROUNDS)]
    w_table, w_trace = M.walk(rounds, N_RUNS, TRACE_FIRST, THETA, PATIENCE)
    # the cases, on the restatement: rows (FRAMES, TRACKED, FAILED, LOW) of the runs the patterns name
    shape = lambda r: [int(w_table[r, c]) for c in (M.FRAMES, M.TRACKED, M.FAILED, M.LOW)]
    assert shape(3) == [12, 2, 1, 0] and shape(0) == [12, 10, 0, 2] and shape(6) == [12, 3, 1, 0]
    assert shape(1) == [9, 1, 1, 0] and shape(4) == [6, 0, 1, 0] and shape(7) == [5, 4, 0, 1]
    assert (w_table[[2, 5, 8]] == 0).all()
    scored = ~np.isnan(want_iou)
    on = scored & (want_iou == THETA)
    assert on.sum() == 2 and w_table[6, M.PENDING] == w_table[6, M.SUM_IOU] and w_table[0, M.PENDING] > w_table[0, M.SUM_IOU] > 0
    margin = np.abs(want_iou[scored & ~on] - THETA).min()
    print("%s: %d scored frames, %d low, the nearest overlap off the threshold is %.3g away" % (kind, scored.sum(),
                                                                                               (want_iou[scored] <= THETA).sum(), margin))
    assert margin > 1e-3 and ((want_iou[scored] > 0) & (want_iou[scored] <= THETA)).sum() >= 8          # low frames that add to PENDING

    table, trace, ious, own = run_machine(cuda, kind, pred, gt, active, RUN_OF)
    assert same_bits(ious, own), "the overlaps are not those of ntk_track_overlap_scores"
    assert (np.isnan(ious) == ~scored).all()
    if kind == "poly":                                               # clipping on the device: values to test_polygon_gpu's bound,
        assert np.abs(ious - want_iou)[scored].max() <= POLY_ATOL     # every bit against the walk over the device's own overlaps
        assert same_bits(ious[on], want_iou[on]) and same_bits(ious == 0, want_iou == 0)
        exact = [M.FRAMES, M.TRACKED, M.FAILED, M.LOW]
        np.testing.assert_array_equal(table[:, exact], w_table[:, exact])
        assert np.abs(table - w_table).max() <= 12 * POLY_ATOL and np.abs(trace - w_trace).max() <= POLY_ATOL
        w_table, w_trace = M.walk([(own[r], RUN_OF[r]) for r in range(ROUNDS)], N_RUNS, TRACE_FIRST, THETA, PATIENCE)
        want_iou = own
    bad = np.argwhere(table != w_table)
    assert same_bits(table, w_table), [(tuple(i), table[tuple(i)].hex(), w_table[tuple(i)].hex()) for i in bad[:6]]
    assert same_bits(trace, w_trace) and same_bits(ious, want_iou)

    # a slot whose run is outside the table: nothing of it is written, the other slots' bits are unchanged
    for outside in (N_RUNS, -1):
        run_of = [list(r) for r in RUN_OF]
        for r in run_of:
            r[2] = outside
        t2, tr2, i2, _own = run_machine(cuda, kind, pred, gt, active, run_of)
        assert np.isnan(i2[:, :, 2]).all() and (t2[6] == 0).all() and (tr2[TRACE_FIRST[6]:TRACE_FIRST[7]] == 0).all()
        keep, rows = [0, 1, 3, 4], [3, 0, 1, 4, 7]
        assert same_bits(i2[:, :, keep], ious[:, :, keep]) and same_bits(t2[rows], table[rows])
        assert all(same_bits(tr2[TRACE_FIRST[r]:TRACE_FIRST[r + 1]], trace[TRACE_FIRST[r]:TRACE_FIRST[r + 1]]) for r in rows)

    # the same frames with a frame on which every slot is inactive behind every one of them: the same bits
    t3, tr3, i3, _own = run_machine(cuda, kind, pred, gt, active, RUN_OF, every=2)
    assert same_bits(t3, table) and same_bits(tr3, trace) and same_bits(i3[:, 0::2], ious) and np.isnan(i3[:, 1::2]).all()


def test_a_trace_stretch_that_is_too_short_is_never_overrun(cuda):
    """An ordinal that would reach the next run's stretch is counted and not stored."""
    from ntmtrack import evaluate as E
    pred, gt, active = machine_case("rect")
    first = np.array([0, 4, 4, 9])                                   # run 0 holds 4 overlaps, run 1 none, run 2 five
    ms = E.MultiStart(3, first, THETA, PATIENCE, device=cuda)
    ms.trace.fill_(-7.0)
    run_of = dev(np.array([0, 1, 2, -1, 3]), cuda, torch.int32)
    ious = np.stack([ms.add(dev(pred[r], cuda), dev(gt[r], cuda), run_of, frame_iou=True).cpu().numpy() for r in range(ROUNDS)])
    table, trace = ms.table.cpu().numpy(), ms.trace.cpu().numpy()
    assert table[:, M.FRAMES].tolist() == [12, 12, 12] and len(trace) == 9
    assert same_bits(trace[:4], ious[:, :, 0].reshape(-1)[:4]) and same_bits(trace[4:], ious[:, :, 2].reshape(-1)[:5])


# ------------------------------------------------------------------------------------------------------------- 2. the curve
def curve_set(which):
    """-> (table, trace_first, trace) of finished runs, made by the restatement's walk over planted overlaps (patience 2): runs of
    1, 63, 64, 65 and 129 scored frames, failures at ordinals 0, 63 and 64, and a run without a scored frame."""
    rng = np.random.default_rng(9)
    plans = {"mixed": [(1, None), (63, None), (64, None), (65, 0), (129, 63), (129, 64), (65, None), (129, None), (0, None), (64, 0)],
             "unfailed": [(1, None), (63, None), (64, None), (65, None), (129, None)],
             "all fail at 0": [(65, 0), (129, 0), (3, 0), (64, 0)]}[which]
    n_runs, longest = len(plans), max(n for n, _f in plans)
    overlaps = np.full((longest, n_runs), np.nan)
    for r, (n, f) in enumerate(plans):
        overlaps[:n, r] = rng.uniform(0.2, 1.0, n)
        if f is not None:
            overlaps[f:f + PATIENCE + 1, r] = rng.uniform(0.0, 0.1, PATIENCE + 1)
    first = np.concatenate([[0], np.cumsum([max(n, 1) for n, _f in plans])])
    table, trace = M.walk([(overlaps, np.arange(n_runs))], n_runs, first, THETA, PATIENCE)
    assert table[:, M.FRAMES].tolist() == [n for n, _f in plans]
    assert [int(t) if fl else None for t, fl in zip(table[:, M.TRACKED], table[:, M.FAILED])] == [f for _n, f in plans]
    return table, first, trace


@pytest.mark.parametrize("which", ["mixed", "unfailed", "all fail at 0"])
def test_eao_curve_matches_exact_arithmetic(cuda, which):
    from ntmtrack import evaluate as E
    table, first, trace = curve_set(which)
    n_runs = len(table)
    ms = E.MultiStart(n_runs, first, THETA, PATIENCE, device=cuda)
    ms.table.copy_(dev(table, cuda))
    ms.trace.copy_(dev(trace, cuda))
    for n_max in (1, 64, 65, 200):
        want = M.curve_exact(table, first, trace, n_max)
        got, again = ms.curve(n_max).cpu().numpy(), ms.curve(n_max).cpu().numpy()
        assert same_bits(got, again), "two launches on the same input differ"
        assert got.shape == (n_max,) and (np.isnan(got) == np.isnan(want)).all()
        held = ~np.isnan(want)
        n = np.arange(1, n_max + 1)
        rel = np.abs(got - want)[held] / np.where(want[held] > 0, want[held], 1.0)
        print("%s, n_max %d: max relative error %.3g (%.2f of the bound), %d NaN" % (
            which, n_max, rel.max() if held.any() else 0, (rel / ((n[held] + n_runs + 4) * 2.0 ** -53)).max() if held.any() else 0,
            (~held).sum()))
        assert (rel <= (n[held] + n_runs + 4) * 2.0 ** -53).all()
        if which == "unfailed":
            assert held.sum() == min(n_max, 129)                     # beyond the longest unfailed run S_n is empty
        if which == "all fail at 0":
            assert held.all() and (got == 0).all()
    # the result: one read-back, the EAO over the interval's non-NaN points
    res = ms.result((60, 200))
    want = M.curve_exact(table, first, trace, 200)
    used = ~np.isnan(want[59:200])
    assert res["eao_points"] == used.sum() and res["runs"] == n_runs
    assert res["eao"] == pytest.approx(want[59:200][used].mean(), rel=1e-13)
    N, N_F, failed = M.finished(table)
    assert res["per_run"]["frames"].tolist() == N.tolist() and res["per_run"]["tracked"].tolist() == N_F.tolist()
    assert res["failures"] == failed.sum() and res["runs_without_frames"] == (N == 0).sum()


# ------------------------------------------------------------------------------------------------------------ 3. end to end
SPACING, E2E_B, E2E_T = 4, 3, 4
E2E_LENGTHS = [12, 9, 7, 5, 6]
E2E_SEED = 73                                                        # the first seed from 71 on at which every reference overlap, of both
                                                                     # families, is farther off the threshold than the regions' bound


def multistart_clips(maker=None, seed=E2E_SEED):
    """Five clips of 90 x 120.  The tracker under test goes its own way over random frames, so the ground truth of clips 0 and 1
    is fitted to it: a box about a tenth of the frame wide at frame 0, then what ``maker``'s tracker makes of it frame by frame,
    moved by up to a quarter of a pixel -- the forward run from frame 0 overlaps it well, whatever the weights are.  Clip 0: from
    frame 5 on the ground truth lies three box widths beside that: the run fails at ordinal 4.  Clip 1: it does on frames 3 and 4
    alone, `patience` frames: a streak that is forgiven.  Clips 2 to 4: the drifting boxes of make_clips, clip 2 with an absent
    object inside, clip 4 with an absent first anchor.  maker=None: the boxes stay where they start (the runs are the same)."""
    from ntmtrack.evaluate import Clip
    clips = TE.make_clips(seed, E2E_LENGTHS, H, W)
    rng = np.random.default_rng(seed + 1)

    def fitted(frames, lo, hi):
        start = np.array([14.0, 40.0, 12.0, 9.0])
        if maker is None:
            tracked = np.tile(start, (len(frames) - 1, 1))
        else:
            tracked = maker(frames[:1], start[None]).track_clip(frames[1:, None]).cpu().numpy()[:, 0]
        assert np.isfinite(tracked).all() and (tracked[:, 2:] > 2).all(), "the tracker's boxes: %s" % tracked.tolist()
        regions = np.concatenate([start[None], tracked + rng.uniform(-0.25, 0.25, size=tracked.shape)])
        regions[lo:hi, 0] += 3 * regions[lo:hi, 2]
        return regions
    clips[0] = Clip(clips[0].frames, fitted(clips[0].frames, 5, None))
    clips[1] = Clip(clips[1].frames, fitted(clips[1].frames, 3, 5))
    clips[2].regions[3] = np.nan
    clips[4].regions[0] = np.nan
    return clips


def reference_tables(run_clips, regions, runs):
    """The restatement over whole runs: regions[r] [L-1,4] against the run's ground truth -> (overlaps per run, table, trace,
    trace_first)."""
    first = np.concatenate([[0], np.cumsum(runs[:, 3] - 1)])
    overlaps = [M.frame_overlaps(np.asarray(reg)[:, None], np.asarray(c.regions)[1:, None])[:, 0] for reg, c in zip(regions, run_clips)]
    table, trace = M.walk([(o[:, None], [r]) for r, o in enumerate(overlaps)], len(runs), first, THETA, PATIENCE)
    return overlaps, table, trace, first


def check_reference(overlaps, table, runs):
    """The conditions on the inputs, on the reference run: they keep the comparison from passing on an empty case."""
    N, N_F, failed = M.finished(table)
    print("reference run: runs (clip, anchor, direction, length) %s" % runs.tolist())
    print("reference run: overlaps %s" % [np.round(o, 3).tolist() for o in overlaps])
    print("reference run: N %s N_F %s failed %s" % (N.tolist(), N_F.tolist(), failed.astype(int).tolist()))
    forgiven = np.zeros(len(runs), dtype=int)                        # streaks of low frames that ended among the run's N_F frames
    for r, o in enumerate(overlaps):
        low = o[~np.isnan(o)][:N_F[r]] <= THETA
        forgiven[r] = sum(1 for i in range(1, len(low)) if low[i - 1] and not low[i])
    assert failed.sum() >= 1 and forgiven.sum() >= 1 and (runs[:, 2] < 0).sum() >= 1 and (~failed & (N > 0)).sum() >= 1
    # the planted ones: clip 0's forward run from frame 0 fails where the ground truth jumps, clip 1's forgives its streak
    assert runs[0].tolist() == [0, 0, 1, 12] and failed[0] and N_F[0] == 4 and N[0] == 11
    assert runs[4].tolist() == [1, 0, 1, 9] and not failed[4] and forgiven[4] == 1 and N_F[4] == N[4] == 8


def margins(overlaps, ref, run_clips):
    """-> per run, how far each scored overlap is from the threshold beyond what REGION_ATOL on the regions can move it
    (iou_bound): positive everywhere means that no decision can turn; and the bounds themselves."""
    bounds = [np.array([iou_bound(reg[t], np.asarray(c.regions)[t + 1], REGION_ATOL) for t in range(len(reg))])
              for reg, c in zip(ref, run_clips)]
    return [np.abs(o - THETA) - bnd for o, bnd in zip(overlaps, bounds)], bounds


def plain(run_clips):
    """The run clips with frames of their own: a tracker of B = 1 is handed frames[:1], and a one-frame view of a backward run
    still has its negative stride."""
    from ntmtrack.evaluate import Clip
    return [Clip(np.array(c.frames), c.regions) for c in run_clips]


def test_the_runs_of_the_end_to_end_clips():
    from ntmtrack import evaluate as E
    _run_clips, runs = E.multistart_runs(multistart_clips(), spacing=SPACING)
    assert runs.tolist() == [[0, 0, 1, 12], [0, 4, 1, 8], [0, 8, -1, 9], [0, 11, -1, 12], [1, 0, 1, 9], [1, 4, 1, 5], [1, 8, -1, 9],
                             [2, 0, 1, 7], [2, 4, -1, 5], [2, 6, -1, 7], [3, 0, 1, 5], [3, 4, -1, 5], [4, 1, 1, 5], [4, 4, -1, 5],
                             [4, 5, -1, 6]]


@pytest.fixture(scope="module")
def ntm_multistart(world, cuda):                                                                     # noqa: F811
    """The multi-start validation of the five clips with the NTM tracker, run once: (the Validation, its regions per run)."""
    from ntmtrack import evaluate as E
    clips = multistart_clips(TE.ntm_maker(world, cuda))
    v = E.Validation(TE.ntm_maker(world, cuda), clips, E2E_B, E2E_T, return_regions=True, device=cuda,
                     protocol="multistart", spacing=SPACING, patience=PATIENCE).finish()
    return v, v.regions(), clips


def test_validate_multistart_ntm_is_the_one_pass_validation_of_its_runs(world, cuda, ntm_multistart):   # noqa: F811
    from ntmtrack import evaluate as E
    v, regions, clips = ntm_multistart
    run_clips, runs = E.multistart_runs(clips, spacing=SPACING)
    assert same_bits(v.runs, runs) and v.multistart.failure_overlap == THETA and len(regions) == len(runs)
    one = E.Validation(TE.ntm_maker(world, cuda), run_clips, E2E_B, E2E_T, return_regions=True, device=cuda, protocol="one_pass").finish()
    for r, (got, want) in enumerate(zip(regions, one.regions())):
        assert got.shape == (runs[r, 3] - 1, 4) and same_bits(got, want), "run %d" % r
    overlaps, w_table, w_trace, first = reference_tables(run_clips, regions, runs)
    check_reference(overlaps, w_table, runs)
    scored = np.concatenate([o[~np.isnan(o)] for o in overlaps])
    assert np.abs(scored - THETA).min() > 1e-9                       # no decision hinges on a last bit
    table, trace = v.multistart.table.cpu().numpy(), v.multistart.trace.cpu().numpy()
    exact = [M.FRAMES, M.TRACKED, M.FAILED, M.LOW]
    np.testing.assert_array_equal(table[:, exact], w_table[:, exact])
    e_sum, e_trace = np.abs(table - w_table).max(), np.abs(trace - w_trace).max()
    print("NTM multi-start table against the restatement: max |sum err| %.3g, max |trace err| %.3g" % (e_sum, e_trace))
    assert e_sum <= TE.SUM_IOU_ATOL and e_trace <= TE.FRAME_IOU_ATOL and same_bits(v.multistart.trace_first, first)
    # the result's figures: the host arithmetic over the restatement's table and exact curve
    default = v.multistart.result(v.eao_interval, v.runs, len(clips))
    assert v.eao_interval == (115, 755) and default["eao_points"] == 641 and len(default["eao_curve"]) == 755      # failed runs: no empty S_n
    lo, hi = 2, 8
    res = v.multistart.result((lo, hi), v.runs, len(clips))
    want = E.summarize_multistart(w_table, runs, M.curve_exact(w_table, first, w_trace, hi), (lo, hi), len(clips))
    for k in ("failures", "runs", "runs_without_frames", "clips_without_runs", "eao_points"):
        assert res[k] == want[k], k
    for k in ("accuracy", "robustness", "eao"):
        assert res[k] == pytest.approx(want[k], rel=1e-12) and 0 < res[k] < 1, k
    for k in ("clip", "anchor", "direction", "frames", "tracked", "failed"):
        assert res["per_run"][k].tolist() == want["per_run"][k].tolist(), k
    np.testing.assert_allclose(res["per_run"]["accuracy"], want["per_run"]["accuracy"], rtol=1e-12)
    np.testing.assert_allclose(res["clips"]["accuracy"], want["clips"]["accuracy"], rtol=1e-12)
    np.testing.assert_allclose(res["eao_curve"], want["eao_curve"], rtol=1e-12)
    assert res["clips_without_runs"] == 0 and res["runs"] == 15
    with pytest.raises(ValueError):
        v.codes()


def test_validate_function_returns_the_multistart_result(world, cuda, ntm_multistart):              # noqa: F811
    from ntmtrack import evaluate as E
    v, regions, clips = ntm_multistart
    res, got = E.validate(TE.ntm_maker(world, cuda), clips, E2E_B, E2E_T, return_regions=True, device=cuda,
                          protocol="multistart", spacing=SPACING, patience=PATIENCE, eao_interval=(2, 8))
    assert all(same_bits(a, b) for a, b in zip(got, regions)) and len(got) == len(regions)
    want = v.multistart.result((2, 8), v.runs, 5)
    assert res["eao"] == want["eao"] and res["accuracy"] == want["accuracy"] and res["robustness"] == want["robustness"]
    assert res["per_run"]["tracked"].tolist() == want["per_run"]["tracked"].tolist() and "decode" not in res


def test_validate_multistart_dnc_matches_one_tracker_per_run(world, cuda):                          # noqa: F811
    from ntmtrack import evaluate as E
    cores, ref_cores = [], []
    clips = multistart_clips(TE.dnc_maker(world, cuda, ref_cores))
    run_clips, runs = E.multistart_runs(clips, spacing=SPACING)
    ref = TE.singles(TE.dnc_maker(world, cuda, ref_cores), plain(run_clips))
    overlaps, w_table, w_trace, first = reference_tables(run_clips, ref, runs)
    check_reference(overlaps, w_table, runs)
    room, bounds = margins(overlaps, ref, run_clips)
    for r, (o, m) in enumerate(zip(overlaps, room)):                 # the margin: no decision can turn within the regions' bound
        assert (m[~np.isnan(o)] > 0).all(), "run %d: overlaps %s, margins %s" % (r, o, m)
    v = E.Validation(TE.dnc_maker(world, cuda, cores), clips, E2E_B, E2E_T, return_regions=True, device=cuda, protocol="multistart",
                     spacing=SPACING, patience=PATIENCE).finish()
    TE.assert_one_workgroup_family(cores + ref_cores)
    regions = v.regions()
    err = max(np.abs(g - w_).max() for g, w_ in zip(regions, ref))
    print("DNC (seq family): multi-start at B = %d against one B = 1 tracker per run: max |region err| %.3g px" % (E2E_B, err))
    assert all(g.shape == w_.shape and np.isfinite(g).all() for g, w_ in zip(regions, ref)) and err <= REGION_ATOL
    table = v.multistart.table.cpu().numpy()
    exact = [M.FRAMES, M.TRACKED, M.FAILED, M.LOW]
    np.testing.assert_array_equal(table[:, exact], w_table[:, exact])
    for r, (o, bnd) in enumerate(zip(overlaps, bounds)):
        allowed = bnd[~np.isnan(o)].sum() + TE.SUM_IOU_ATOL
        assert np.abs(table[r, [M.SUM_IOU, M.PENDING]] - w_table[r, [M.SUM_IOU, M.PENDING]]).max() <= allowed, "run %d" % r


# ------------------------------------------------------------------------------------------------------ 4. no synchronisation
@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_multistart_rounds_after_the_first_do_not_synchronise(world, cuda, family):                 # noqa: F811
    from ntmtrack import evaluate as E
    cores = []
    maker = TE.ntm_maker(world, cuda) if family == "ntm" else TE.dnc_maker(world, cuda, cores)
    v = E.Validation(maker, multistart_clips(maker), E2E_B, E2E_T, device=cuda, protocol="multistart", spacing=SPACING, patience=PATIENCE)
    assert v.step()                                                # builds the tracker, its plans and workspaces
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
    res = v.finish().multistart.result((2, 8), v.runs, 5)
    assert res["failures"] >= 1 and res["per_run"]["failed"][1:].any()       # a failure confirmed inside the unsynchronised rounds
