"""GPU: the supervised protocol on the device -- ntk_track_restart_boxes against the host geometry, ntk_track_supervise against
the NumPy restatement of its rules (tests/supervised_util.py), a restart inside the online trackers' pass against reset, and
evaluate.validate(protocol="supervised") against one B = 1 tracker per clip driven from the host (supervised_util.run_supervised:
code this feature does not touch).

Model shapes, clips and makers: those of tests/test_evaluate_gpu.py."""

import numpy as np
import pytest
import torch

import evaluate_util as U
import supervised_util as S
import test_evaluate_gpu as TE
from test_evaluate_gpu import world                                  # noqa: F401  (the module-scoped fixture: cell, trunk, clips)

pytestmark = pytest.mark.gpu

REGION_ATOL, OFFSET_ATOL = TE.REGION_ATOL, 1e-4                      # what the existing tests hold a batch to against single trackers
same_bits = TE.same_bits
H, W = TE.H, TE.W


def dev(a, cuda, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(cuda)


# --------------------------------------------------------------------------------- 1. restart boxes against the host geometry
SENT = -777.25


def ulp32_distance(a, b):
    """Distance in units in the last place between two non-negative fp32 arrays."""
    return np.abs(a.view(np.int32).astype(np.int64) - b.view(np.int32).astype(np.int64))


@pytest.mark.parametrize("size", [(90, 120), (64, 80)])
@pytest.mark.parametrize("B", [1, 5, 70])
@pytest.mark.parametrize("mask", ["all", "none", "alternating"])
def test_restart_boxes_match_the_host_geometry(cuda, B, mask, size):
    from ntmtrack import _lib
    h, w = size
    rng = np.random.default_rng(100 * B + h)
    regions = np.concatenate([rng.uniform(0.05, 0.5, (B, 2)) * [w, h], rng.uniform(0.1, 0.4, (B, 2)) * [w, h]], axis=1)
    regions[B // 2] = [0.21, 0.33, 0.25, 0.125]                       # one region given normalised (all four < 1)
    restart = {"all": np.ones(B), "none": np.zeros(B), "alternating": np.arange(B) % 2 == 0}[mask].astype(np.uint8)
    active = (np.arange(B) % 3 != 1).astype(np.uint8)
    state = np.full((B, 10), SENT)
    state[:, 0], state[:, 1] = w, h
    d_state = dev(state, cuda)
    d_c32, d_reg = torch.full((B, 4), SENT, device=cuda), torch.full((B, 4), SENT, device=cuda, dtype=torch.float64)
    d_off, d_frame = torch.full((B, 2), SENT, device=cuda), torch.full((B,), 12345, device=cuda, dtype=torch.int32)
    d_gts = torch.full((B, 64), SENT, device=cuda)
    d_run, d_move = torch.full((B,), 9, device=cuda, dtype=torch.uint8), torch.full((B,), 9, device=cuda, dtype=torch.uint8)
    P = _lib.ptr
    d_in, d_restart, d_active = dev(regions, cuda), dev(restart, cuda), dev(active, cuda)
    _lib.check(_lib.lib().ntk_track_restart_boxes(P(d_in), P(d_restart), P(d_active), B, 8.0, 6.0,
                                                  float(6 // 3), 64, P(d_state), P(d_c32), P(d_reg), P(d_off), P(d_frame), P(d_gts),
                                                  P(d_run), P(d_move), _lib.stream()), "ntk_track_restart_boxes")
    torch.cuda.synchronize()
    rows, c32, gts = S.first_frame_geometry(regions, w, h)
    on = restart.astype(bool)
    g_state, g_c32, g_reg, g_gts = d_state.cpu().numpy(), d_c32.cpu().numpy(), d_reg.cpu().numpy(), d_gts.cpu().numpy()
    # restarted rows: the bits of the NumPy path (both are IEEE float64 without contraction)
    bad = np.argwhere(g_state[on] != rows[on])
    assert same_bits(g_state[on], rows[on]), "state rows differ by up to %.3g: %s" % (
        np.abs(g_state[on] - rows[on]).max(), [(tuple(i), g_state[on][tuple(i)].hex(), rows[on][tuple(i)].hex()) for i in bad[:6]])
    assert same_bits(g_c32[on], c32[on]) and same_bits(g_reg[on], regions[on])
    assert (d_off.cpu().numpy()[on] == 0).all() and (d_frame.cpu().numpy()[on] == 0).all()
    if on.any():
        ulps = ulp32_distance(g_gts[on], gts[on])
        print("heat-map: %d of %d elements differ from the host's, at most %d fp32 ulp" % ((ulps > 0).sum(), ulps.size, ulps.max()))
        assert ulps.max() <= 1
        assert np.abs(g_gts[on].astype(np.float64).sum(axis=1) - 1).max() <= 1e-6 and (g_gts[on] >= 0).all()
    # rows that do not restart keep their sentinels everywhere but in gts0, which is zero
    off = ~on
    want_state = np.full((B, 10), SENT)
    want_state[:, 0], want_state[:, 1] = w, h
    assert same_bits(g_state[off], want_state[off]) and (g_c32[off] == SENT).all() and (g_reg[off] == SENT).all()
    assert (d_off.cpu().numpy()[off] == SENT).all() and (d_frame.cpu().numpy()[off] == 12345).all()
    assert (g_gts[off] == 0).all() and not np.signbit(g_gts[off]).any()
    assert d_run.cpu().numpy().tolist() == (active | restart).tolist()
    assert d_move.cpu().numpy().tolist() == (active & (1 - restart)).tolist()


# ------------------------------------------------------------------------------- 2. the state machine against the restatement
T, B, N_CLIPS = 40, 5, 7
CLIP_OF = [3, 0, 6, 1, 4]


def machine_data():
    """Predictions that overlap their ground truth well, except where a failure is planted (a prediction moved off its box)."""
    rng = np.random.default_rng(11)
    gt = np.concatenate([rng.uniform(10, 200, (T, B, 2)), rng.uniform(30, 120, (T, B, 2))], axis=2)
    pred = gt + rng.standard_normal((T, B, 4)) * np.array([2, 2, 1.5, 1.5])
    for t, b in ((3, 0), (12, 0), (5, 1), (39, 1), (37, 2), (20, 4), (38, 4)):       # slot 3 never fails
        pred[t, b, 0] = gt[t, b, 0] + gt[t, b, 2] + 40.0
    gt[11, 1] = np.nan                  # defaults: slot 1 failed on 5 and is inactive on 6, its restart frame 11 has no object
    gt[21, 4] = np.nan                  # skip 1: slot 4 failed on 20, its restart frame 21 has no object
    gt[2, 4, 2] = 0.0                   # an absent object while tracking
    pred[30, 3] = gt[30, 3]             # identical boxes: overlap exactly 1
    pred[25, 2, 3] = -3.0               # a negative height: clamped, overlap 0, a failure of slot 2
    pred[33, 4, 1] = np.inf             # a prediction that is not finite: overlap 0, a failure of slot 4
    active = np.ones((T, B), dtype=np.uint8)
    active[15, 3] = active[30, 0] = active[6, 1] = 0
    return pred, gt, active


def occurrences(codes, skip, burn_in):
    """What the walk's codes show, per kind of event."""
    seen = {"failure": 0, "restart": 0, "delayed restart": 0, "failure inside a burn-in": 0, "failure in the last skip frames": 0,
            "slot that never fails": 0}
    for b in range(codes.shape[1]):
        col = codes[:, b]
        fails, restarts = np.nonzero(col == S.FAILURE)[0], np.nonzero(col == S.RESTART)[0]
        seen["failure"] += len(fails)
        seen["restart"] += len(restarts)
        seen["slot that never fails"] += int(len(fails) == 0 and (col == S.TRACKED_CODE).any())
        for f in fails:
            later = restarts[restarts > f]
            # frames of the slot between the failure and its restart: more than skip - 1 of them sat out means the restart slipped
            if len(later) and (col[f + 1:later[0]] == S.SKIP).sum() > skip - 1:
                seen["delayed restart"] += 1
            start = restarts[restarts < f].max() if (restarts < f).any() else -1
            judged_since = (col[start + 1:f + 1] != S.INACTIVE).sum()
            seen["failure inside a burn-in"] += int(judged_since <= burn_in)
            seen["failure in the last skip frames"] += int(f >= codes.shape[0] - skip)
    return seen


def run_machine(cuda, pred, gt, active, clip_of, skip, burn_in, interleave=False):
    """The frames through one Supervisor, one plan and one judge per frame -> (codes [T,B], frame_iou [T,B], table, state).
    interleave: a frame on which every slot is inactive goes between every two frames (and changes nothing)."""
    from ntmtrack import evaluate as E
    sup = E.Supervisor(B, N_CLIPS, skip=skip, burn_in=burn_in, device=cuda)
    d_pred, d_gt, d_act, d_clip = dev(pred, cuda), dev(gt, cuda), dev(active, cuda), dev(np.asarray(clip_of), cuda, torch.int32)
    codes = torch.zeros((T, B), dtype=torch.int8, device=cuda)
    ious = torch.zeros((T, B), dtype=torch.float64, device=cuda)
    idle = torch.zeros((B,), dtype=torch.uint8, device=cuda)
    for t in range(T):
        sup.plan(d_gt[t], d_act[t], d_clip, codes=codes[t], frame_iou=ious[t])
        sup.judge(d_pred[t], d_gt[t], d_clip, codes=codes[t], frame_iou=ious[t])
        if interleave:
            scratch = torch.zeros((B,), dtype=torch.int8, device=cuda)
            track, restart = sup.plan(d_gt[t], idle, d_clip, codes=scratch)
            sup.judge(d_pred[t], d_gt[t], d_clip, codes=scratch)
            assert (scratch.cpu().numpy() == S.INACTIVE).all() and not track.any() and not restart.any()
    torch.cuda.synchronize()
    return codes.cpu().numpy(), ious.cpu().numpy(), sup.table.cpu().numpy(), sup.state.cpu().numpy()


@pytest.mark.parametrize("skip,burn_in", [(5, 10), (1, 0)])
def test_state_machine_matches_the_restatement(cuda, skip, burn_in):
    pred, gt, active = machine_data()
    w_codes, w_iou, w_table, w_state = S.walk(pred, gt, CLIP_OF, N_CLIPS, active, skip=skip, burn_in=burn_in)
    seen = occurrences(w_codes, skip, burn_in)
    print("skip %d burn_in %d: %s" % (skip, burn_in, seen))
    needed = [k for k in seen if not (k == "failure inside a burn-in" and burn_in == 0)]
    assert all(seen[k] >= 1 for k in needed), seen
    judged = ~np.isnan(w_iou)
    assert ((w_iou[judged] == 0) | (w_iou[judged] > 0.3)).all()          # no decision hinges on a last bit
    codes, ious, table, state = run_machine(cuda, pred, gt, active, CLIP_OF, skip, burn_in)
    np.testing.assert_array_equal(codes, w_codes)
    np.testing.assert_array_equal(state, w_state)
    exact = [c for c in range(S.HEAD) if c != S.SUM_IOU]
    np.testing.assert_array_equal(table[:, exact], w_table[:, exact])
    e_sum, e_iou = np.abs(table[:, S.SUM_IOU] - w_table[:, S.SUM_IOU]).max(), np.abs(ious - w_iou)[judged].max()
    print("max |SUM_IOU err| %.3g, max |frame_iou err| %.3g" % (e_sum, e_iou))
    assert (np.isnan(ious) == ~judged).all() and e_sum <= TE.SUM_IOU_ATOL and e_iou <= TE.FRAME_IOU_ATOL
    for row in (2, 5):                                               # rows no slot named stay as the owner made them
        assert (table[row] == S.new_table(1)[0]).all()

    # a slot whose row is outside the table: code -1, nothing of it written, the others' bits unchanged
    for outside in (N_CLIPS, -1):
        clip_of = list(CLIP_OF)
        clip_of[2] = outside
        c2, i2, t2, s2 = run_machine(cuda, pred, gt, active, clip_of, skip, burn_in)
        assert (c2[:, 2] == S.INACTIVE).all() and np.isnan(i2[:, 2]).all() and (s2[2] == 0).all()
        assert (t2[CLIP_OF[2]] == S.new_table(1)[0]).all()
        keep = [0, 1, 3, 4]
        assert same_bits(c2[:, keep], codes[:, keep]) and same_bits(i2[:, keep], ious[:, keep]) and same_bits(s2[keep], state[keep])
        assert all(same_bits(t2[CLIP_OF[b]], table[CLIP_OF[b]]) for b in keep)

    # the same frames with a frame on which every slot is inactive between every two of them: the same bits
    c3, i3, t3, s3 = run_machine(cuda, pred, gt, active, CLIP_OF, skip, burn_in, interleave=True)
    assert same_bits(c3, codes) and same_bits(i3, ious) and same_bits(t3, table) and same_bits(s3, state)


# --------------------------------------------------------------------------------- 3. a restart inside the pass equals reset
class CountingTrunk(object):
    """The trunk behind a counter of its calls (the trackers ask a trunk's signature for ``latency`` and ``out``)."""

    def __init__(self, vgg):
        self.vgg, self.calls = vgg, 0

    def __call__(self, frames, out=None, latency=False):
        self.calls += 1
        return self.vgg(frames, out=out, latency=latency)


def make_tracker(family, world_, cuda, images, regions):
    from ntmtrack import online
    trunk = CountingTrunk(world_["vgg"])
    if family == "ntm":
        return online.BatchNTMTracker(images, regions, world_["cell"], trunk, device=cuda), trunk
    return online.BatchDNCTracker(images, regions, TE.dnc_core(cuda), trunk, device=cuda), trunk


@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_a_restart_inside_the_pass_equals_reset(world, cuda, family):                               # noqa: F811
    rng = np.random.default_rng(41)
    n, frames_n = 3, 4
    first = rng.integers(0, 256, size=(n, H, W, 3), dtype=np.uint8)
    frames = rng.integers(0, 256, size=(frames_n, n, H, W, 3), dtype=np.uint8)
    start = np.array([[20.0, 15.0, 40.0, 30.0], [50.0, 30.0, 36.0, 28.0], [30.0, 40.0, 44.0, 26.0]])
    again = np.array([61.5, 22.25, 30.0, 33.5])                      # where slot 1 is started again, on the second tracked frame
    AT = 1
    restart = dev(np.array([0, 1, 0], dtype=np.uint8), cuda)
    regions_in = torch.full((n, 4), np.nan, device=cuda, dtype=torch.float64)     # only the restarted slot's row may be read
    regions_in[1] = dev(again, cuda)

    def run(variant):
        trk, trunk = make_tracker(family, world, cuda, first, start)
        out, offs = [], []
        for t in range(frames_n):
            before = trunk.calls
            if variant == "in the pass" and t == AT:
                r = trk.track(frames[t], restart=restart, restart_regions=regions_in)
            elif variant == "reset" and t == AT:
                trk.reset([1], frames[t, 1:2], again[None])
                before = trunk.calls                                  # reset's own pass is the cost the feature removes
                r = trk.track(frames[t], active=[1, 0, 1])
            elif variant == "zeros":
                r = trk.track(frames[t], restart=torch.zeros_like(restart), restart_regions=regions_in)
            else:
                r = trk.track(frames[t])
            assert trunk.calls == before + 1, "%s, frame %d: %d trunk calls" % (variant, t, trunk.calls - before)
            out.append(r.cpu().numpy())
            offs.append(trk.offsets.cpu().numpy().copy())
        return np.stack(out), np.stack(offs), trk.frame.cpu().numpy()

    a_reg, a_off, a_frame = run("in the pass")
    b_reg, b_off, b_frame = run("reset")
    c_reg, c_off, _f = run("plain")
    d_reg, d_off, _f = run("zeros")
    assert np.isfinite(a_reg).all() and same_bits(a_reg[AT, 1], again) and (a_off[AT, 1] == 0).all()
    assert a_frame.tolist() == [frames_n, frames_n - AT - 1, frames_n] and b_frame.tolist() == a_frame.tolist()
    e_reg, e_off = np.abs(a_reg[AT:, 1] - b_reg[AT:, 1]).max(), np.abs(a_off[AT:, 1] - b_off[AT:, 1]).max()
    print("%s: slot 1 after its restart, in the pass against reset: max |region diff| %.3g px, max |offset diff| %.3g"
          % (family, e_reg, e_off))
    assert e_reg <= REGION_ATOL and e_off <= OFFSET_ATOL
    assert not same_bits(a_reg[AT + 1:, 1], c_reg[AT + 1:, 1])        # the restart changed what slot 1 does
    for slot in (0, 2):
        assert same_bits(a_reg[:, slot], c_reg[:, slot]) and same_bits(a_off[:, slot], c_off[:, slot]), "slot %d" % slot
    assert same_bits(d_reg, c_reg) and same_bits(d_off, c_off)


# ------------------------------------------------------------------------- 4. validate(protocol="supervised") against singles
SKIP, BURN_IN = 2, 1
SUP_LENGTHS = [9, 4, 6, 4, 7]
SUP_SEED = 62                                                        # the first seed from 31 on whose clips meet check_inputs for both families


def supervised_clips(seed=SUP_SEED):
    """Five clips of 90 x 120: clips 0 and 2 carry planted failures, the others are the drifting boxes of make_clips (clip 4 with
    an absent object).  A planted failure: the ground truth, a box about a tenth of the frame wide, jumps three box widths along
    x.  The box update moves a box by less than cropbox_grid / bbox_grid = 8/6 of its side per frame (the offsets are tanh outputs
    in crop units), so the prediction cannot overlap the ground truth on that frame, whatever the weights are."""
    from ntmtrack.evaluate import Clip
    clips = TE.make_clips(seed, SUP_LENGTHS, H, W)
    rng = np.random.default_rng(seed + 1)

    def planted(n, jumps):
        box = np.array([14.0, 40.0, 12.0, 9.0])
        regions = np.tile(box, (n, 1)) + np.cumsum(rng.uniform(-0.25, 0.25, size=(n, 4)), axis=0)
        for frame, widths in jumps:
            regions[frame:, 0] += widths * 12.0
        return regions
    # clip 0: fails on frame 1, restarted on frame 3, fails again on the frame after its restart, restarted on frame 6
    clips[0] = Clip(clips[0].frames, planted(SUP_LENGTHS[0], [(1, 3), (4, 3)]))
    # clip 2: fails on frame 1, restarted on frame 3
    clips[2] = Clip(clips[2].frames, planted(SUP_LENGTHS[2], [(1, 3)]))
    clips[4].regions[3] = np.nan
    return clips


def iou_bound(regions, gt, atol):
    """How far the overlap of a frame can move when each of the prediction's four numbers moves by at most atol: the corners
    move by at most 2 atol, so the intersection and the prediction's area change by at most dA = 2 atol (w + h) + 4 atol^2 with
    (w, h) the larger sides, the union by at most 2 dA, and |d(I / U)| <= dI / U + I dU / U^2 <= 3 dA / U with U >= the ground
    truth's area."""
    w, h = np.maximum(regions[2], gt[2]), np.maximum(regions[3], gt[3])
    return 3 * (2 * atol * (w + h) + 4 * atol * atol) / (gt[2] * gt[3])


def reference_run(maker, clips):
    return [S.run_supervised(maker, c, skip=SKIP, burn_in=BURN_IN) for c in clips]


def check_inputs(ref, clips, strict_margins):
    """The conditions on the inputs, on the reference run: they keep the comparison from passing on an empty case."""
    table = np.stack([r[2] for r in ref])
    print("reference run: codes %s" % [r[1].tolist() for r in ref])
    print("reference run: overlaps %s" % [np.round(r[3], 4).tolist() for r in ref])
    assert table[:, S.FAILURES].sum() >= 2 and table[:, S.RESTARTS].sum() >= 2
    assert ((table[:, S.FAILURES] == 0) & (table[:, S.VALID] > 0)).any()
    assert ref[0][1][:4].tolist() == [S.FAILURE, S.SKIP, S.RESTART, S.FAILURE] and ref[2][1][:3].tolist() == [S.FAILURE, S.SKIP, S.RESTART]
    if strict_margins:
        for (regions, _codes, _row, ious), c in zip(ref, clips):
            for t in np.nonzero(~np.isnan(ious))[0]:
                p, g = regions[t], c.regions[t + 1]
                gap = max(max(p[0], g[0]) - min(p[0] + p[2], g[0] + g[2]), max(p[1], g[1]) - min(p[1] + p[3], g[1] + g[3]))
                assert ious[t] > 0.05 or (ious[t] == 0 and gap > 1.0), "frame %d: overlap %.4g, gap %.3g px" % (t + 1, ious[t], gap)


@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_validate_supervised_matches_one_tracker_per_clip(world, cuda, family):                     # noqa: F811
    from ntmtrack import evaluate as E
    clips = supervised_clips()
    cores = []
    maker = TE.ntm_maker(world, cuda) if family == "ntm" else TE.dnc_maker(world, cuda, cores)
    ref = reference_run(maker, clips)
    check_inputs(ref, clips, strict_margins=(family == "dnc"))
    v = E.Validation(maker, clips, 2, 2, return_regions=True, device=cuda, protocol="supervised", skip=SKIP, burn_in=BURN_IN).finish()
    regions, codes, table = v.regions(), v.codes(), v.supervisor.table.cpu().numpy()
    if family == "dnc":
        TE.assert_one_workgroup_family(cores)
    want_table = np.stack([r[2] for r in ref])                        # rows in the caller's clip order
    exact = [c for c in range(S.HEAD) if c != S.SUM_IOU]
    worst, worst_sum = 0.0, 0.0
    for i, (w_reg, w_codes, w_row, _ious) in enumerate(ref):
        assert codes[i].tolist() == w_codes.tolist(), "clip %d" % i
        assert (np.isnan(regions[i]) == np.isnan(w_reg)).all() and (np.isnan(regions[i]).all(axis=1) == (w_codes == S.SKIP)).all()
        held = ~np.isnan(w_reg)
        if held.any():
            worst = max(worst, np.abs(regions[i][held] - w_reg[held]).max())
        np.testing.assert_array_equal(table[i, exact], w_row[exact], "clip %d" % i)
        # SUM_IOU: the regions' bound turned into overlap, over the frames that may have been added
        counted = [t for t in range(len(w_codes)) if w_codes[t] == S.TRACKED_CODE and U.frame_score(w_reg[t], clips[i].regions[t + 1])]
        bound = sum(iou_bound(w_reg[t], clips[i].regions[t + 1], REGION_ATOL) for t in counted) + TE.SUM_IOU_ATOL
        err = abs(table[i, S.SUM_IOU] - w_row[S.SUM_IOU])
        worst_sum = max(worst_sum, err)
        assert err <= bound, "clip %d: |SUM_IOU err| %.3g, bound %.3g" % (i, err, bound)
    print("%s: validate(supervised) at B = 2 against one B = 1 tracker per clip: max |region err| %.3g px, max |SUM_IOU err| %.3g"
          % (family, worst, worst_sum))
    assert worst <= REGION_ATOL
    res = v.supervisor.result()
    assert res["failures"] == int(want_table[:, S.FAILURES].sum()) and res["restarts"] == int(want_table[:, S.RESTARTS].sum())
    assert res["clips"]["tracked"].tolist() == want_table[:, S.TRACKED].astype(int).tolist()
    with pytest.raises(ValueError):
        E.Validation(maker, clips[:1], 1, 2, device=cuda).codes()


def test_one_pass_protocol_is_todays_table(world, cuda):                                            # noqa: F811
    from ntmtrack import evaluate as E
    clips = supervised_clips()
    maker = TE.ntm_maker(world, cuda)
    v = E.Validation(maker, clips, 2, 2, return_regions=True, device=cuda, protocol="one_pass").finish()
    d = E.Validation(maker, clips, 2, 2, return_regions=True, device=cuda).finish()
    assert v.supervisor is None and same_bits(v.scores.table.cpu().numpy(), d.scores.table.cpu().numpy())
    # today's table: the one-pass regions of one tracker per clip, scored by the restatement of the overlap table
    ref = TE.singles(maker, clips)
    assert all(same_bits(g, w_) for g, w_ in zip(v.regions(), ref))
    TE.assert_table(v.scores.table.cpu().numpy(), U.score_clips(ref, [c.regions for c in clips], TE.IOU_THR, TE.DIST_THR),
                    "one_pass on the supervised test's clips")


# ------------------------------------------------------------------------------------------------------ 5. no synchronisation
@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_supervised_rounds_after_the_first_do_not_synchronise(world, cuda, family):                 # noqa: F811
    from ntmtrack import evaluate as E
    clips = supervised_clips()
    cores = []
    maker = TE.ntm_maker(world, cuda) if family == "ntm" else TE.dnc_maker(world, cuda, cores)
    v = E.Validation(maker, clips, 2, 2, device=cuda, protocol="supervised", skip=SKIP, burn_in=BURN_IN)
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
    res = v.finish().supervisor.result()
    assert res["failures"] >= 2 and res["restarts"] >= 2          # the planted failures ran inside the unsynchronised rounds
