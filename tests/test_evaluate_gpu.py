"""GPU: validation over clips on the device -- ntk_track_overlap_scores against the NumPy restatement of its rules
(tests/evaluate_util.py), and evaluate.validate (continuous batching over the slots of a BatchNTMTracker / BatchDNCTracker)
against one tracker of B = 1 per clip, code this feature does not touch.

Model shapes: tests/test_online_batch_gpu.py's (90 x 120 frames, NTM 128 x 20) and, for the DNC, the one-workgroup family on the
smallest core of tests/test_online_dnc_gpu.py."""
import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O

import evaluate_util as U

pytestmark = pytest.mark.gpu

REGION_ATOL = 1e-2                                       # the bound tests/test_online_dnc_gpu.py holds a DNC batch to
IOU_THR, DIST_THR = np.linspace(0, 1, 21), np.arange(0, 51.)
SUM_IOU_ATOL, SUM_DIST_ATOL, FRAME_IOU_ATOL = 1e-12, 1e-9, 1e-14


def same_bits(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def assert_table(got, want, what=""):
    """Counters, LOST and FIRST_LOST exact; the two sums within their bounds."""
    sums = [U.SUM_IOU, U.SUM_DIST]
    exact = [c for c in range(want.shape[1]) if c not in sums]
    e_iou, e_dist = np.abs(got[:, U.SUM_IOU] - want[:, U.SUM_IOU]).max(), np.abs(got[:, U.SUM_DIST] - want[:, U.SUM_DIST]).max()
    print("%s: max |SUM_IOU err| %.3g, max |SUM_DIST err| %.3g px" % (what, e_iou, e_dist))
    np.testing.assert_array_equal(got[:, exact], want[:, exact])
    assert e_iou <= SUM_IOU_ATOL and e_dist <= SUM_DIST_ATOL


def run_kernel(cuda, regions, gt, clip_of, n_clips, active=None, table=None, frame_iou=True):
    """One or more adds on a fresh (or the given) OverlapScores -> (table as numpy, frame_iou as numpy, the scores object)."""
    from ntmtrack import evaluate as E
    s = table if table is not None else E.OverlapScores(n_clips, device=cuda)
    fi = s.add(torch.from_numpy(np.ascontiguousarray(regions)).to(cuda), torch.from_numpy(np.ascontiguousarray(gt)).to(cuda),
               torch.tensor(clip_of, dtype=torch.int32, device=cuda),
               None if active is None else torch.from_numpy(np.ascontiguousarray(active)).to(cuda), frame_iou=frame_iou)
    torch.cuda.synchronize()
    return s.table.cpu().numpy(), None if fi is None else fi.cpu().numpy(), s


# ------------------------------------------------------------------------------------------- 1. the kernel against the rules
T, B, N_CLIPS = 6, 5, 7
CLIP_OF = [3, 0, 6, 1, 4]


def kernel_data():
    rng = np.random.default_rng(7)
    gt = np.concatenate([rng.uniform(10, 200, (T, B, 2)), rng.uniform(8, 120, (T, B, 2))], axis=2)
    pred = gt + rng.standard_normal((T, B, 4)) * np.array([25, 25, 6, 6.])
    return pred, gt


def test_kernel_matches_the_restatement(cuda):
    pred, gt = kernel_data()
    # the precondition of the counter comparisons, on the data as generated: 24 IoUs inside (0, 1) and 6 exact zeros, none within
    # 1e-9 of a threshold, nor any centre distance (they are 1.2e-3 and 1.4e-2 px away), so no count can hinge on a last bit
    ious, dists = U.accumulate(U.new_table(N_CLIPS, 21, 51), pred, gt, CLIP_OF, IOU_THR, DIST_THR)
    inside = (ious > 0) & (ious < 1)
    assert inside.sum() == 24 and (ious == 0).sum() == 6
    m_iou, m_dist = np.abs(ious[inside][:, None] - IOU_THR[None]).min(), np.abs(dists.reshape(-1, 1) - DIST_THR[None]).min()
    print("margins: IoU %.3g, centre distance %.3g px" % (m_iou, m_dist))
    assert m_iou >= 1e-9 and m_dist >= 1e-9
    nan = np.nan
    gt[0, 0], pred[0, 0] = (20.25, 31.5, 40.125, 17.0), (20.25, 31.5, 40.125, 17.0)          # identical boxes
    gt[1, 0], pred[1, 0] = (50.0, 60.0, 30.0, 20.0), (20.5, 60.0, 29.5, 20.0)                # touching along x = 50
    gt[2, 0], pred[2, 0] = (50.0, 60.0, 30.0, 20.0), (60.5, 40.5, 10.0, 19.5)                # touching along y = 60
    gt[0, 1], pred[0, 1] = (10.0, 10.0, 100.0, 80.0), (30.0, 20.0, 50.0, 40.0)               # prediction contained: 2000 / 8000
    gt[1, 1], pred[1, 1] = (30.0, 20.0, 50.0, 40.0), (10.0, 10.0, 100.0, 80.0)               # ground truth contained
    pred[2, 1, 2] = 0.0                                                                        # zero-width prediction
    pred[3, 1, 3] = -5.0                                                                       # negative height: clamped to 0
    pred[0, 2, 1] = nan                                                                        # NaN prediction: lost
    pred[1, 2, 2] = np.inf                                                                     # infinite prediction: lost
    gt[2, 2, 2] = 0.0                                                                          # ground truth with w = 0: skipped
    gt[3, 2, 3] = -1.0                                                                         # and with h < 0
    gt[0, 3, 0] = nan                                                                          # NaN ground truth: skipped
    gt[1, 3, 3] = np.inf
    active = np.ones((T, B), dtype=np.uint8)
    active[4, 4] = active[2, 3] = 0

    want = U.new_table(N_CLIPS, 21, 51)
    w_iou, w_dist = U.accumulate(want, pred, gt, CLIP_OF, IOU_THR, DIST_THR, active)
    # the precondition again, on the data with its special cases: a value is either 1e-9 away from every threshold or ON one
    # exactly, by exact arithmetic (IoU 0 and 1; 2000 / 8000 = 0.25 of the contained boxes, which must NOT count as > 0.25; the
    # distance 0 of the identical boxes)
    inside, apart = (w_iou > 0) & (w_iou < 1), np.isfinite(w_dist) & (w_dist > 0)
    d_iou, d_dist = np.abs(w_iou[inside][:, None] - IOU_THR[None]), np.abs(w_dist[apart][:, None] - DIST_THR[None])
    assert (d_iou == 0).sum() == 2 and IOU_THR[5] == 0.25 and d_iou[d_iou > 0].min() >= 1e-9 and d_dist.min() >= 1e-9
    got, g_iou, _s = run_kernel(cuda, pred, gt, CLIP_OF, N_CLIPS, active)
    assert_table(got, want, "kernel against the restatement")
    unscored = np.isnan(w_iou)
    assert unscored.sum() == 6 and (np.isnan(g_iou) == unscored).all()
    e = np.abs(g_iou - w_iou)[~unscored].max()
    print("frame_iou: max |err| %.3g" % e)
    assert e <= FRAME_IOU_ATOL
    # exact values
    assert g_iou[0, 0] == 1.0 and g_iou[1, 0] == 0.0 and g_iou[2, 0] == 0.0
    assert g_iou[0, 1] == 0.25 and g_iou[1, 1] == 0.25
    assert g_iou[2, 1] == 0.0 and g_iou[3, 1] == 0.0 and g_iou[0, 2] == 0.0 and g_iou[1, 2] == 0.0
    assert (g_iou[~unscored] >= 0).all() and (g_iou[~unscored] <= 1).all()
    # rows no slot named stay as the owner made them; FIRST_LOST of slot 0's clip is the second scored frame
    for row in (2, 5):
        assert (got[row] == U.new_table(1, 21, 51)[0]).all()
    assert got[CLIP_OF[0], U.FIRST_LOST] == 1 and got[CLIP_OF[0], U.LOST] >= 2
    assert got[CLIP_OF[2], U.FIRST_LOST] == 0 and got[CLIP_OF[2], U.FRAMES] == T - 2
    # a non-finite prediction adds no distance: the sum stays finite
    assert np.isfinite(got[:, U.SUM_DIST]).all()


def test_integer_boxes_give_numpys_bits(cuda):
    rng = np.random.default_rng(8)
    gt = np.concatenate([rng.integers(0, 300, (T, B, 2)), rng.integers(1, 150, (T, B, 2))], axis=2).astype(np.float64)
    pred = gt + rng.integers(-40, 41, (T, B, 4))
    w_iou, _d = U.accumulate(U.new_table(N_CLIPS, 21, 51), pred, gt, CLIP_OF, IOU_THR, DIST_THR)
    _t, g_iou, _s = run_kernel(cuda, pred, gt, CLIP_OF, N_CLIPS)
    assert ((w_iou > 0) & (w_iou < 1)).sum() >= 10
    assert same_bits(g_iou, w_iou)


# ------------------------------------------------------------------------------------------------------- 2. masks and rows
def test_masks_rows_and_split_calls(cuda):
    from ntmtrack import evaluate as E
    pred, gt = kernel_data()
    SENT = -777.25
    whole, whole_iou, _s = run_kernel(cuda, pred, gt, CLIP_OF, N_CLIPS)

    # an inactive (t, b) changes nothing: the same as a call in which that frame's ground truth is absent
    active = np.ones((T, B), dtype=np.uint8)
    active[1, 2] = active[5, 0] = 0
    gt_absent = gt.copy()
    gt_absent[1, 2] = gt_absent[5, 0] = np.nan
    a, a_iou, _s = run_kernel(cuda, pred, gt, CLIP_OF, N_CLIPS, active)
    b_, b_iou, _s = run_kernel(cuda, pred, gt_absent, CLIP_OF, N_CLIPS)
    assert same_bits(a, b_) and same_bits(a_iou, b_iou) and np.isnan(a_iou[1, 2]) and np.isnan(a_iou[5, 0])
    assert a[CLIP_OF[2], U.FRAMES] == T - 1 and not same_bits(a, whole)

    # clip_of = -1 and clip_of = n_clips touch nothing: every row those slots might have reached keeps its sentinel
    clip_of = [3, -1, 6, N_CLIPS, 4]
    s = E.OverlapScores(N_CLIPS + 1, device=cuda)                  # one row more than the kernel is told of
    s.n_clips = N_CLIPS
    s.table[[0, 1, 2, 5, N_CLIPS]] = SENT
    got, got_iou, _s = run_kernel(cuda, pred, gt, clip_of, N_CLIPS, table=s)
    assert (got[[0, 1, 2, 5, N_CLIPS]] == SENT).all()
    assert np.isnan(got_iou[:, [1, 3]]).all()
    for slot in (0, 2, 4):
        assert same_bits(got[clip_of[slot]], whole[clip_of[slot]]) and same_bits(got_iou[:, slot], whole_iou[:, slot])

    # two calls over frames [0,3) and [3,6), and T one-frame calls, leave the bits of one call over [0,6)
    _t, _i, s2 = run_kernel(cuda, pred[:3], gt[:3], CLIP_OF, N_CLIPS)
    two, _i, _s = run_kernel(cuda, pred[3:], gt[3:], CLIP_OF, N_CLIPS, table=s2)
    assert same_bits(two, whole)
    s1 = None
    for t in range(T):
        one, _i, s1 = run_kernel(cuda, pred[t], gt[t], CLIP_OF, N_CLIPS, table=s1, frame_iou=False)      # the [B,4] form of add
    assert same_bits(one, whole)


# ------------------------------------------------------------------------------------------------------ 3-6. the validator
H, W = 90, 120
LENGTHS = [2, 3, 6, 4, 5]
SMALL_H, SMALL_W, SMALL_LENGTHS = 64, 80, [3, 2, 4]


def make_clips(seed, lengths, h, w):
    """Random uint8 frames; the ground truth a box that drifts a few pixels per frame, with one absent object."""
    from ntmtrack.evaluate import Clip
    rng = np.random.default_rng(seed)
    clips = []
    for n in lengths:
        frames = rng.integers(0, 256, size=(n, h, w, 3), dtype=np.uint8)
        start = np.array([rng.uniform(0.15, 0.4) * w, rng.uniform(0.15, 0.4) * h, rng.uniform(0.25, 0.4) * w, rng.uniform(0.25, 0.4) * h])
        regions = start + np.cumsum(rng.uniform(-2, 2, size=(n, 4)), axis=0)
        regions[0] = start
        clips.append(Clip(frames, regions))
    return clips


@pytest.fixture(scope="module")
def world(cuda):
    """Cell and trunk of tests/test_online_batch_gpu.py's fixture; five clips of 90 x 120 and three of 64 x 80."""
    from ntmtrack.ntm import NTMCell
    from ntmtrack.vgg import VGG16Conv43
    rng = np.random.default_rng(5)
    ws = O.init_vgg_weights(rng)
    cfg = O.NTMConfig(514, 2, mem_size=128, mem_dim=20, shift_range=1, controller_hidden_size=200, controller_num_layers=1,
                      write_head_size=1, read_head_size=4)
    params = O.init_params(cfg, rng, scale=0.05)
    cell = NTMCell(2, mem_size=128, mem_dim=20, controller_hidden_size=200, controller_num_layers=1, write_head_size=1,
                   read_head_size=4, device=cuda)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, input_dim=514)
    clips = make_clips(21, LENGTHS, H, W)
    clips[2].regions[3] = np.nan                                   # the object is absent in one frame: tracked, not scored
    return {"cell": cell, "vgg": VGG16Conv43(ws, device=cuda), "clips": clips, "small": make_clips(22, SMALL_LENGTHS, SMALL_H, SMALL_W)}


def ntm_maker(world, cuda):
    from ntmtrack import online
    return lambda images, regions: online.BatchNTMTracker(images, regions, world["cell"], world["vgg"], device=cuda)


DNC_SEQ = dict(memory_size=24, word_size=5, num_reads=1, num_writes=1, hidden_size=12, clip_value=0.0)       # the smallest core of
                                                                          # tests/test_online_dnc_gpu.py (its "seq" family)


def dnc_core(cuda):
    """A fresh core of the one-workgroup family: 514 inputs, 2 outputs, cluster kernels switched off."""
    from dnc_util import conditioned_params
    from ntmtrack.dnc import DNC
    from oracle import dnc_oracle as D
    p = conditioned_params(D.DNCConfig(514, 2, **DNC_SEQ), np.random.default_rng(17), 2)
    p["lstm/w_gates"] = (p["lstm/w_gates"] * 0.05).astype(np.float32)      # trunk features are O(10): keep the gates off saturation
    core = DNC({k: DNC_SEQ[k] for k in ("memory_size", "word_size", "num_reads", "num_writes")}, {"hidden_size": DNC_SEQ["hidden_size"]},
               2, DNC_SEQ["clip_value"], device=cuda)
    core.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in p.items()})
    core.cluster_k = 0
    return core


def dnc_maker(world, cuda, cores=None):
    """-> make_tracker for Validation; every core it builds is appended to ``cores`` so that a test can ask which family ran."""
    from ntmtrack import online

    def make(images, regions):
        core = dnc_core(cuda)
        if cores is not None:
            cores.append(core)
        return online.BatchDNCTracker(images, regions, core, world["vgg"], device=cuda)
    return make


def assert_one_workgroup_family(cores):
    assert cores
    for core in cores:
        assert core.last_cluster_form is None and core.last_cluster_k == 1, (core.last_cluster_form, core.last_cluster_k)


def singles(maker, clips):
    """One tracker of B = 1 per clip, run with track_clip: [L-1,4] per clip."""
    out = []
    for c in clips:
        trk = maker(c.frames[:1], c.regions[:1])
        out.append(trk.track_clip(c.frames[1:, None]).cpu().numpy()[:, 0])
    return out


@pytest.fixture(scope="module")
def ntm_run(world, cuda):
    """validate over the five clips at B = 2, T = 2, computed once: (result, regions per clip, the table)."""
    from ntmtrack import evaluate as E
    v = E.Validation(ntm_maker(world, cuda), world["clips"], 2, 2, return_regions=True, device=cuda).finish()
    return v.scores.result(), v.regions(), v.scores.table.cpu().numpy()


def test_validate_ntm_is_bit_equal_to_one_tracker_per_clip(world, cuda, ntm_run):
    result, regions, table = ntm_run
    ref = singles(ntm_maker(world, cuda), world["clips"])
    assert len(regions) == len(LENGTHS)
    for i, (got, want) in enumerate(zip(regions, ref)):
        assert got.shape == (LENGTHS[i] - 1, 4) and np.isfinite(got).all()
        assert same_bits(got, want), "clip %d: max |diff| %.3g px" % (i, np.abs(got - want).max())
    want_table = U.score_clips(regions, [c.regions for c in world["clips"]], IOU_THR, DIST_THR)
    assert_table(table, want_table, "NTM validation table against the restatement")
    scored = [n - 1 for n in LENGTHS]
    scored[2] -= 1                                                 # the frame without an object
    assert result["clips"]["frames"].tolist() == scored and result["frames"] == sum(scored)
    assert result["clips_scored"] == 5 and result["clips_without_frames"] == 0
    assert 0 < result["mean_overlap_frames"] < 1                   # boxes that overlap their ground truth, not a comparison of zeros
    assert result["success_auc"] == pytest.approx(np.mean(want_table[:, U.HEAD:U.HEAD + 21].sum(axis=0) / sum(scored)), abs=1e-15)


def test_validate_function_returns_the_result_alone(world, cuda, ntm_run):
    from ntmtrack import evaluate as E
    res = E.validate(ntm_maker(world, cuda), world["clips"][:2], 8, 3, device=cuda)               # fewer clips than slots
    assert isinstance(res, dict) and res["clips"]["frames"].tolist() == [1, 2]
    for k in ("mean_overlap", "mean_centre_error"):
        assert same_bits(res["clips"][k], ntm_run[0]["clips"][k][:2]), k


def test_validate_dnc_matches_one_tracker_per_clip(world, cuda):
    from ntmtrack import evaluate as E
    cores, ref_cores = [], []
    v = E.Validation(dnc_maker(world, cuda, cores), world["clips"], 2, 2, return_regions=True, device=cuda).finish()
    regions, table = v.regions(), v.scores.table.cpu().numpy()
    ref = singles(dnc_maker(world, cuda, ref_cores), world["clips"])
    assert len(cores) == 1 and len(ref_cores) == len(LENGTHS)
    assert_one_workgroup_family(cores + ref_cores)
    err = max(np.abs(g - w).max() for g, w in zip(regions, ref))
    print("DNC (seq family): validate at B = 2 against one B = 1 tracker per clip: max |region err| %.3g px" % err)
    assert all(g.shape == w.shape and np.isfinite(g).all() for g, w in zip(regions, ref)) and err <= REGION_ATOL
    # the table against the restatement on the validator's OWN regions: counters, LOST and FIRST_LOST exact, sums within test 1's bounds
    assert_table(table, U.score_clips(regions, [c.regions for c in world["clips"]], IOU_THR, DIST_THR),
                 "DNC validation table against the restatement")
    scored = [n - 1 for n in LENGTHS]
    scored[2] -= 1
    assert v.scores.result()["clips"]["frames"].tolist() == scored


def test_two_frame_sizes_come_back_in_input_order(world, cuda, ntm_run):
    from ntmtrack import evaluate as E
    big, small = world["clips"], world["small"]
    mixed = [big[0], small[0], big[1], big[2], small[1], big[3], small[2], big[4]]
    where_big, where_small = [0, 2, 3, 5, 7], [1, 4, 6]
    v = E.Validation(ntm_maker(world, cuda), mixed, 2, 2, return_regions=True, device=cuda).finish()
    assert [c.size for c in v.classes] == [(H, W), (SMALL_H, SMALL_W)]
    regions, table = v.regions(), v.scores.table.cpu().numpy()
    alone = E.Validation(ntm_maker(world, cuda), small, 2, 2, return_regions=True, device=cuda).finish()
    _res, big_regions, big_table = ntm_run
    for j, i in enumerate(where_big):
        assert same_bits(regions[i], big_regions[j]) and same_bits(table[i], big_table[j]), "90 x 120 clip %d" % j
    for j, i in enumerate(where_small):
        assert same_bits(regions[i], alone.regions()[j]) and same_bits(table[i], alone.scores.table.cpu().numpy()[j]), "64 x 80 clip %d" % j
    assert v.scores.result()["clips"]["frames"].tolist() == [1, 2, 2, 4, 1, 3, 3, 4]


@pytest.mark.parametrize("family", ["ntm", "dnc"])
def test_rounds_after_the_first_do_not_synchronise(world, cuda, family):
    from ntmtrack import evaluate as E
    clips = make_clips(23, [3, 3, 5, 4], H, W)
    cores = []
    maker = ntm_maker(world, cuda) if family == "ntm" else dnc_maker(world, cuda, cores)
    v = E.Validation(maker, clips, 2, 2, device=cuda)
    assert v.step()                                                # builds the tracker, its plans and workspaces
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    rounds = 0
    try:
        while v.step():                                            # round 2 resets both slots, round 3 runs one slot half idle
            rounds += 1
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert rounds == 2
    if family == "dnc":
        assert_one_workgroup_family(cores)
    res = v.finish().scores.result()
    assert res["clips"]["frames"].tolist() == [2, 2, 4, 3]
