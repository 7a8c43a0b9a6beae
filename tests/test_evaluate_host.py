"""CPU: the host side of validation over clips -- evaluate.ClipSchedule (continuous batching of clips over slots),
data.load_frame_region / pixel_region / validation_clips (the validation records) and the arithmetic of
evaluate.OverlapScores.result() on a hand-filled table."""
import os

import numpy as np
import pytest

RANDOM_LENGTHS = np.random.default_rng(3).integers(2, 31, size=40).tolist()
SCHEDULES = [([2], 1, 1), ([2], 4, 3),
             ([2, 3, 6, 4, 5], 2, 2), ([2, 3, 6, 4, 5], 3, 4), ([2, 3, 6, 4, 5], 8, 3),
             ([5, 3, 7, 3], 2, 2),                     # clips 0 and 2 end exactly at the end of a round (4 and 6 tracked frames)
             (RANDOM_LENGTHS, 6, 5), (RANDOM_LENGTHS, 16, 7)]


@pytest.mark.parametrize("lengths,B,T", SCHEDULES)
def test_schedule_tracks_every_frame_once_in_order_in_one_slot(lengths, B, T):
    from ntmtrack.evaluate import ClipSchedule
    sched = ClipSchedule(lengths, B, T)
    Be = min(B, len(lengths))
    assert sched.B == Be and sched.T == T
    seen = {c: [] for c in range(len(lengths))}          # clip -> [(slot, frame)] in the order tracked
    holder = [-1] * Be                                   # the clip whose reset was the last one in the slot
    started = []
    rounds = list(sched)
    assert rounds == [] or rounds[0].resets == [(s, s) for s in range(Be)]
    for r in rounds:
        assert r.frame_index.shape == (T, Be) and r.active.shape == (T, Be) and r.clip_of.shape == (Be,)
        assert r.active.dtype == np.uint8 and r.clip_of.dtype == np.int32
        for slot, clip in r.resets:
            assert holder[slot] == -1 or len(seen[holder[slot]]) == lengths[holder[slot]] - 1, "reset of a slot whose clip has not ended"
            holder[slot] = clip
            started.append(clip)
        # clip_of: the slot's clip, -1 exactly for the slots without one; no clip in two slots
        held = [int(c) for c in r.clip_of if c >= 0]
        assert len(set(held)) == len(held)
        for s in range(Be):
            running = holder[s] >= 0 and len(seen[holder[s]]) < lengths[holder[s]] - 1
            assert int(r.clip_of[s]) == (holder[s] if running else -1)
            if not running:
                assert not r.active[:, s].any()
        for t in range(T):
            for s in range(Be):
                if r.active[t, s]:
                    assert int(r.clip_of[s]) == holder[s] >= 0          # only the clip whose reset came last runs in the slot
                    seen[holder[s]].append((s, int(r.frame_index[t, s])))
                else:
                    assert r.frame_index[t, s] == 0
        assert any(r.active[0]), "an empty round"
    assert started == list(range(len(lengths))), "clips are handed out in index order"
    for c, n in enumerate(lengths):
        assert [f for _s, f in seen[c]] == list(range(1, n)), "clip %d" % c
        assert len({s for s, _f in seen[c]}) == 1


def test_schedule_gives_a_new_clip_the_lowest_free_slot_at_the_next_round():
    from ntmtrack.evaluate import ClipSchedule
    rounds = list(ClipSchedule([2, 3, 6, 4, 5], 2, 2))
    assert [r.resets for r in rounds] == [[(0, 0), (1, 1)], [(0, 2), (1, 3)], [], [(1, 4)], []]
    assert rounds[0].active.tolist() == [[1, 1], [0, 1]]          # clip 0 ends mid-round: its slot idles until the round ends
    assert rounds[2].active.tolist() == [[1, 1], [1, 0]]          # so does clip 3's; clip 4 starts with the NEXT round
    assert rounds[3].clip_of.tolist() == [2, 4] and rounds[3].frame_index.tolist() == [[5, 1], [0, 2]]
    assert rounds[4].clip_of.tolist() == [-1, 4] and rounds[4].active.tolist() == [[0, 1], [0, 1]]


@pytest.mark.parametrize("lengths", [[1], [3, 1, 4], [2, 0]])
def test_schedule_refuses_a_clip_without_a_frame_to_track(lengths):
    from ntmtrack.evaluate import ClipSchedule
    with pytest.raises(ValueError):
        ClipSchedule(lengths, 2, 2)


def test_round_slices_reproduce_frame_index_and_active():
    """Round.slices() names a slot's frames once, for the frames and the ground truth alike.  [5, 2, 9, 3] over 3 slots of 4 frames
    is the smallest schedule with a clip that ends mid-round (clip 1), a slot that idles (slot 1 in round 1) and a slot refilled in
    the next round (slot 0, clip 3)."""
    from ntmtrack.evaluate import ClipSchedule
    rounds = list(ClipSchedule([5, 2, 9, 3], 3, 4))
    for r in rounds:
        frame_index, active = np.zeros_like(r.frame_index), np.zeros_like(r.active)
        for b, lo, hi in r.slices():
            assert hi > lo
            frame_index[:hi - lo, b], active[:hi - lo, b] = np.arange(lo, hi), 1
        assert np.array_equal(frame_index, r.frame_index) and np.array_equal(active, r.active)
    assert [list(r.slices()) for r in rounds] == [[(0, 1, 5), (1, 1, 2), (2, 1, 5)], [(0, 1, 3), (2, 5, 9)]]
    assert rounds[1].resets == [(0, 3)] and rounds[1].clip_of.tolist() == [3, -1, 2]


def test_the_three_kinds_of_host_truth_agree_with_the_functions_they_wrap():
    """A 4-frame clip whose object is absent on frame 2, written as rectangles, as 5-gons and as masks: present(), first() and
    take() of its truth object against regions_present, polygon_bounds / mask_bounds and fancy indexing / MaskRegions.take."""
    from ntmtrack import evaluate as E
    order = [3, 2, 1, 0]
    rects = np.array([[1.0, 2.0, 4.0, 3.0], [2.0, 2.0, 4.0, 3.0], [np.nan] * 4, [3.0, 1.0, 2.0, 5.0]])
    t = E.as_truth(rects)
    assert type(t) is E.RectTruth and len(t) == 4
    assert t.present().tolist() == E.regions_present(rects).tolist() == [True, True, False, True]
    assert t.first().tobytes() == rects[0].tobytes()
    assert type(t.take(order)) is E.RectTruth and t.take(order).regions.tobytes() == rects[order].tobytes()

    gons = np.array([[x, y, x + 4, y, x + 5, y + 2, x + 2, y + 4, x, y + 3] for x, y in ((1.0, 2.0), (2.0, 2.5), (0.0, 0.0), (3.5, 1.0))])
    gons[2] = np.nan
    t = E.as_truth(gons)
    assert type(t) is E.PolyTruth and len(t) == 4 and t.regions.shape == (4, E.POLY_DOUBLES)
    assert t.present().tolist() == E.regions_present(gons).tolist() == [True, True, False, True]
    assert t.first().tobytes() == E.polygon_bounds(E.pad_polygons(gons[0])).tobytes() and t.first().tolist() == [1.0, 2.0, 5.0, 4.0]
    assert type(t.take(order)) is E.PolyTruth and np.array_equal(t.take(order).regions, E.pad_polygons(gons)[order], equal_nan=True)
    # rectangles promoted to 4-gons (a set with a polygon clip) keep the rectangle they start from, bit for bit
    promoted = E.as_truth(rects).as_polygons()
    assert type(promoted) is E.PolyTruth and promoted.first().tobytes() == rects[0].tobytes()
    assert np.array_equal(promoted.regions, E.rect_polygons(rects), equal_nan=True) and promoted.present().tolist() == [True, True, False, True]

    dense = np.zeros((4, 6, 8), dtype=np.uint8)
    dense[0, 1:4, 2:5], dense[1, 2:5, 3:7], dense[3, 0:2, 5:8] = 1, 1, 1
    dense[1, 3, 4] = 0                                              # a hole: more than one run per row
    masks = E.MaskRegions.from_arrays(dense)
    t = E.as_truth(masks)
    assert type(t) is E.MaskTruth and len(t) == 4
    assert t.present().tolist() == E.regions_present(masks).tolist() == [True, True, False, True]
    assert t.first().tobytes() == E.mask_bounds(masks, 0).tobytes() and t.first().tolist() == [2.0, 1.0, 3.0, 3.0]
    got, want = t.take(order).regions, masks.take(order)
    assert type(t.take(order)) is E.MaskTruth
    assert all(np.array_equal(getattr(got, k), getattr(want, k)) for k in ("boxes", "counts", "offsets"))
    assert all(np.array_equal(got.dense(k, 6, 8), dense[i] != 0) for k, i in enumerate(order))


# ---------------------------------------------------------------------------------------------------- the validation records
def write_record(folder, stem, normalized_xywh, image_path):
    """A format-(B) record as the offline preparation writes it: crop box, the object box in crop coordinates, image path."""
    from ntmtrack import geometry as G
    x, y, w, h = normalized_xywh
    nb = [y, x, y + h, x + w]
    cropbox = G.calculate_cropbox(nb, 8, 6)
    in_crop = G.apply_transformation(nb, G.calculate_transformation(cropbox))
    with open(os.path.join(folder, stem + ".txt"), "w") as f:
        f.write(",".join([repr(float(v)) for v in cropbox + list(in_crop)] + [image_path, "0.0", "0.0"]) + "\n")


def test_load_frame_region_inverts_the_crop_transformation(tmp_path):
    from ntmtrack import data
    rng = np.random.default_rng(1)
    for i in range(20):
        box = (rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.6), rng.uniform(0.05, 0.35), rng.uniform(0.05, 0.35))
        write_record(str(tmp_path), "%06d" % i, box, "imgs/%06d.JPEG" % i)
        assert not os.path.exists(str(tmp_path / ("%06d.bin" % i)))                  # the heat-map is not needed
        path, region = data.load_frame_region(str(tmp_path / ("%06d" % i)))
        assert path == "imgs/%06d.JPEG" % i
        assert np.abs(np.array(region) - np.array(box)).max() <= 1e-12
    with open(str(tmp_path / "short.txt"), "w") as f:
        f.write("0,0,1,1,0.1,0.1\n")
    with pytest.raises(ValueError):
        data.load_frame_region(str(tmp_path / "short"))


def test_pixel_region_is_the_inverse_of_normalize_bbox():
    from ntmtrack import data, geometry as G
    rng = np.random.default_rng(2)
    for _ in range(20):
        W, H = int(rng.integers(32, 2000)), int(rng.integers(32, 2000))
        x, y, w, h = rng.uniform(0, W / 2), rng.uniform(0, H / 2), rng.uniform(1, W / 2), rng.uniform(1, H / 2)
        y1, x1, y2, x2 = G.normalize_bbox((W, H), (y, x, y + h, x + w))
        back = data.pixel_region((W, H), (x1, y1, x2 - x1, y2 - y1))
        assert np.abs(np.array(back) - np.array([x, y, w, h])).max() <= 1e-9 * max(W, H)
    assert data.pixel_region((101, 51), (0.5, 0.5, 0.25, 1.0)) == (50.0, 25.0, 25.0, 50.0)


def test_validation_clips_decode_lazily_and_start_normalised(tmp_path):
    from PIL import Image
    from ntmtrack import data
    rng = np.random.default_rng(4)
    root, W, H = tmp_path / "seqs" / "val_seq_0", 40, 24
    os.makedirs(str(root))
    boxes = [(0.2, 0.3, 0.25, 0.2), (0.25, 0.3, 0.25, 0.25), (0.3, 0.35, 0.2, 0.25)]
    pixels = rng.integers(0, 256, size=(3, H, W, 3), dtype=np.uint8)
    for i, box in enumerate(boxes):
        Image.fromarray(pixels[i]).save(str(tmp_path / ("f%d.png" % i)))
        write_record(str(root), "%06d" % i, box, "f%d.png" % i)
    _all, train, val = data.get_valid_sequences(str(tmp_path / "seqs"), 3)
    assert train == [] and val == [(str(root), ["000000", "000001", "000002"])]
    clips = data.validation_clips(val, image_root=str(tmp_path))
    assert len(clips) == 1
    clip = clips[0]
    assert callable(clip.frames) and clip.size == (H, W)
    assert np.abs(np.array(clip.init) - np.array(boxes[0])).max() <= 1e-12 and max(clip.init) < 1
    want = np.array(boxes) * np.array([W - 1, H - 1, W - 1, H - 1])
    assert clip.regions.shape == (3, 4) and np.abs(clip.regions - want).max() <= 1e-9
    frames = clip.frames()
    assert frames.shape == (3, H, W, 3) and (frames == pixels).all()


# ------------------------------------------------------------------------------------------- the arithmetic of result()
def test_result_arithmetic_on_a_hand_filled_table():
    import torch
    from ntmtrack import evaluate as E
    iou_thr, dist_thr = [0.0, 0.5, 1.0], [10.0, 20.0]
    s = E.OverlapScores(4, iou_thr, dist_thr, device="cpu")
    assert s.table.shape == (4, E.SCORE_HEAD + 5) and (s.table[:, E.SCORE_FIRST_LOST] == -1).all()
    assert (s.table[:, [0, 1, 2, 3] + list(range(5, 10))] == 0).all()
    #          frames sum_iou sum_dist lost first_lost | iou > 0, > .5, > 1 | dist <= 10, <= 20
    rows = [[4, 2.0, 40.0, 1, 2, 3, 2, 0, 1, 3],
            [6, 4.5, 30.0, 0, -1, 6, 5, 0, 4, 6],
            [0, 0.0, 0.0, 0, -1, 0, 0, 0, 0, 0],              # a clip without a scored frame
            [2, 0.0, 100.0, 2, 0, 0, 0, 0, 0, 0]]
    s.table.copy_(torch.tensor(rows, dtype=torch.float64))
    r = s.result()
    c = r["clips"]
    assert c["frames"].tolist() == [4, 6, 0, 2] and c["lost"].tolist() == [1, 0, 0, 2] and c["first_lost"].tolist() == [2, -1, -1, 0]
    np.testing.assert_array_equal(c["mean_overlap"], [0.5, 0.75, np.nan, 0.0])
    np.testing.assert_array_equal(c["mean_centre_error"], [10.0, 5.0, np.nan, 50.0])
    assert c["success"].shape == (4, 3) and c["precision"].shape == (4, 2)
    np.testing.assert_array_equal(c["success"][0], [0.75, 0.5, 0.0])
    np.testing.assert_array_equal(c["precision"][1], [4 / 6, 1.0])
    assert np.isnan(c["success"][2]).all() and np.isnan(c["precision"][2]).all()
    assert r["frames"] == 12 and r["clips_scored"] == 3 and r["clips_without_frames"] == 1
    assert r["mean_overlap_frames"] == 6.5 / 12
    assert r["mean_overlap_clips"] == pytest.approx((0.5 + 0.75 + 0.0) / 3, abs=1e-15)
    np.testing.assert_array_equal(r["success_curve"], [9 / 12, 7 / 12, 0.0])
    assert r["success_auc"] == pytest.approx((9 + 7) / 12 / 3, abs=1e-15)
    np.testing.assert_array_equal(r["precision_curve"], [5 / 12, 9 / 12])
    assert r["precision_20px"] == 9 / 12
    assert r["lost"] == 3 and r["clips_never_lost"] == 1
    # no 20 px threshold: no figure
    assert np.isnan(E.summarize(np.array(rows)[:, :9], iou_thr, [10.0])["precision_20px"])


def test_overlap_scores_refuses_too_many_thresholds():
    from ntmtrack import evaluate as E
    with pytest.raises(ValueError):
        E.OverlapScores(3, np.linspace(0, 1, E.SCORE_MAX_THRESHOLDS + 1), device="cpu")
    with pytest.raises(ValueError):
        E.OverlapScores(0, device="cpu")


def test_lazy_clips_without_a_size_are_probed_and_not_kept():
    """Grouping by frame size needs a size: a callable clip without one is decoded for its shape and dropped again, so building
    a Validation does not leave the whole set decoded in memory; a clip that names its size is not decoded at all."""
    from ntmtrack import evaluate as E
    calls = []

    def lazy(i, h, w):
        def frames():
            calls.append(i)
            return np.zeros((3, h, w, 3), dtype=np.uint8)
        return frames
    regions = np.tile(np.array([4.0, 4.0, 8.0, 8.0]), (3, 1))
    clips = [E.Clip(lazy(0, 16, 24), regions), E.Clip(lazy(1, 32, 24), regions), E.Clip(lazy(2, 16, 24), regions, size=(16, 24)),
             {"frames": np.zeros((3, 32, 24, 3), dtype=np.uint8), "regions": regions}]
    v = E.Validation(None, clips, 2, 2, device="cpu")
    assert calls == [0, 1] and [c.source.held for c in v.classes] == [{}, {}]
    assert [(c.size, c.members) for c in v.classes] == [((16, 24), [0, 2]), ((32, 24), [1, 3])]


@pytest.mark.parametrize("float_clip", [None, 2])
def test_array_source_builds_every_round_on_the_host(float_clip):
    """The host half of the array source (NumPy only: no device): over the whole schedule every active cell of the [T,B,H,W,3]
    block holds its clip's frame and every inactive one zeros, the starting frames are frame 0 of the clips reset, in reset
    order, a clip is held from its reset to the round that hands out its last frame, and a callable is called once when its
    clip is scheduled (and once before, for its size, when it names none).  Frame k of clip i is filled with 16 i + k.  A round
    that involves a float clip is float32, any other stays uint8."""
    from ntmtrack import evaluate as E
    lengths, H, W, B, T = [3, 2, 6, 4, 5], 8, 12, 2, 2
    calls = []

    def frames_of(i, dtype=np.uint8):
        return np.stack([np.full((H, W, 3), 16 * i + k, dtype=dtype) for k in range(lengths[i])])

    def lazy(i):
        return lambda: calls.append(i) or frames_of(i)
    regions = [np.tile(np.array([2.0, 2.0, 4.0, 4.0]), (n, 1)) for n in lengths]
    clips = [E.Clip(frames_of(0), regions[0]), E.Clip(lazy(1), regions[1], size=(H, W)),
             E.Clip(frames_of(2, np.uint8 if float_clip is None else np.float64), regions[2]), E.Clip(lazy(3), regions[3]),
             E.Clip(frames_of(4), regions[4])]
    v = E.Validation(None, clips, B, T, device="cpu")
    (cls,) = v.classes
    assert calls == [3] and cls.size == (H, W) and cls.source.held == {}
    dtype_with = lambda members: np.float32 if float_clip in members else np.uint8
    rounds = 0
    for rnd in E.ClipSchedule(lengths, B, T):
        ids = cls.ids(rnd)
        assert ids.tolist() == rnd.clip_of.tolist()
        firsts, frames = cls.source.host_round(rnd, ids)
        assert frames.shape == (T, B, H, W, 3) and frames.dtype == dtype_with(ids.tolist())
        left = set()
        for b in range(B):
            for t in range(T):
                assert (frames[t, b] == (16 * ids[b] + rnd.frame_index[t, b] if rnd.active[t, b] else 0)).all()
            n = int(rnd.active[:, b].sum())
            if n and rnd.frame_index[n - 1, b] + 1 < lengths[ids[b]]:
                left.add(int(ids[b]))
        assert set(cls.source.held) == left                         # gone with the round that hands out its last frame
        if rnd.resets:
            new = [c for _s, c in rnd.resets]
            assert firsts.shape == (len(new), H, W, 3) and firsts.dtype == dtype_with(new)
            assert all((f == 16 * c).all() for f, c in zip(firsts, new))
        else:
            assert firsts is None
        rounds += 1
    assert rounds == 5 and cls.source.held == {} and calls == [3, 1, 3]
