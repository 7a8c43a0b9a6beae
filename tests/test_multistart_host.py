"""CPU: the host half of the multi-start protocol -- which runs a clip has (evaluate.multistart_runs against the restatement's
anchors and against cases worked by hand), MaskRegions.take, the run clips of array, file and callable clips, and
summarize_multistart on a hand-made table."""
import numpy as np
import pytest

import multistart_util as M
from ntmtrack import evaluate as E


def rect_clip(L, absent=(), frames=None, **kw):
    regions = np.tile([10.0, 12.0, 20.0, 16.0], (L, 1)) + np.arange(L)[:, None]
    for k in absent:
        regions[k] = np.nan
    return E.Clip(np.zeros((L, 2, 2, 3), np.uint8) if frames is None else frames, regions, **kw)


def runs_of(clip, **kw):
    return [tuple(r[1:]) for r in E.multistart_runs([clip], **kw)[1].tolist()]


# ------------------------------------------------------------------------------------------------------------ 1. anchor rules
@pytest.mark.parametrize("L,spacing,absent,want", [
    (2, 50, (), [(0, 1, 2), (1, -1, 2)]),
    (5, 4, (), [(0, 1, 5), (4, -1, 5)]),                              # L = spacing + 1: the last anchor IS a multiple of spacing
    (8, 4, (), [(0, 1, 8), (4, -1, 5), (7, -1, 8)]),                  # L = 2 spacing: 3 frames ahead of 4, 4 behind: backward
    (9, 4, (), [(0, 1, 9), (4, 1, 5), (8, -1, 9)]),                   # the tie, 4 ahead and 4 behind: forward
    (9, 4, (0, 1), [(2, 1, 7), (4, 1, 5), (8, -1, 9)]),               # an absent anchor moved forward
    (9, 4, (8, 7), [(0, 1, 9), (4, 1, 5), (6, -1, 7)]),               # and backward
    (9, 4, (0, 1, 2, 3), [(4, 1, 5), (8, -1, 9)]),                    # moved onto another anchor: one run
    (6, 2, (1,), [(0, 1, 6), (2, 1, 4), (4, -1, 5), (5, -1, 6)]),
    (6, 3, (3, 2, 1), [(0, 1, 6), (5, -1, 6)]),                       # anchor 3 runs backward, moves to frame 0: 1 frame, dropped
    (4, 50, (0, 1, 2), [(3, -1, 4)]),                                 # anchor 0 moves to the last frame: 1 frame, dropped
])
def test_anchor_rules(L, spacing, absent, want):
    clip = rect_clip(L, absent)
    assert runs_of(clip, spacing=spacing) == want
    assert M.anchors(E.regions_present(clip.regions), spacing) == want


def test_an_all_absent_clip_yields_no_run_and_a_set_without_runs_is_refused():
    empty, full = rect_clip(6, range(6)), rect_clip(3)
    _clips, runs = E.multistart_runs([full, empty, full], spacing=4)
    assert runs.tolist() == [[0, 0, 1, 3], [0, 2, -1, 3], [2, 0, 1, 3], [2, 2, -1, 3]] and runs.dtype == np.int64
    with pytest.raises(ValueError, match="no run"):
        E.multistart_runs([empty], spacing=4)
    with pytest.raises(ValueError, match="spacing=0"):
        E.multistart_runs([full], spacing=0)


def test_explicit_anchors():
    clip = rect_clip(10, absent=(3,))
    assert runs_of(clip, anchors=[[7, 3, 3]]) == [(4, 1, 6), (7, -1, 8)]          # sorted, merged, L - 1 not added, 3 moved to 4
    assert M.anchors(E.regions_present(clip.regions), given=[7, 3, 3]) == [(4, 1, 6), (7, -1, 8)]
    with pytest.raises(ValueError, match="anchors"):
        E.multistart_runs([clip], anchors=[[10]])
    with pytest.raises(ValueError, match="anchor lists"):
        E.multistart_runs([clip, clip], anchors=[[0]])


def test_absence_follows_the_kind_of_ground_truth():
    poly = np.full((4, 8), np.nan)
    poly[0, :6] = (0, 0, 4, 0, 0, 3)                                  # a triangle
    poly[1, :6] = (0, 0, 4, 0, 8, 0)                                  # three points on a line: no area, absent
    poly[2] = (0, 0, 4, 0, 4, 3, 0, 3)
    poly[3, :4] = (0, 0, 4, 0)                                        # two vertices: absent
    assert E.regions_present(poly).tolist() == [True, False, True, False]
    masks = E.MaskRegions.from_lists([(2, 2, 3, 2, [1, 2]), None, (0, 0, 2, 2, [4]), (1, 1, 2, 2, [0, 4])])
    assert E.regions_present(masks).tolist() == [True, False, False, True]       # frame 2: counts without a pixel set
    assert E.regions_present(np.array([[1, 1, 2, 2], [1, 1, 0, 2], [1, np.inf, 2, 2.0]])).tolist() == [True, False, False]


# ------------------------------------------------------------------------------------------------------- 2. MaskRegions.take
def test_mask_regions_take_gives_the_frames_in_the_given_order():
    rng = np.random.default_rng(3)
    H, W = 9, 11
    dense = rng.random((6, H, W)) < 0.4
    dense[2] = False                                                  # an absent frame
    masks = E.MaskRegions.from_arrays(dense)
    for order in ([4, 3, 2, 1, 0], [2, 3, 4, 5], [5, 5, 0], [2], []):
        taken = masks.take(order)
        assert len(taken) == len(order) and taken.offsets[-1] == len(taken.counts)
        for k, i in enumerate(order):
            assert (taken.dense(k, H, W) == dense[i]).all() and (taken.dense(k, H, W) == masks.dense(i, H, W)).all()
            assert taken.frame(k)[:4] == masks.frame(i)[:4] and taken.frame(k)[4].tolist() == masks.frame(i)[4].tolist()
    with pytest.raises(ValueError):
        masks.take([6])


# ------------------------------------------------------------------------------------------------------------- 3. run clips
def numbered_frames(L):
    return np.arange(L, dtype=np.uint8)[:, None, None, None] * np.ones((1, 2, 2, 3), np.uint8)


def test_array_file_and_callable_clips_give_the_runs_frames_in_run_order():
    L = 7
    frames = numbered_frames(L)
    files = ["f%d.jpg" % k for k in range(L)]
    calls = []

    def decode():
        calls.append(1)
        return numbered_frames(L)
    init = np.array([0.1, 0.1, 0.2, 0.2])
    masks = E.MaskRegions.from_arrays(np.arange(L)[:, None, None] >= np.arange(3)[None, :, None] * np.ones((1, 1, 4)))
    for source in (frames, files, decode):
        for regions in (rect_clip(L).regions, masks):
            clip = E.Clip(source, regions, init, (2, 2))
            run_clips, runs = E.multistart_runs([clip], spacing=3)
            assert runs.tolist() == [[0, 0, 1, 7], [0, 3, 1, 4], [0, 6, -1, 7]]
            for rc, (_c, a, d, n) in zip(run_clips, runs.tolist()):
                order = list(range(a, L)) if d > 0 else list(range(a, -1, -1))
                assert len(order) == n and rc.size == (2, 2)
                assert (rc.init is init) == (a == 0 and d == 1) and (rc.init is None) != (a == 0 and d == 1)
                got = rc.frames() if callable(rc.frames) else rc.frames
                if source is files:
                    assert got == [files[k] for k in order]
                else:
                    assert np.asarray(got)[:, 0, 0, 0].tolist() == order
                    assert source is not frames or np.shares_memory(got, frames)           # a view, not a copy
                if regions is masks:
                    assert all(rc.regions.frame(k)[4].tolist() == masks.frame(i)[4].tolist() and
                               rc.regions.frame(k)[:4] == masks.frame(i)[:4] for k, i in enumerate(order))
                else:
                    assert (rc.regions == regions[order]).all()


def test_a_callable_clip_is_decoded_once_while_two_of_its_runs_are_alive():
    calls = []

    def decode():
        calls.append(1)
        return numbered_frames(6).astype(np.float64)                  # not uint8: kept as float32, once
    run_clips, _runs = E.multistart_runs([E.Clip(decode, rect_clip(6).regions, None, (2, 2))], spacing=5)
    assert len(run_clips) == 2 and not calls                          # nothing is decoded before a run is scheduled
    a = run_clips[0].frames()
    b = run_clips[1].frames()
    assert len(calls) == 1 and a.dtype == np.float32 and np.shares_memory(a, b)
    assert a[:, 0, 0, 0].tolist() == [0, 1, 2, 3, 4, 5] and b[:, 0, 0, 0].tolist() == [5, 4, 3, 2, 1, 0]
    del a
    assert run_clips[0].frames() is not None and len(calls) == 1      # the other run still holds the array
    del b
    run_clips[1].frames()
    assert len(calls) == 2                                            # both runs had ended: decoded again


# --------------------------------------------------------------------------------------------------- 4. summarize_multistart
def test_summarize_multistart_on_a_hand_made_table():
    #            FRAMES TRACKED SUM  FAILED LOW PENDING
    table = np.array([[4, 4, 2.0, 0, 0, 2.0],      # run 0, clip 0: unfailed, N = N_F = 4
                      [5, 2, 1.0, 1, 0, 1.0],      # run 1, clip 0: failed at ordinal 2
                      [3, 0, 0.0, 1, 0, 0.0],      # run 2, clip 1: failed at ordinal 0: N_F = 0, accuracy NaN
                      [0, 0, 0.0, 0, 0, 0.0],      # run 3, clip 1: N = 0: takes part in nothing
                      [3, 2, 1.5, 0, 1, 1.5625]],  # run 4, clip 3: a streak of 1 open at the end: forgiven, sum = PENDING
                     dtype=np.float64)
    runs = np.array([[0, 0, 1, 5], [0, 4, -1, 6], [1, 0, 1, 4], [1, 3, -1, 4], [3, 0, 1, 4]])
    curve = np.array([0.5, 0.25, np.nan, 0.125, np.nan, np.nan])
    res = E.summarize_multistart(table, runs, curve, (2, 5), n_clips=4)
    per = res["per_run"]
    assert per["clip"].tolist() == [0, 0, 1, 1, 3] and per["anchor"].tolist() == [0, 4, 0, 3, 0]
    assert per["direction"].tolist() == [1, -1, 1, -1, 1]
    assert per["frames"].tolist() == [4, 5, 3, 0, 3] and per["tracked"].tolist() == [4, 2, 0, 0, 3]
    assert per["failed"].tolist() == [False, True, True, False, False]
    np.testing.assert_array_equal(per["accuracy"], [0.5, 0.5, np.nan, np.nan, 1.5625 / 3])
    np.testing.assert_array_equal(per["robustness"], [1.0, 0.4, 0.0, np.nan, 1.0])
    assert res["clips"]["runs"].tolist() == [2, 2, 0, 1]
    np.testing.assert_array_equal(res["clips"]["accuracy"], [3.0 / 6, np.nan, np.nan, 1.5625 / 3])
    np.testing.assert_array_equal(res["clips"]["robustness"], [6.0 / 9, 0.0, np.nan, 1.0])
    assert res["accuracy"] == 4.5625 / 9 and res["robustness"] == 9.0 / 15
    assert res["failures"] == 2 and res["runs"] == 5 and res["runs_without_frames"] == 1 and res["clips_without_runs"] == 1
    assert res["eao"] == (0.25 + 0.125) / 2 and res["eao_points"] == 2 and res["eao_interval"] == (2, 5)
    assert res["eao_curve"] is not None and len(res["eao_curve"]) == 6
    empty = E.summarize_multistart(table, runs, curve, (5, 6), n_clips=4)             # S_n empty on the whole interval
    assert np.isnan(empty["eao"]) and empty["eao_points"] == 0
    for bad in ((0, 3), (4, 3), (2, 7)):
        with pytest.raises(ValueError):
            E.summarize_multistart(table, runs, curve, bad)


def test_validation_refuses_bad_multistart_arguments_before_it_touches_a_device():
    clip = rect_clip(4)
    for kw, named in (({"spacing": 0}, "spacing=0"), ({"patience": -1}, "patience=-1"), ({"failure_overlap": 1.0}, "failure_overlap=1"),
                      ({"failure_overlap": -0.25}, "failure_overlap=-0.25"), ({"eao_interval": (0, 5)}, r"eao_interval=\(0, 5\)"),
                      ({"eao_interval": (6, 5)}, r"eao_interval=\(6, 5\)")):
        with pytest.raises(ValueError, match=named):
            E.Validation(None, [clip], 2, 2, protocol="multistart", **kw)
    assert "multistart" in E.PROTOCOLS
