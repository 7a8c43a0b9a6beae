"""CPU: the C ABI of the on-device overlap scores (ntk_track_overlap_scores) is exported and bound, refuses null pointers and
bad sizes on the host before anything is launched (no GPU is needed: a refused call never reaches the device), and the header's
row layout is the one Python uses."""
import ctypes
import os
import re

import pytest

ONE = ctypes.c_void_p(16)                       # non-null, aligned, never dereferenced: the checks fire first


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


def scores(L, regions=ONE, gt=ONE, active=None, clip_of=ONE, T=2, B=3, n_clips=4, iou_thr=ONE, n_iou=21, dist_thr=ONE, n_dist=51,
           table=ONE, frame_iou=None):
    return L.ntk_track_overlap_scores(regions, gt, active, clip_of, T, B, n_clips, iou_thr, n_iou, dist_thr, n_dist, table, frame_iou,
                                      None)


def test_symbol_is_exported_and_bound(L):
    from ntmtrack import _lib
    assert hasattr(L, "ntk_track_overlap_scores"), "libntmtrack_hip.so does not export ntk_track_overlap_scores"
    assert "ntk_track_overlap_scores" in _lib.exported_symbols()
    assert len(L.ntk_track_overlap_scores.argtypes) == 14


@pytest.mark.parametrize("arg", ["regions", "gt", "clip_of", "table"])
def test_refuses_null_pointers(L, arg):
    assert scores(L, **{arg: None}) == -2


@pytest.mark.parametrize("kw,named", [({"T": 0}, b"T=0"), ({"T": -2}, b"T=-2"), ({"B": 0}, b"B=0"), ({"B": -1}, b"B=-1"),
                                      ({"B": 65536}, b"B=65536"), ({"n_clips": 0}, b"n_clips=0"), ({"n_clips": -7}, b"n_clips=-7"),
                                      ({"n_iou": -1}, b"n_iou=-1"), ({"n_dist": -3}, b"n_dist=-3"),
                                      ({"n_iou": 257}, b"n_iou=257"), ({"n_dist": 1000}, b"n_dist=1000"),
                                      ({"iou_thr": None}, b"n_iou=21"), ({"dist_thr": None}, b"n_dist=51")])
def test_refuses_bad_sizes_and_names_the_value(L, kw, named):
    assert scores(L, **kw) == -1
    assert named in L.ntk_last_error()


def test_a_missing_threshold_array_is_named(L):
    assert scores(L, iou_thr=None) == -1 and b"iou_thr" in L.ntk_last_error()
    assert scores(L, dist_thr=None) == -1 and b"dist_thr" in L.ntk_last_error()


def test_the_row_layout_of_the_header_is_the_one_python_uses():
    from ntmtrack import evaluate
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")).read()
    d = {k: int(v) for k, v in re.findall(r"#define (NTK_SCORE_[A-Z_]+)\s+(\d+)", hdr)}
    assert d == {"NTK_SCORE_FRAMES": evaluate.SCORE_FRAMES, "NTK_SCORE_SUM_IOU": evaluate.SCORE_SUM_IOU,
                 "NTK_SCORE_SUM_DIST": evaluate.SCORE_SUM_DIST, "NTK_SCORE_LOST": evaluate.SCORE_LOST,
                 "NTK_SCORE_FIRST_LOST": evaluate.SCORE_FIRST_LOST, "NTK_SCORE_HEAD": evaluate.SCORE_HEAD,
                 "NTK_SCORE_MAX_THRESHOLDS": evaluate.SCORE_MAX_THRESHOLDS}
    assert [d["NTK_SCORE_" + k] for k in ("FRAMES", "SUM_IOU", "SUM_DIST", "LOST", "FIRST_LOST", "HEAD")] == [0, 1, 2, 3, 4, 5]
    import evaluate_util as U
    assert (U.FRAMES, U.SUM_IOU, U.SUM_DIST, U.LOST, U.FIRST_LOST, U.HEAD) == (0, 1, 2, 3, 4, 5)
