"""CPU: the C ABI of the polygon ground truth (ntk_track_poly_bounds, ntk_track_overlap_scores_poly, ntk_track_supervise_poly) is
exported and bound, refuses null pointers and bad sizes on the host before anything is launched (no GPU is needed: a refused call
never reaches the device), and the header's NTK_POLY_* constants are the ones Python uses."""
import ctypes
import os
import re

import pytest

ONE = ctypes.c_void_p(16)                       # non-null, aligned, never dereferenced: the checks fire first
PLAN, JUDGE = 0, 1


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


def bounds(L, poly=ONE, n=3, rects=ONE):
    return L.ntk_track_poly_bounds(poly, n, rects, None)


def scores(L, regions=ONE, gt=ONE, active=None, clip_of=ONE, T=2, B=3, n_clips=4, iou_thr=ONE, n_iou=21, dist_thr=ONE, n_dist=51,
           table=ONE, frame_iou=None):
    return L.ntk_track_overlap_scores_poly(regions, gt, active, clip_of, T, B, n_clips, iou_thr, n_iou, dist_thr, n_dist, table,
                                           frame_iou, None)


def supervise(L, phase=PLAN, regions=ONE, gt=ONE, active=None, clip_of=ONE, B=3, n_clips=4, skip=5, burn_in=10,
              failure_overlap=0.0, state=ONE, table=ONE, track=ONE, restart=ONE, codes=None, frame_iou=None):
    return L.ntk_track_supervise_poly(phase, regions, gt, active, clip_of, B, n_clips, skip, burn_in, failure_overlap, state, table,
                                      track, restart, codes, frame_iou, None)


def test_symbols_are_exported_and_bound(L):
    from ntmtrack import _lib
    for name, nargs in (("ntk_track_poly_bounds", 4), ("ntk_track_overlap_scores_poly", 14), ("ntk_track_supervise_poly", 17)):
        assert hasattr(L, name), "libntmtrack_hip.so does not export %s" % name
        assert name in _lib.exported_symbols()
        assert len(getattr(L, name).argtypes) == nargs
    # the polygon entries take the argument lists of the rectangle entries
    assert L.ntk_track_overlap_scores_poly.argtypes == L.ntk_track_overlap_scores.argtypes
    assert L.ntk_track_supervise_poly.argtypes == L.ntk_track_supervise.argtypes


@pytest.mark.parametrize("arg", ["poly", "rects"])
def test_bounds_refuses_null_pointers(L, arg):
    assert bounds(L, **{arg: None}) == -2


@pytest.mark.parametrize("n", [0, -1, -70])
def test_bounds_refuses_bad_sizes_and_names_the_value(L, n):
    assert bounds(L, n=n) == -1
    assert ("n=%d" % n).encode() in L.ntk_last_error() and b"ntk_track_poly_bounds" in L.ntk_last_error()


@pytest.mark.parametrize("arg", ["regions", "gt", "clip_of", "table"])
def test_scores_refuses_null_pointers(L, arg):
    assert scores(L, **{arg: None}) == -2


@pytest.mark.parametrize("kw,named", [({"B": 0}, b"B=0"), ({"B": 65536}, b"B=65536"), ({"B": -2}, b"B=-2"),
                                      ({"T": 0}, b"T=0"), ({"T": -1}, b"T=-1"),
                                      ({"n_clips": 0}, b"n_clips=0"), ({"n_clips": -3}, b"n_clips=-3"),
                                      ({"n_iou": -1}, b"n_iou=-1"), ({"n_iou": 257}, b"n_iou=257"),
                                      ({"n_dist": -1}, b"n_dist=-1"), ({"n_dist": 257}, b"n_dist=257"),
                                      ({"iou_thr": None}, b"iou_thr is null"), ({"dist_thr": None}, b"dist_thr is null")])
def test_scores_refuses_bad_sizes_and_names_the_value(L, kw, named):
    assert scores(L, **kw) == -1
    assert named in L.ntk_last_error() and b"ntk_track_overlap_scores_poly" in L.ntk_last_error()


@pytest.mark.parametrize("phase,arg", [(PLAN, "gt"), (PLAN, "clip_of"), (PLAN, "state"), (PLAN, "table"), (PLAN, "track"),
                                       (PLAN, "restart"), (JUDGE, "regions"), (JUDGE, "gt"), (JUDGE, "clip_of"), (JUDGE, "state"),
                                       (JUDGE, "table"), (JUDGE, "track")])
def test_supervise_refuses_null_pointers(L, phase, arg):
    assert supervise(L, phase=phase, **{arg: None}) == -2


@pytest.mark.parametrize("phase", [PLAN, JUDGE])
@pytest.mark.parametrize("kw,named", [({"skip": 0}, b"skip=0"), ({"skip": -1}, b"skip=-1"), ({"burn_in": -1}, b"burn_in=-1"),
                                      ({"B": 0}, b"B=0"), ({"B": 65536}, b"B=65536"), ({"n_clips": 0}, b"n_clips=0"),
                                      ({"n_clips": -3}, b"n_clips=-3"), ({"failure_overlap": -0.5}, b"failure_overlap=-0.5"),
                                      ({"failure_overlap": 1.0}, b"failure_overlap=1")])
def test_supervise_refuses_bad_sizes_and_names_the_value(L, phase, kw, named):
    assert supervise(L, phase=phase, **kw) == -1
    assert named in L.ntk_last_error() and b"ntk_track_supervise_poly" in L.ntk_last_error()


@pytest.mark.parametrize("phase", [2, -1])
def test_supervise_refuses_a_phase_other_than_the_two(L, phase):
    assert supervise(L, phase=phase) == -1
    assert ("phase=%d" % phase).encode() in L.ntk_last_error()


def test_the_constants_of_the_header_are_the_ones_python_uses():
    from ntmtrack import evaluate as E, online
    import poly_util as P
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")).read()
    d = {k: int(v) for k, v in re.findall(r"#define (NTK_POLY_[A-Z_]+)\s+(\d+)", hdr)}
    assert d == {"NTK_POLY_MAX_POINTS": E.POLY_MAX_POINTS, "NTK_POLY_DOUBLES": E.POLY_DOUBLES}
    assert d["NTK_POLY_DOUBLES"] == 2 * d["NTK_POLY_MAX_POINTS"] == 16
    assert (P.MAX_POINTS, P.DOUBLES) == (E.POLY_MAX_POINTS, E.POLY_DOUBLES) and online.POLY_DOUBLES == E.POLY_DOUBLES
    # the header states the contract for simple polygons and the one difference from the reference's conversion
    assert "MUST BE SIMPLE" in hdr and "sys.float_info.min" in hdr
