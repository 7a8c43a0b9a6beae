"""CPU: the C ABI of the supervised protocol (ntk_track_restart_boxes, ntk_track_supervise) is exported and bound, refuses null
pointers and bad sizes on the host before anything is launched (no GPU is needed: a refused call never reaches the device), and
the header's NTK_SUP_* constants are the ones Python uses."""
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


def boxes(L, regions_in=ONE, restart=ONE, active=None, B=3, cropbox_grid=8.0, bbox_grid=6.0, sigma=2.0, gts_width=64, state=ONE,
          cropbox32=ONE, regions=ONE, offsets=ONE, frame=ONE, gts0=ONE, run_mask=None, move_mask=None):
    return L.ntk_track_restart_boxes(regions_in, restart, active, B, cropbox_grid, bbox_grid, sigma, gts_width, state, cropbox32,
                                     regions, offsets, frame, gts0, run_mask, move_mask, None)


def supervise(L, phase=PLAN, regions=ONE, gt=ONE, active=None, clip_of=ONE, B=3, n_clips=4, skip=5, burn_in=10,
              failure_overlap=0.0, state=ONE, table=ONE, track=ONE, restart=ONE, codes=None, frame_iou=None):
    return L.ntk_track_supervise(phase, regions, gt, active, clip_of, B, n_clips, skip, burn_in, failure_overlap, state, table, track,
                                 restart, codes, frame_iou, None)


def test_symbols_are_exported_and_bound(L):
    from ntmtrack import _lib
    for name, nargs in (("ntk_track_restart_boxes", 17), ("ntk_track_supervise", 17)):
        assert hasattr(L, name), "libntmtrack_hip.so does not export %s" % name
        assert name in _lib.exported_symbols()
        assert len(getattr(L, name).argtypes) == nargs


@pytest.mark.parametrize("arg", ["regions_in", "restart", "state", "cropbox32", "regions", "offsets", "frame", "gts0"])
def test_restart_boxes_refuses_null_pointers(L, arg):
    assert boxes(L, **{arg: None}) == -2


@pytest.mark.parametrize("kw,named", [({"B": 0}, b"B=0"), ({"B": -4}, b"B=-4"), ({"B": 65536}, b"B=65536"),
                                      ({"cropbox_grid": 0.0}, b"cropbox_grid=0"), ({"cropbox_grid": -8.0}, b"cropbox_grid=-8"),
                                      ({"bbox_grid": 0.0}, b"bbox_grid=0"), ({"bbox_grid": -6.0}, b"bbox_grid=-6"),
                                      ({"sigma": 0.0}, b"sigma=0"),
                                      ({"gts_width": 63}, b"gts_width=63"), ({"gts_width": 0}, b"gts_width=0"),
                                      ({"cropbox_grid": 8.5, "gts_width": 64}, b"cropbox_grid=8.5"),
                                      ({"cropbox_grid": 7.0}, b"gts_width=64")])
def test_restart_boxes_refuses_bad_sizes_and_names_the_value(L, kw, named):
    assert boxes(L, **kw) == -1
    assert named in L.ntk_last_error()


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
    assert named in L.ntk_last_error()


@pytest.mark.parametrize("phase", [2, -1, 7])
def test_supervise_refuses_a_phase_other_than_the_two(L, phase):
    assert supervise(L, phase=phase) == -1
    assert ("phase=%d" % phase).encode() in L.ntk_last_error()


def test_the_constants_of_the_header_are_the_ones_python_uses():
    from ntmtrack import evaluate as E
    import supervised_util as S
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")).read()
    d = {k: int(v.strip("()")) for k, v in re.findall(r"#define (NTK_SUP_[A-Z_]+)\s+(\(?-?\d+\)?)", hdr)}
    assert d == {"NTK_SUP_PLAN": E.SUP_PLAN, "NTK_SUP_JUDGE": E.SUP_JUDGE,
                 "NTK_SUP_STATE_INTS": E.SUP_STATE_INTS, "NTK_SUP_STATE_MODE": E.SUP_STATE_MODE,
                 "NTK_SUP_STATE_COUNTDOWN": E.SUP_STATE_COUNTDOWN, "NTK_SUP_STATE_SINCE": E.SUP_STATE_SINCE,
                 "NTK_SUP_MODE_TRACK": E.SUP_MODE_TRACK, "NTK_SUP_MODE_WAIT": E.SUP_MODE_WAIT,
                 "NTK_SUP_VALID": E.SUP_VALID, "NTK_SUP_SUM_IOU": E.SUP_SUM_IOU, "NTK_SUP_FAILURES": E.SUP_FAILURES,
                 "NTK_SUP_RESTARTS": E.SUP_RESTARTS, "NTK_SUP_TRACKED": E.SUP_TRACKED, "NTK_SUP_SKIPPED": E.SUP_SKIPPED,
                 "NTK_SUP_FIRST_FAILURE": E.SUP_FIRST_FAILURE, "NTK_SUP_HEAD": E.SUP_HEAD,
                 "NTK_SUP_CODE_INACTIVE": E.SUP_CODE_INACTIVE, "NTK_SUP_CODE_TRACKED": E.SUP_CODE_TRACKED,
                 "NTK_SUP_CODE_RESTART": E.SUP_CODE_RESTART, "NTK_SUP_CODE_FAILURE": E.SUP_CODE_FAILURE,
                 "NTK_SUP_CODE_SKIPPED": E.SUP_CODE_SKIPPED}
    assert (S.VALID, S.SUM_IOU, S.FAILURES, S.RESTARTS, S.TRACKED, S.SKIPPED, S.FIRST_FAILURE, S.HEAD) == \
        (E.SUP_VALID, E.SUP_SUM_IOU, E.SUP_FAILURES, E.SUP_RESTARTS, E.SUP_TRACKED, E.SUP_SKIPPED, E.SUP_FIRST_FAILURE, E.SUP_HEAD)
    assert (S.MODE, S.COUNTDOWN, S.SINCE, S.STATE_INTS) == (E.SUP_STATE_MODE, E.SUP_STATE_COUNTDOWN, E.SUP_STATE_SINCE, E.SUP_STATE_INTS)
    assert (S.TRACK, S.WAIT) == (E.SUP_MODE_TRACK, E.SUP_MODE_WAIT)
    assert (S.INACTIVE, S.TRACKED_CODE, S.RESTART, S.FAILURE, S.SKIP) == \
        (E.SUP_CODE_INACTIVE, E.SUP_CODE_TRACKED, E.SUP_CODE_RESTART, E.SUP_CODE_FAILURE, E.SUP_CODE_SKIPPED)
