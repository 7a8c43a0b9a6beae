"""CPU: the C ABI of the mask ground truth (ntk_track_mask_bounds, ntk_track_mask_overlaps, ntk_track_overlap_scores_mask,
ntk_track_supervise_mask) is exported and bound, refuses null pointers and bad sizes on the host before anything is launched (no
GPU is needed: a refused call never reaches the device), and the header's NTK_MASK_* constants are the ones Python uses."""
import ctypes
import os
import re

import pytest

ONE = ctypes.c_void_p(16)                       # non-null, aligned, never dereferenced: the checks fire first
PLAN, JUDGE = 0, 1
P, I, D = ctypes.c_void_p, ctypes.c_int, ctypes.c_double


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


def bounds(L, cells=ONE, rle=ONE, n_rle=40, n=3, rects=ONE, area=ONE):
    return L.ntk_track_mask_bounds(cells, rle, n_rle, n, rects, area, None)


def overlaps(L, regions=ONE, cells=ONE, rle=ONE, n_rle=40, n=3, overlap=ONE):
    return L.ntk_track_mask_overlaps(regions, cells, rle, n_rle, n, overlap, None)


def scores(L, regions=ONE, rects=ONE, overlap=ONE, active=None, clip_of=ONE, T=2, B=3, n_clips=4, iou_thr=ONE, n_iou=21, dist_thr=ONE,
           n_dist=51, table=ONE, frame_iou=None):
    return L.ntk_track_overlap_scores_mask(regions, rects, overlap, active, clip_of, T, B, n_clips, iou_thr, n_iou, dist_thr, n_dist,
                                           table, frame_iou, None)


def supervise(L, phase=PLAN, regions=ONE, rects=ONE, overlap=ONE, active=None, clip_of=ONE, B=3, n_clips=4, skip=5, burn_in=10,
              failure_overlap=0.0, state=ONE, table=ONE, track=ONE, restart=ONE, codes=None, frame_iou=None):
    return L.ntk_track_supervise_mask(phase, regions, rects, overlap, active, clip_of, B, n_clips, skip, burn_in, failure_overlap,
                                      state, table, track, restart, codes, frame_iou, None)


def test_symbols_are_exported_and_bound(L):
    from ntmtrack import _lib
    for name, nargs in (("ntk_track_mask_bounds", 7), ("ntk_track_mask_overlaps", 7), ("ntk_track_overlap_scores_mask", 15),
                        ("ntk_track_supervise_mask", 18)):
        assert hasattr(L, name), "libntmtrack_hip.so does not export %s" % name
        assert name in _lib.exported_symbols()
        assert len(getattr(L, name).argtypes) == nargs
    assert L.ntk_track_mask_bounds.argtypes == [P, P, I, I, P, P, P]
    assert L.ntk_track_mask_overlaps.argtypes == [P, P, P, I, I, P, P]


def test_the_table_entries_take_the_siblings_lists_with_gt_as_rects_and_overlap(L):
    """The contract: the argument lists of ntk_track_overlap_scores and ntk_track_supervise, ``gt`` replaced by ``rects`` and
    ``overlap`` (two pointers where there was one)."""
    for mask, sibling, gt_at in ((L.ntk_track_overlap_scores_mask, L.ntk_track_overlap_scores, 1),
                                 (L.ntk_track_supervise_mask, L.ntk_track_supervise, 2)):
        sib = list(sibling.argtypes)
        assert sib[gt_at] == P
        assert list(mask.argtypes) == sib[:gt_at] + [P, P] + sib[gt_at + 1:]
    assert list(L.ntk_track_supervise_mask.argtypes) == [I, P, P, P, P, P, I, I, I, I, D, P, P, P, P, P, P, P]
    assert L.ntk_track_supervise_mask.restype == I and L.ntk_track_overlap_scores_mask.restype == I


@pytest.mark.parametrize("arg", ["cells", "rle", "rects", "area"])
def test_bounds_refuses_null_pointers(L, arg):
    assert bounds(L, **{arg: None}) == -2 and b"ntk_track_mask_bounds" in L.ntk_last_error()


@pytest.mark.parametrize("arg", ["regions", "cells", "rle", "overlap"])
def test_overlaps_refuses_null_pointers(L, arg):
    assert overlaps(L, **{arg: None}) == -2 and b"ntk_track_mask_overlaps" in L.ntk_last_error()


@pytest.mark.parametrize("call,name", [(bounds, b"ntk_track_mask_bounds"), (overlaps, b"ntk_track_mask_overlaps")])
@pytest.mark.parametrize("kw,named", [({"n": 0}, b"n=0"), ({"n": -1}, b"n=-1"), ({"n": -70}, b"n=-70"), ({"n_rle": -1}, b"n_rle=-1"),
                                      ({"n_rle": -2 ** 31}, b"n_rle=-2147483648")])
def test_mask_entries_refuse_bad_sizes_and_name_the_value(L, call, name, kw, named):
    assert call(L, **kw) == -1
    assert named in L.ntk_last_error() and name in L.ntk_last_error()


@pytest.mark.parametrize("arg", ["regions", "rects", "overlap", "clip_of", "table"])
def test_scores_refuses_null_pointers(L, arg):
    assert scores(L, **{arg: None}) == -2 and b"ntk_track_overlap_scores_mask" in L.ntk_last_error()


@pytest.mark.parametrize("kw,named", [({"B": 0}, b"B=0"), ({"B": 65536}, b"B=65536"), ({"B": -2}, b"B=-2"),
                                      ({"T": 0}, b"T=0"), ({"T": -1}, b"T=-1"),
                                      ({"n_clips": 0}, b"n_clips=0"), ({"n_clips": -3}, b"n_clips=-3"),
                                      ({"n_iou": -1}, b"n_iou=-1"), ({"n_iou": 257}, b"n_iou=257"),
                                      ({"n_dist": -1}, b"n_dist=-1"), ({"n_dist": 257}, b"n_dist=257"),
                                      ({"iou_thr": None}, b"iou_thr is null"), ({"dist_thr": None}, b"dist_thr is null")])
def test_scores_refuses_bad_sizes_and_names_the_value(L, kw, named):
    assert scores(L, **kw) == -1
    assert named in L.ntk_last_error() and b"ntk_track_overlap_scores_mask" in L.ntk_last_error()


@pytest.mark.parametrize("phase,arg", [(PLAN, "rects"), (PLAN, "clip_of"), (PLAN, "state"), (PLAN, "table"), (PLAN, "track"),
                                       (PLAN, "restart"), (JUDGE, "regions"), (JUDGE, "rects"), (JUDGE, "overlap"),
                                       (JUDGE, "clip_of"), (JUDGE, "state"), (JUDGE, "table"), (JUDGE, "track")])
def test_supervise_refuses_null_pointers(L, phase, arg):
    assert supervise(L, phase=phase, **{arg: None}) == -2 and b"ntk_track_supervise_mask" in L.ntk_last_error()


@pytest.mark.parametrize("phase", [PLAN, JUDGE])
@pytest.mark.parametrize("kw,named", [({"skip": 0}, b"skip=0"), ({"skip": -1}, b"skip=-1"), ({"burn_in": -1}, b"burn_in=-1"),
                                      ({"B": 0}, b"B=0"), ({"B": 65536}, b"B=65536"), ({"n_clips": 0}, b"n_clips=0"),
                                      ({"n_clips": -3}, b"n_clips=-3"), ({"failure_overlap": -0.5}, b"failure_overlap=-0.5"),
                                      ({"failure_overlap": 1.0}, b"failure_overlap=1")])
def test_supervise_refuses_bad_sizes_and_names_the_value(L, phase, kw, named):
    assert supervise(L, phase=phase, **kw) == -1
    assert named in L.ntk_last_error() and b"ntk_track_supervise_mask" in L.ntk_last_error()


@pytest.mark.parametrize("phase", [2, -1])
def test_supervise_refuses_a_phase_other_than_the_two(L, phase):
    assert supervise(L, phase=phase) == -1
    assert ("phase=%d" % phase).encode() in L.ntk_last_error()


def test_the_constants_of_the_header_are_the_ones_python_uses():
    from ntmtrack import evaluate as E, online
    import mask_util as M
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")).read()
    d = dict(re.findall(r"#define (NTK_MASK_[A-Z_]+)\s+(\S+(?: << \d+\))?)", hdr))
    assert d == {"NTK_MASK_CELL_INTS": "6", "NTK_MASK_OVERLAP_DOUBLES": "3", "NTK_MASK_MAX_PIXELS": "(1 << 30)"}
    assert (E.MASK_CELL_INTS, E.MASK_OVERLAP_DOUBLES, E.MASK_MAX_PIXELS) == (6, 3, 1 << 30)
    assert (M.CELL_INTS, M.OVERLAP_DOUBLES, M.MAX_PIXELS) == (6, 3, 1 << 30) and online.MASK_OVERLAP_DOUBLES == 3
    # the header says whose rules these are
    assert "THE RULES BELOW ARE THE CONTRACT" in hdr and "modelled on the" in hdr
    assert "RASTERISES A FRACTIONAL RECTANGLE IS THE PROJECT'S OWN" in hdr
