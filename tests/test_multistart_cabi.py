"""CPU: the C ABI of the multi-start protocol (ntk_track_multistart, _poly, _mask, ntk_track_eao_curve) is exported and bound,
refuses null pointers and bad sizes on the host before anything is launched (no GPU is needed: a refused call never reaches the
device), and the header's NTK_MS_* constants are the ones Python and the restatement use."""
import ctypes
import os
import re

import pytest

ONE = ctypes.c_void_p(16)                       # non-null, aligned, never dereferenced: the checks fire first
ENTRIES = ["ntk_track_multistart", "ntk_track_multistart_poly", "ntk_track_multistart_mask"]


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


def multistart(L, entry, regions=ONE, gt=ONE, overlap=ONE, active=None, clip_of=ONE, T=3, B=5, n_runs=4, failure_overlap=0.1,
               patience=10, table=ONE, trace_first=ONE, trace=ONE, frame_iou=None):
    truth = (gt, overlap) if entry.endswith("_mask") else (gt,)
    return getattr(L, entry)(regions, *truth, active, clip_of, T, B, n_runs, failure_overlap, patience, table, trace_first, trace,
                             frame_iou, None)


def eao(L, table=ONE, trace_first=ONE, trace=ONE, n_runs=4, n_max=8, prefix=ONE, curve=ONE):
    return L.ntk_track_eao_curve(table, trace_first, trace, n_runs, n_max, prefix, curve, None)


def test_symbols_are_exported_bound_and_declared(L):
    from ntmtrack import _lib
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")).read()
    for name, nargs in (("ntk_track_multistart", 14), ("ntk_track_multistart_poly", 14), ("ntk_track_multistart_mask", 15),
                        ("ntk_track_eao_curve", 8)):
        assert hasattr(L, name), "libntmtrack_hip.so does not export %s" % name
        assert name in _lib.exported_symbols()
        assert len(getattr(L, name).argtypes) == nargs
        assert re.search(r"^int %s\(" % name, hdr, re.M), "%s is not declared in include/ntmtrack.h" % name


@pytest.mark.parametrize("entry,arg", [(e, a) for e in ENTRIES for a in ["regions", "gt", "overlap", "clip_of", "table", "trace_first",
                                                                          "trace"] if a != "overlap" or e.endswith("_mask")])
def test_multistart_refuses_null_pointers(L, entry, arg):
    assert multistart(L, entry, **{arg: None}) == -2
    assert entry.encode() in L.ntk_last_error()


@pytest.mark.parametrize("entry", ENTRIES)
@pytest.mark.parametrize("kw,named", [({"T": 0}, b"T=0"), ({"T": -2}, b"T=-2"), ({"B": 0}, b"B=0"), ({"B": 65536}, b"B=65536"),
                                      ({"n_runs": 0}, b"n_runs=0"), ({"n_runs": -3}, b"n_runs=-3"),
                                      ({"patience": -1}, b"patience=-1"), ({"failure_overlap": -0.5}, b"failure_overlap=-0.5"),
                                      ({"failure_overlap": 1.0}, b"failure_overlap=1"),
                                      ({"failure_overlap": float("nan")}, b"failure_overlap=nan")])
def test_multistart_refuses_bad_sizes_and_names_the_value(L, entry, kw, named):
    assert multistart(L, entry, **kw) == -1
    assert named in L.ntk_last_error() and entry.encode() in L.ntk_last_error()


@pytest.mark.parametrize("arg", ["table", "trace_first", "trace", "prefix", "curve"])
def test_eao_curve_refuses_null_pointers(L, arg):
    assert eao(L, **{arg: None}) == -2


@pytest.mark.parametrize("kw,named", [({"n_runs": 0}, b"n_runs=0"), ({"n_runs": -1}, b"n_runs=-1"), ({"n_max": 0}, b"n_max=0"),
                                      ({"n_max": -5}, b"n_max=-5")])
def test_eao_curve_refuses_bad_sizes_and_names_the_value(L, kw, named):
    assert eao(L, **kw) == -1
    assert named in L.ntk_last_error()


def test_the_constants_of_the_header_are_the_ones_python_and_the_restatement_use():
    from ntmtrack import evaluate as E
    import multistart_util as M
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")).read()
    d = {k: int(v) for k, v in re.findall(r"#define (NTK_MS_[A-Z_]+)\s+(\d+)", hdr)}
    assert d == {"NTK_MS_FRAMES": E.MS_FRAMES, "NTK_MS_TRACKED": E.MS_TRACKED, "NTK_MS_SUM_IOU": E.MS_SUM_IOU,
                 "NTK_MS_FAILED": E.MS_FAILED, "NTK_MS_LOW": E.MS_LOW, "NTK_MS_PENDING": E.MS_PENDING, "NTK_MS_HEAD": E.MS_HEAD}
    assert (M.FRAMES, M.TRACKED, M.SUM_IOU, M.FAILED, M.LOW, M.PENDING, M.HEAD) == \
        (E.MS_FRAMES, E.MS_TRACKED, E.MS_SUM_IOU, E.MS_FAILED, E.MS_LOW, E.MS_PENDING, E.MS_HEAD)
    assert sorted(d.values()) == list(range(7))
