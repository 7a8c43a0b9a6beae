"""CPU: the C ABI of the one-launch training input (ntk_frames_crop_batch) is declared, exported and bound, and refuses null
pointers and sizes outside its contract on the host, before anything is launched (no GPU is needed: a refused call never
reaches the device), naming the offending value in ntk_last_error."""
import ctypes
import os
import re

import pytest

NAME = "ntk_frames_crop_batch"
ONE = ctypes.c_void_p(16)                       # non-null, aligned, never dereferenced: the checks fire first
HEADER = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


def call(L, pixels=ONE, pixels_bytes=4096, table=ONE, boxes=ONE, mean=None, out=ONE, n=2, C=3, rh=36, rw=64, ch=24, cw=24, flip=0):
    return L.ntk_frames_crop_batch(pixels, pixels_bytes, table, boxes, mean, out, n, C, rh, rw, ch, cw, flip, 0.0, None)


def test_symbol_is_declared_exported_and_bound(L):
    from ntmtrack import _lib
    hdr = open(HEADER).read()
    assert re.search(r"^int %s\(" % NAME, hdr, re.M), "%s is not declared in include/ntmtrack.h" % NAME
    assert hasattr(L, NAME), "libntmtrack_hip.so does not export %s" % NAME
    assert NAME in _lib.exported_symbols()
    fn = getattr(L, NAME)
    assert fn.restype is ctypes.c_int and len(fn.argtypes) == 15
    assert fn.argtypes[1] is ctypes.c_longlong and fn.argtypes[13] is ctypes.c_float


def test_the_table_width_of_the_header_is_the_one_python_uses():
    from ntmtrack import data
    d = dict(re.findall(r"#define (NTK_FRAME_TABLE_COLS)\s+(\d+)", open(HEADER).read()))
    assert int(d["NTK_FRAME_TABLE_COLS"]) == data.FRAME_TABLE_COLS == 7


@pytest.mark.parametrize("arg", ["pixels", "table", "boxes", "out"])
def test_refuses_null_pointers(L, arg):
    assert call(L, **{arg: None}) == -2
    assert b"null" in L.ntk_last_error()


@pytest.mark.parametrize("kw,named", [
    ({"n": 0}, b"n=0"), ({"n": -1}, b"n=-1"), ({"n": 65536}, b"n=65536"),
    ({"C": 0}, b"C=0"), ({"C": 5}, b"C=5"), ({"C": -3}, b"C=-3"),
    ({"rh": 0}, b"resize=0x64"), ({"rw": -2}, b"resize=36x-2"),
    ({"ch": 0}, b"crop=0x24"), ({"cw": -1}, b"crop=24x-1"),
    ({"pixels_bytes": 0}, b"pixels_bytes=0"), ({"pixels_bytes": -7}, b"pixels_bytes=-7"),
])
def test_refuses_bad_shapes_and_names_the_value(L, kw, named):
    assert call(L, **kw) == -1
    assert named in L.ntk_last_error()


@pytest.mark.parametrize("ch,cw,C,named", [
    (46341, 46341, 1, b"crop=46341x46341 C=1"),                  # 46341^2 = 2^31 + 4633
    (32768, 16384, 4, b"crop=32768x16384 C=4"),                  # exactly 2^31
    (2147483392, 1, 1, b"crop=2147483392x1 C=1"),                # 2^31 - 256: the first refused count
])
def test_refuses_an_element_count_at_or_above_the_limit(L, ch, cw, C, named):
    assert call(L, ch=ch, cw=cw, C=C) == -1
    assert named in L.ntk_last_error()
