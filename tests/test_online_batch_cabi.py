"""CPU: the C ABI of the batched online tracker (ntk_crop_and_resize_batch, ntk_track_boxes_update, ntk_select_rows) is
exported and bound, and refuses null pointers and non-positive sizes on the host, before anything is launched (no GPU is
needed: a refused call never reaches the device)."""
import ctypes

import pytest

NEW = ("ntk_crop_and_resize_batch", "ntk_track_boxes_update", "ntk_select_rows")
ONE = ctypes.c_void_p(16)                       # non-null, aligned, never dereferenced: the checks fire first


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


def crop(L, images=ONE, dtype=0, F=2, H=8, W=8, C=3, frame_of=ONE, boxes=ONE, mean=None, out=ONE, B=2, ch=4, cw=4):
    return L.ntk_crop_and_resize_batch(images, dtype, F, H, W, C, frame_of, boxes, mean, out, B, ch, cw, 0.0, None)


def boxes(L, logits=ONE, B=2, S=65, cg=8.0, bg=6.0, active=None, state=ONE, cb32=ONE, regions=ONE, offsets=ONE, frame=None):
    return L.ntk_track_boxes_update(logits, B, S, cg, bg, active, state, cb32, regions, offsets, frame, None)


def select(L, mask=ONE, a=ONE, b=ONE, out=ONE, B=2, n=8):
    return L.ntk_select_rows(mask, a, b, out, B, n, None)


def test_new_symbols_are_exported_and_bound(L):
    from ntmtrack import _lib
    for s in NEW:
        assert hasattr(L, s), "libntmtrack_hip.so does not export %s" % s
        assert s in _lib.exported_symbols()
        assert getattr(L, s).argtypes is not None


@pytest.mark.parametrize("arg", ["images", "frame_of", "boxes", "out"])
def test_crop_batch_refuses_null_pointers(L, arg):
    assert crop(L, **{arg: None}) == -2


@pytest.mark.parametrize("arg", ["logits", "state", "cb32", "regions", "offsets"])
def test_boxes_update_refuses_null_pointers(L, arg):
    assert boxes(L, **{arg: None}) == -2


@pytest.mark.parametrize("arg", ["mask", "a", "b", "out"])
def test_select_rows_refuses_null_pointers(L, arg):
    assert select(L, **{arg: None}) == -2


@pytest.mark.parametrize("kw,named", [({"B": 0}, b"B=0"), ({"B": -3}, b"B=-3"), ({"F": 0}, b"F=0"), ({"F": -1}, b"F=-1"),
                                      ({"C": 0}, b"C=0"), ({"ch": 0}, b"crop=0x4"), ({"cw": -2}, b"crop=4x-2"),
                                      ({"H": 0}, b"H=0"), ({"dtype": 2}, b"dtype=2"), ({"B": 65536}, b"B=65536")])
def test_crop_batch_refuses_bad_shapes_and_names_the_value(L, kw, named):
    assert crop(L, **kw) == -1
    assert named in L.ntk_last_error()


@pytest.mark.parametrize("kw,named", [({"B": 0}, b"B=0"), ({"S": 0}, b"S=0"), ({"S": -65}, b"S=-65"), ({"bg": 0.0}, b"bbox_grid=0"),
                                      ({"cg": -8.0}, b"cropbox_grid=-8")])
def test_boxes_update_refuses_bad_shapes_and_names_the_value(L, kw, named):
    assert boxes(L, **kw) == -1
    assert named in L.ntk_last_error()


@pytest.mark.parametrize("kw,named", [({"B": 0}, b"B=0"), ({"n": 0}, b"n=0"), ({"B": -1}, b"B=-1")])
def test_select_rows_refuses_bad_shapes_and_names_the_value(L, kw, named):
    assert select(L, **kw) == -1
    assert named in L.ntk_last_error()


def test_the_state_layout_of_the_header_is_the_one_python_uses():
    import os
    import re
    from ntmtrack import online
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")).read()
    d = dict(re.findall(r"#define (NTK_TRACK_STATE_[A-Z]+)\s+(\d+)", hdr))
    assert int(d["NTK_TRACK_STATE_DOUBLES"]) == online.STATE_DOUBLES == 10
    assert [int(d["NTK_TRACK_STATE_" + k]) for k in ("W", "H", "BBOX", "CROPBOX")] == [0, 1, 2, 6]
