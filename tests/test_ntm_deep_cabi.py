"""CPU: the C entries of the deep-controller NTM kernels (ntk_ntm_seq_{fwd,bwd}_deep, the weight pack, the support query) are
declared and exported, and their host-side validation refuses bad arguments before any launch."""
import ctypes
import os
import re

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ntmtrack.h")
ENTRIES = ("ntk_ntm_seq_deep_supported", "ntk_ntm_seq_deep_plan", "ntk_ntm_seq_deep_packed_floats", "ntk_ntm_seq_deep_pack",
           "ntk_ntm_seq_fwd_deep", "ntk_ntm_seq_bwd_deep")
OK, BAD_SHAPE, BAD_PTR, UNSUPPORTED = 0, -1, -2, -3
TRACKER = (128, 20, 4, 1, 200, 1, 2)          # N, Md, R, Wh, hid, shift_range, O (direct_offset_output.py:21-27)


def _lib():
    from ntmtrack import _lib
    return _lib.lib()


def test_header_declares_and_library_exports_the_deep_entries():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    from ntmtrack import _lib
    L = _lib.lib()
    for name in ENTRIES:
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert hasattr(L, name), name
        assert name in _lib.exported_symbols(), name


def test_supported_answers_the_named_shapes_and_refuses_beyond_the_bound():
    L = _lib()
    N, Md, R, Wh, hid, sr, O = TRACKER
    for layers in (2, 3, 4):                                          # the tracker's shape
        assert L.ntk_ntm_seq_deep_supported(32, N, Md, R, Wh, hid, sr, O, layers) == 1, layers
    for layers in range(2, 11):                                       # the reference constructor's default (10 layers of 100)
        assert L.ntk_ntm_seq_deep_supported(4, 128, 20, 3, 3, 100, 1, 2, layers) == 1, layers
    assert L.ntk_ntm_seq_deep_supported(3, 64, 12, 2, 2, 24, 1, 3, 4) == 1          # the odd test shape
    assert L.ntk_ntm_seq_deep_supported(3, 64, 12, 2, 2, 24, 3, 3, 2) == 1          # shift_range 3
    # beyond the bound: one layer, every layer's state past the LDS, hidden not a multiple of 4, the single-layer limits
    assert L.ntk_ntm_seq_deep_supported(32, N, Md, R, Wh, hid, sr, O, 1) == 0
    assert L.ntk_ntm_seq_deep_supported(32, N, Md, R, Wh, hid, sr, O, 200) == 0
    assert b"LDS" in L.ntk_last_error()
    assert L.ntk_ntm_seq_deep_supported(32, N, Md, R, Wh, 202, sr, O, 2) == 0
    assert L.ntk_ntm_seq_deep_supported(32, 100, Md, R, Wh, hid, sr, O, 2) == 0     # mem_size % 64
    assert L.ntk_ntm_seq_deep_supported(32, N, Md, R, Wh, hid, 5, O, 2) == 0        # shift_range 5
    # the plan gives the same answers (mask 3 = forward and BPTT) and the workgroup sizes: 5 x 128 slots at the tracker's shape
    v = [ctypes.c_int() for _ in range(4)]
    for wf in (0, 1):
        assert L.ntk_ntm_seq_deep_plan(32, N, Md, R, Wh, hid, sr, O, 2, wf, *[ctypes.byref(x) for x in v]) == 3
        assert [x.value for x in v] == [1, 640, 1, 640]                             # NTK_NTM_DEEP_768 both ways
    assert L.ntk_ntm_seq_deep_plan(32, N, Md, R, Wh, hid, sr, O, 1, 0, *[ctypes.byref(x) for x in v]) == 0
    assert [x.value for x in v] == [0, 0, 0, 0] and b"L=1" in L.ntk_last_error()
    assert L.ntk_ntm_seq_deep_plan(32, N, Md, R, Wh, 202, sr, O, 2, 0, None, None, None, None) == 0


def _fwd(L, layers=2, N=128, hid=200, ptr=None, wf=None):
    one = ctypes.c_void_p(16) if ptr is None else ptr                # non-null, aligned, never dereferenced
    return L.ntk_ntm_seq_fwd_deep(2, 3, N, 20, 4, 1, hid, 1, 2, layers, 0, 514,
                                  one, one, one if wf is None else wf, one, one, one, one, one,
                                  one, None, one, one, one, one, *([None] * 15), None)


def _bwd(L, layers=2, N=128, hid=200, wb=None):
    one = ctypes.c_void_p(16)
    return L.ntk_ntm_seq_bwd_deep(2, 3, N, 20, 4, 1, hid, 1, 2, layers, 0, one if wb is None else wb, one, 200,
                                  *([one] * 13), None, None, None, None, *([one] * 7), None)


def test_host_validation_refuses_without_launching():
    L = _lib()
    # fewer than two layers
    assert _fwd(L, layers=1) == BAD_SHAPE and b"L=1" in L.ntk_last_error()
    assert _bwd(L, layers=1) == BAD_SHAPE
    assert L.ntk_ntm_seq_deep_pack(514, 4, 20, 200, 1, *([ctypes.c_void_p(16)] * 6), None) == BAD_SHAPE
    # null / misaligned weight pointers
    assert _fwd(L, wf=ctypes.c_void_p(0)) == BAD_PTR
    assert _fwd(L, wf=ctypes.c_void_p(20)) == BAD_PTR and b"aligned" in L.ntk_last_error()
    assert _bwd(L, wb=ctypes.c_void_p(0)) == BAD_PTR
    assert _bwd(L, wb=ctypes.c_void_p(24)) == BAD_PTR
    assert L.ntk_ntm_seq_deep_pack(514, 4, 20, 200, 2, None, *([ctypes.c_void_p(16)] * 5), None) == BAD_PTR
    assert L.ntk_ntm_seq_deep_pack(514, 4, 20, 200, 2, *([ctypes.c_void_p(16)] * 4), ctypes.c_void_p(20), ctypes.c_void_p(16), None) == BAD_PTR
    # unsupported shapes
    assert _fwd(L, N=100) == UNSUPPORTED
    assert _fwd(L, hid=202) == UNSUPPORTED and b"multiple of 4" in L.ntk_last_error()
    assert _fwd(L, layers=200) == UNSUPPORTED
    assert _bwd(L, hid=202) == UNSUPPORTED
    assert L.ntk_ntm_seq_deep_pack(514, 4, 20, 202, 2, *([ctypes.c_void_p(16)] * 6), None) == UNSUPPORTED


def test_packed_sizes_follow_the_header_formulas():
    L = _lib()
    n = [ctypes.c_size_t() for _ in range(3)]
    D, R, Md, hid, layers = 514, 4, 20, 200, 3
    assert L.ntk_ntm_seq_deep_packed_floats(D, R, Md, hid, layers, *[ctypes.byref(v) for v in n]) == OK
    a4 = lambda v: (v + 3) // 4 * 4
    RM = R * Md
    assert n[0].value == 4 * hid * a4(D)
    assert n[1].value == 4 * hid * (a4(RM + hid + 1) + (layers - 1) * a4(2 * hid + 1))
    assert n[2].value == 4 * hid * (a4(RM + hid) + (layers - 1) * 2 * hid)
    assert L.ntk_ntm_seq_deep_packed_floats(D, R, Md, hid, 1, *[ctypes.byref(v) for v in n]) == BAD_SHAPE
