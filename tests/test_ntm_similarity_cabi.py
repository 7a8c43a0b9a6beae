"""CPU: the similarity argument of the NTM sequence kernels' C ABI (the eight *_sim entry points) and of the cell's constructor.

Mode 0 (as coded) answers exactly as the entries without the suffix; mode 1 (row-wise smooth cosine) never plans a wave-specialised
kernel and its launchers follow its plan; any other mode is refused before a pointer is looked at.  The shape grid and the fake-pointer
convention are those of tests/test_ntm_shapes_cabi.py, re-stated here: a direction the plan accepts passes every host-side check and
fails at the first device call (NTK_ERR_HIP) where no device is visible, which is why the launcher sweeps run only there."""
import ctypes
import itertools
import os
import re

import pytest
import torch

no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: runs only where no device is visible")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "ntmtrack.h")
ENTRIES = ("ntk_ntm_seq_plan_sim", "ntk_ntm_seq_fwd_sim", "ntk_ntm_seq_bwd_sim", "ntk_ntm_step_fwd_sim", "ntk_ntm_step_bwd_sim",
           "ntk_ntm_seq_deep_plan_sim", "ntk_ntm_seq_fwd_deep_sim", "ntk_ntm_seq_bwd_deep_sim")

NTK_ERR_BAD_SHAPE, NTK_ERR_UNSUPPORTED, NTK_ERR_HIP = -1, -3, -4
AS_CODED, SMOOTH = 0, 1
FWD, BWD = 1, 2                                                  # NTK_NTM_PLAN_FWD / _BWD
F_WS, F_FIX512, F_G768, F_G1024 = 1, 2, 3, 4                     # NTK_NTM_FWD_*
B_WS, B_FIX, B_G768, B_G1024 = 1, 2, 3, 4                        # NTK_NTM_BWD_*
P = ctypes.c_void_p(1 << 20)
BATCH, STEPS, DIN = 2, 3, 10

MEM_SIZE = (0, 64, 100, 128, 256, 512, 1024, 1088)
MEM_DIM = (0, 1, 8, 13, 20, 64, 100, 256, 257)
HEADS = ((0, 1), (1, 0), (1, 1), (2, 1), (4, 1), (4, 2), (8, 7), (8, 8))
HIDDEN = (0, 64, 77, 200, 256, 320, 340, 344, 960, 1000)
TRACKER = (128, 20, 4, 1, 200, 1, 2)                             # N, Md, R, Wh, hid, shift_range, O


def _grid():
    """(N, Md, R, Wh, hid, shift_range, O, write_first): the grid of tests/test_ntm_shapes_cabi.py."""
    for N, Md, (R, Wh), hid, sr, wf in itertools.product(MEM_SIZE, MEM_DIM, HEADS, HIDDEN, (1, 4), (0, 1)):
        yield N, Md, R, Wh, hid, sr, 2, wf
    for N, Md, (R, Wh), hid, (sr, O), wf in itertools.product((64, 128, 512), (8, 20), ((1, 1), (4, 1), (8, 7)), (64, 200, 320),
                                                                ((5, 2), (32, 2), (64, 2), (2, 2), (3, 3), (1, 0), (1, 3), (1, 4)), (0, 1)):
        yield N, Md, R, Wh, hid, sr, O, wf


def _lib():
    from ntmtrack import _lib
    return _lib.lib()


def _a4(v):
    return (v + 3) // 4 * 4


def _plan(L, shape, B=BATCH):
    N, Md, R, Wh, hid, sr, O, wf = shape
    v = [ctypes.c_int() for _ in range(4)]
    mask = L.ntk_ntm_seq_plan(B, N, Md, R, Wh, hid, sr, O, wf, _a4(R * Md + hid), _a4(hid), *[ctypes.byref(x) for x in v])
    return (mask,) + tuple(x.value for x in v)


def _plan_sim(L, shape, mode, B=BATCH):
    N, Md, R, Wh, hid, sr, O, wf = shape
    v = [ctypes.c_int() for _ in range(4)]
    mask = L.ntk_ntm_seq_plan_sim(B, N, Md, R, Wh, hid, sr, O, wf, mode, _a4(R * Md + hid), _a4(hid), *[ctypes.byref(x) for x in v])
    return (mask,) + tuple(x.value for x in v)


def _deep_plan(L, shape, layers, B=BATCH):
    N, Md, R, Wh, hid, sr, O, wf = shape
    v = [ctypes.c_int() for _ in range(4)]
    mask = L.ntk_ntm_seq_deep_plan(B, N, Md, R, Wh, hid, sr, O, layers, wf, *[ctypes.byref(x) for x in v])
    return (mask,) + tuple(x.value for x in v)


def _deep_plan_sim(L, shape, layers, mode, B=BATCH):
    N, Md, R, Wh, hid, sr, O, wf = shape
    v = [ctypes.c_int() for _ in range(4)]
    mask = L.ntk_ntm_seq_deep_plan_sim(B, N, Md, R, Wh, hid, sr, O, layers, wf, mode, *[ctypes.byref(x) for x in v])
    return (mask,) + tuple(x.value for x in v)


# the six launchers; p = the value every required pointer takes (a fake one, or None: "null buffers")
def _fwd(L, shape, mode, p=P, B=BATCH, S=STEPS):
    N, Md, R, Wh, hid, sr, O, wf = shape
    return L.ntk_ntm_seq_fwd_sim(B, S, N, Md, R, Wh, hid, sr, O, wf, mode, *([p] * 8), None, *([p] * 4), *([None] * 10), None)


def _bwd(L, shape, mode, p=P, B=BATCH, S=STEPS):
    N, Md, R, Wh, hid, sr, O, wf = shape
    return L.ntk_ntm_seq_bwd_sim(B, S, N, Md, R, Wh, hid, sr, O, wf, mode, p, _a4(R * Md + hid), p, _a4(hid), *([p] * 11),
                                 None, None, None, None, *([p] * 6), None)


def _step_fwd(L, shape, mode, p=P, B=BATCH):
    N, Md, R, Wh, hid, sr, O, wf = shape
    return L.ntk_ntm_step_fwd_sim(B, N, Md, R, Wh, hid, sr, O, wf, mode, *([p] * 8), None, *([p] * 4), *([None] * 10), None)


def _step_bwd(L, shape, mode, p=P, B=BATCH):
    N, Md, R, Wh, hid, sr, O, wf = shape
    return L.ntk_ntm_step_bwd_sim(B, N, Md, R, Wh, hid, sr, O, wf, mode, p, _a4(R * Md + hid), p, _a4(hid), *([p] * 11),
                                  None, None, None, None, *([p] * 6), None)


def _fwd_deep(L, shape, layers, mode, p=P, B=BATCH, S=STEPS):
    N, Md, R, Wh, hid, sr, O, wf = shape
    return L.ntk_ntm_seq_fwd_deep_sim(B, S, N, Md, R, Wh, hid, sr, O, layers, wf, mode, DIN, *([p] * 9), None, *([p] * 4),
                                      *([None] * 15), None)


def _bwd_deep(L, shape, layers, mode, p=P, B=BATCH, S=STEPS):
    N, Md, R, Wh, hid, sr, O, wf = shape
    return L.ntk_ntm_seq_bwd_deep_sim(B, S, N, Md, R, Wh, hid, sr, O, layers, wf, mode, p, p, _a4(hid), *([p] * 13),
                                      None, None, None, None, *([p] * 7), None)


def test_the_eight_entries_are_declared_and_exported():
    text = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    declared = set(re.findall(r"\b(ntk_[a-z0-9_]+)\s*\(", text))
    from ntmtrack import _lib
    L = _lib.lib()
    for name in ENTRIES:
        assert name in declared, "%s is not declared in include/ntmtrack.h" % name
        assert hasattr(L, name), "libntmtrack_hip.so does not export %s" % name
        assert name in _lib.exported_symbols(), "%s is not bound in _lib.py" % name
    assert re.search(r"#define\s+NTK_NTM_SIM_AS_CODED\s+0\b", text) and re.search(r"#define\s+NTK_NTM_SIM_SMOOTH_COSINE\s+1\b", text)


def test_mode_0_plans_as_the_entries_without_the_suffix():
    """Mask, kernel ids and threads, both directions, single-layer and deep, over the whole grid."""
    L = _lib()
    bad, n = [], 0
    for shape in _grid():
        n += 1
        if _plan_sim(L, shape, AS_CODED) != _plan(L, shape):
            bad.append("%s: %s against %s" % (shape, _plan_sim(L, shape, AS_CODED), _plan(L, shape)))
        if shape[5] == 4 and (shape[1] in (13, 100) or shape[4] in (256, 340)):     # the deep sweep's thinning of the second shift_range
            continue
        for layers in (2, 3, 4, 10):
            if _deep_plan_sim(L, shape, layers, AS_CODED) != _deep_plan(L, shape, layers):
                bad.append("%s L=%d: deep %s against %s" % (shape, layers, _deep_plan_sim(L, shape, layers, AS_CODED), _deep_plan(L, shape, layers)))
    assert n > 20000 and not bad, "%d of %d shapes differ:\n  %s" % (len(bad), n, "\n  ".join(bad[:40]))


def test_smooth_cosine_never_plans_a_wave_specialised_kernel():
    """No shape reports kernel id 1 in either direction; the tracker shape runs fixdims-512 / fix; away from the wave-specialised
    shapes and from the LDS bound the mode does not change which kernel a shape takes."""
    L = _lib()
    assert _plan(L, TRACKER + (0,)) == (FWD | BWD, F_WS, 768, B_WS, 768)
    assert _plan_sim(L, TRACKER + (0,), SMOOTH) == (FWD | BWD, F_FIX512, 512, B_FIX, 640)
    assert _plan_sim(L, TRACKER + (1,), SMOOTH) == (FWD | BWD, F_FIX512, 512, B_G768, 640)
    bad, seen_f, seen_b = [], set(), set()
    for shape in _grid():
        mask, fk, ft, bk, bt = _plan_sim(L, shape, SMOOTH)
        seen_f.add(fk)
        seen_b.add(bk)
        if fk == F_WS or bk == B_WS:
            bad.append("%s: smooth cosine plans ids %d / %d" % (shape, fk, bk))
        m0, fk0, ft0, bk0, bt0 = _plan(L, shape)
        # the normaliser takes N floats of LDS where it took Md, so a shape at the 160 KiB bound may run in one mode only (64 x 100,
        # hid 200, shift 4, write_first trains in smooth mode alone); where both modes run a direction, they run the same kernel
        both = mask & m0
        if (both & FWD and fk0 != F_WS and (fk, ft) != (fk0, ft0)) or (both & BWD and bk0 != B_WS and (bk, bt) != (bk0, bt0)):
            bad.append("%s: smooth %s, as coded %s" % (shape, (mask, fk, ft, bk, bt), (m0, fk0, ft0, bk0, bt0)))
    assert not bad, "\n  ".join(bad[:40])
    assert seen_f == {0, F_FIX512, F_G768, F_G1024} and seen_b == {0, B_FIX, B_G768, B_G1024}, (seen_f, seen_b)


@no_device
@pytest.mark.parametrize("mode", (AS_CODED, SMOOTH))
def test_launchers_follow_the_plan_of_their_mode(mode):
    """All six launchers against ntk_ntm_seq_plan_sim / ntk_ntm_seq_deep_plan_sim in the same mode (the step entries: the plan's
    answer for the sequence entries, S = 1)."""
    L = _lib()
    bad, n = [], 0

    def check(name, accepted, rc, shape, layers=0):
        msg = L.ntk_last_error() or b""
        if accepted and rc != NTK_ERR_HIP:
            bad.append("%s %s L=%d: the plan accepts it, the entry returned %d (%s)" % (name, shape, layers, rc, msg.decode()))
        elif not accepted and (rc not in (NTK_ERR_BAD_SHAPE, NTK_ERR_UNSUPPORTED) or not msg):
            bad.append("%s %s L=%d: the plan refuses it, the entry returned %d (%s)" % (name, shape, layers, rc, msg.decode()))

    for shape in _grid():
        if shape[5] == 4 and (shape[1] in (13, 100) or shape[4] in (256, 340)):
            continue
        n += 1
        mask = _plan_sim(L, shape, mode)[0]
        check("seq_fwd", bool(mask & FWD), _fwd(L, shape, mode), shape)
        check("seq_bwd", bool(mask & BWD), _bwd(L, shape, mode), shape)
        check("step_fwd", bool(mask & FWD), _step_fwd(L, shape, mode), shape)
        check("step_bwd", bool(mask & BWD), _step_bwd(L, shape, mode), shape)
        for layers in (2, 4):
            deep = _deep_plan_sim(L, shape, layers, mode)[0]
            if deep not in (0, 3):
                bad.append("%s L=%d: deep mask %d" % (shape, layers, deep))
            check("fwd_deep", deep == 3, _fwd_deep(L, shape, layers, mode), shape, layers)
            check("bwd_deep", deep == 3, _bwd_deep(L, shape, layers, mode), shape, layers)
    assert n > 10000 and not bad, "%d disagreements:\n  %s" % (len(bad), "\n  ".join(bad[:40]))


@pytest.mark.parametrize("mode", (2, -1))
def test_unknown_modes_are_refused_before_anything_else(mode):
    """NTK_ERR_UNSUPPORTED from all eight entries with a reason, on a shape every kernel takes and with every buffer null: the mode
    is checked before the pointers (which would give NTK_ERR_BAD_PTR) and nothing is dereferenced or launched."""
    L = _lib()
    shape = TRACKER + (0,)
    calls = {
        "ntk_ntm_seq_plan_sim": lambda: _plan_sim(L, shape, mode)[0],
        "ntk_ntm_seq_fwd_sim": lambda: _fwd(L, shape, mode, p=None),
        "ntk_ntm_seq_bwd_sim": lambda: _bwd(L, shape, mode, p=None),
        "ntk_ntm_step_fwd_sim": lambda: _step_fwd(L, shape, mode, p=None),
        "ntk_ntm_step_bwd_sim": lambda: _step_bwd(L, shape, mode, p=None),
        "ntk_ntm_seq_deep_plan_sim": lambda: _deep_plan_sim(L, shape, 2, mode)[0],
        "ntk_ntm_seq_fwd_deep_sim": lambda: _fwd_deep(L, shape, 2, mode, p=None),
        "ntk_ntm_seq_bwd_deep_sim": lambda: _bwd_deep(L, shape, 2, mode, p=None),
    }
    assert set(calls) == set(ENTRIES)
    for name in ENTRIES:
        rc = calls[name]()
        msg = L.ntk_last_error() or b""
        assert rc == NTK_ERR_UNSUPPORTED, "%s(similarity=%d) returned %d (%s)" % (name, mode, rc, msg.decode())
        assert b"similarity=%d" % mode in msg, (name, msg)
    # the known modes with the same null buffers get as far as the pointer check
    for m in (AS_CODED, SMOOTH):
        assert _fwd(L, shape, m, p=None) == _bwd(L, shape, m, p=None) == -2
        assert _fwd_deep(L, shape, 2, m, p=None) == _bwd_deep(L, shape, 2, m, p=None) == -2


def test_the_cell_refuses_an_unknown_similarity():
    from ntmtrack import _lib
    from ntmtrack.ntm import NTMCell, StackedNTMCell
    for layers in (1, 2):
        with pytest.raises(_lib.NtkError, match="cosine"):
            NTMCell(2, controller_num_layers=layers, similarity="cosine")
    with pytest.raises(_lib.NtkError):
        NTMCell(2, controller_num_layers=1, similarity=None)
    # the known values construct (no parameters yet: nothing touches a device), the default is as coded, a deep cell's top follows
    assert NTMCell(2, controller_num_layers=1).similarity == "as_coded"
    assert NTMCell(2, controller_num_layers=1, similarity="smooth_cosine").similarity == "smooth_cosine"
    deep = NTMCell(2, controller_num_layers=3, similarity="smooth_cosine")
    assert isinstance(deep, StackedNTMCell) and deep.similarity == deep.top.similarity == "smooth_cosine"
    assert NTMCell(2, controller_num_layers=3).top.similarity == "as_coded"
