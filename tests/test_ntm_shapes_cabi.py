"""CPU: the plan queries of the NTM sequence kernels (ntk_ntm_seq_plan, ntk_ntm_seq_deep_plan) agree with the four launchers over a grid
of cell shapes, out-of-range values included.

Every entry is called with fake pointers (non-null, 16-byte aligned, never dereferenced): a direction the plan accepts must pass
every host-side check and reach the device calls, which fail without a device (NTK_ERR_HIP); a direction the plan refuses must be
refused before them (NTK_ERR_BAD_SHAPE / NTK_ERR_UNSUPPORTED) with a reason in ntk_last_error().  With a device present a wrongly
accepted shape would launch against the fake pointers, so the file runs only where there is none.  Named anchors pin the plan to
shapes evaluated by hand from the launchers' arithmetic, so that it is not only compared with itself.
tests/test_ntm_shapes_gpu.py runs accepted shapes of every kernel id on the GPU."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: runs only where no device is visible")

NTK_ERR_BAD_SHAPE, NTK_ERR_UNSUPPORTED, NTK_ERR_HIP = -1, -3, -4
FWD, BWD = 1, 2                                                  # NTK_NTM_PLAN_FWD / _BWD
F_WS, F_FIX512, F_G768, F_G1024 = 1, 2, 3, 4                     # NTK_NTM_FWD_*
B_WS, B_FIX, B_G768, B_G1024 = 1, 2, 3, 4                        # NTK_NTM_BWD_*
D_768, D_1024 = 1, 2                                             # NTK_NTM_DEEP_*
P = ctypes.c_void_p(1 << 20)
BATCH, STEPS, DIN = 2, 3, 10

MEM_SIZE = (0, 64, 100, 128, 256, 512, 1024, 1088)
MEM_DIM = (0, 1, 8, 13, 20, 64, 100, 256, 257)
HEADS = ((0, 1), (1, 0), (1, 1), (2, 1), (4, 1), (4, 2), (8, 7), (8, 8))         # (R, Wh): no read / no write head, 15 and 16 heads
HIDDEN = (0, 64, 77, 200, 256, 320, 340, 344, 960, 1000)
TRACKER = (128, 20, 4, 1, 200, 1, 2)                             # N, Md, R, Wh, hid, shift_range, O


def _grid():
    """(N, Md, R, Wh, hid, shift_range, O, write_first): the full product of the four size axes at shift_range 1 and 4, then the
    edges of shift_range and output_dim (5: eleven taps; 32 / 64: a shift space that reaches mem_size 64 / 128; O = 0) over a
    thinner product."""
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


def _plan(L, shape, B=BATCH, ldkT=None, ldhT=None):
    N, Md, R, Wh, hid, sr, O, wf = shape
    v = [ctypes.c_int() for _ in range(4)]
    mask = L.ntk_ntm_seq_plan(B, N, Md, R, Wh, hid, sr, O, wf, _a4(R * Md + hid) if ldkT is None else ldkT,
                              _a4(hid) if ldhT is None else ldhT, *[ctypes.byref(x) for x in v])
    return (mask,) + tuple(x.value for x in v)


def _deep_plan(L, shape, layers, B=BATCH):
    N, Md, R, Wh, hid, sr, O, wf = shape
    v = [ctypes.c_int() for _ in range(4)]
    mask = L.ntk_ntm_seq_deep_plan(B, N, Md, R, Wh, hid, sr, O, layers, wf, *[ctypes.byref(x) for x in v])
    return (mask,) + tuple(x.value for x in v)


def _fwd(L, shape, B=BATCH, S=STEPS):
    N, Md, R, Wh, hid, sr, O, wf = shape
    return L.ntk_ntm_seq_fwd(B, S, N, Md, R, Wh, hid, sr, O, wf, *([P] * 8), None, *([P] * 4), *([None] * 10), None)


def _bwd(L, shape, B=BATCH, S=STEPS, ldkT=None, ldhT=None):
    N, Md, R, Wh, hid, sr, O, wf = shape
    return L.ntk_ntm_seq_bwd(B, S, N, Md, R, Wh, hid, sr, O, wf, P, _a4(R * Md + hid) if ldkT is None else ldkT, P,
                             _a4(hid) if ldhT is None else ldhT, *([P] * 11), None, None, None, None, *([P] * 6), None)


def _fwd_deep(L, shape, layers, B=BATCH, S=STEPS):
    N, Md, R, Wh, hid, sr, O, wf = shape
    return L.ntk_ntm_seq_fwd_deep(B, S, N, Md, R, Wh, hid, sr, O, layers, wf, DIN, *([P] * 9), None, *([P] * 4), *([None] * 15), None)


def _bwd_deep(L, shape, layers, B=BATCH, S=STEPS):
    N, Md, R, Wh, hid, sr, O, wf = shape
    return L.ntk_ntm_seq_bwd_deep(B, S, N, Md, R, Wh, hid, sr, O, layers, wf, P, P, _a4(hid), *([P] * 13), None, None, None, None,
                                  *([P] * 7), None)


class _Sweep(object):
    """Collects every disagreement between a plan and an entry; the failure lists them all."""

    def __init__(self, entry):
        self.entry, self.n, self.bad = entry, 0, []

    def check(self, accepted, rc, shape, **more):
        self.n += 1
        msg = _lib().ntk_last_error() or b""
        what = "N=%d Md=%d R=%d Wh=%d hid=%d shift=%d O=%d write_first=%d" % shape + "".join(" %s=%d" % kv for kv in more.items())
        if accepted and rc != NTK_ERR_HIP:
            self.bad.append("%s: the plan accepts it, the entry returned %d (%s)" % (what, rc, msg.decode()))
        elif not accepted and rc not in (NTK_ERR_BAD_SHAPE, NTK_ERR_UNSUPPORTED):
            self.bad.append("%s: the plan refuses it, the entry returned %d" % (what, rc))
        elif not accepted and not msg:
            self.bad.append("%s: refused with %d and no reason in ntk_last_error()" % (what, rc))

    def note(self, ok, text, shape, **more):
        self.n += 1
        if not ok:
            self.bad.append("N=%d Md=%d R=%d Wh=%d hid=%d shift=%d O=%d write_first=%d" % shape +
                            "".join(" %s=%d" % kv for kv in more.items()) + ": " + text)

    def verdict(self):
        assert self.n > 0
        print("%s: %d calls checked" % (self.entry, self.n))
        assert not self.bad, "%s: %d of %d checks disagree:\n  %s" % (self.entry, len(self.bad), self.n, "\n  ".join(self.bad))


def test_single_layer_entries_agree_with_the_plan():
    """ntk_ntm_seq_fwd and ntk_ntm_seq_bwd against their own bit of ntk_ntm_seq_plan; the BPTT's shapes are a subset of the
    forward's; the accepted shapes of the sweep reach every kernel id of both directions (the two forms behind the development
    switches are covered by test_development_switches_reach_the_plan_and_the_launch)."""
    L = _lib()
    fwd, bwd, sub = _Sweep("ntk_ntm_seq_fwd"), _Sweep("ntk_ntm_seq_bwd"), _Sweep("BPTT within forward")
    seen_f, seen_b, accepted = set(), set(), [0, 0]
    for shape in _grid():
        mask, fk, ft, bk, bt = _plan(L, shape)
        fwd.check(bool(mask & FWD), _fwd(L, shape), shape)
        bwd.check(bool(mask & BWD), _bwd(L, shape), shape)
        sub.note(not (mask & BWD) or bool(mask & FWD), "the BPTT takes a shape the forward refuses", shape)
        sub.note(bool(mask & FWD) == (fk != 0 and ft > 0) and bool(mask & BWD) == (bk != 0 and bt > 0),
                 "mask %d against kernel ids %d / %d and threads %d / %d" % (mask, fk, bk, ft, bt), shape)
        if mask & FWD:
            sub.note(ft % 64 == 0 and ft <= 1024 and (fk == F_G1024) == (ft > 768) or fk in (F_WS, F_FIX512), "forward threads %d, id %d" % (ft, fk), shape)
            seen_f.add(fk)
            accepted[0] += 1
        if mask & BWD:
            sub.note(bt % 64 == 0 and bt <= 1024 and (bk == B_G1024) == (bt > 768) or bk == B_WS, "BPTT threads %d, id %d" % (bt, bk), shape)
            seen_b.add(bk)
            accepted[1] += 1
    print("plan accepts %d shapes forward, %d in BPTT" % tuple(accepted))
    fwd.verdict()
    bwd.verdict()
    sub.verdict()
    assert seen_f == {F_WS, F_FIX512, F_G768, F_G1024}, seen_f
    assert seen_b == {B_WS, B_G768, B_G1024}, seen_b             # B_FIX: only under NTK_NTM_BWD_FORM=res


def test_batch_and_steps_of_zero_are_refused():
    L = _lib()
    sweep = _Sweep("B = 0 / S = 0")
    for shape in (TRACKER + (0,), TRACKER + (1,), (64, 8, 1, 1, 64, 1, 2, 0), (128, 20, 4, 1, 320, 1, 2, 0)):
        assert _plan(L, shape)[0] == FWD | BWD and _deep_plan(L, shape, 2)[0] == FWD | BWD
        sweep.check(False, _fwd(L, shape, S=0), shape, S=0)
        sweep.check(False, _bwd(L, shape, S=0), shape, S=0)
        sweep.check(False, _fwd_deep(L, shape, 2, S=0), shape, S=0, L=2)
        sweep.check(False, _bwd_deep(L, shape, 2, S=0), shape, S=0, L=2)
        sweep.note(_plan(L, shape, B=0)[0] == 0 and _deep_plan(L, shape, 2, B=0)[0] == 0, "a plan accepts B = 0", shape)
        sweep.check(False, _fwd(L, shape, B=0), shape, B=0)
        sweep.check(False, _bwd(L, shape, B=0), shape, B=0)
        sweep.check(False, _fwd_deep(L, shape, 2, B=0), shape, B=0, L=2)
        sweep.check(False, _bwd_deep(L, shape, 2, B=0), shape, B=0, L=2)
    sweep.verdict()


def test_leading_dimensions_of_the_bptt():
    """ldkT / ldhT: below K / hid or not a multiple of 4 is refused; wider ones are taken, but only 280 / 200 take the specialised
    kernels at the tracker shape; <= 0 stands for the smallest valid ones."""
    L = _lib()
    shape = TRACKER + (0,)
    assert _plan(L, shape, ldkT=0, ldhT=0) == _plan(L, shape, ldkT=280, ldhT=200) == (FWD | BWD, F_WS, 768, B_WS, 768)
    sweep = _Sweep("ntk_ntm_seq_bwd leading dimensions")
    for ldkT, ldhT, ok, kernel in ((280, 200, True, B_WS), (284, 200, True, B_G768), (280, 204, True, B_G768), (512, 256, True, B_G768),
                                   (276, 200, False, 0), (280, 196, False, 0), (282, 200, False, 0), (280, 202, False, 0)):
        mask, _fk, _ft, bk, bt = _plan(L, shape, ldkT=ldkT, ldhT=ldhT)
        sweep.note(bool(mask & BWD) == ok and bk == kernel and mask & FWD, "plan says mask %d kernel %d" % (mask, bk), shape, ldkT=ldkT, ldhT=ldhT)
        sweep.check(ok, _bwd(L, shape, ldkT=ldkT, ldhT=ldhT), shape, ldkT=ldkT, ldhT=ldhT)
    sweep.verdict()


def test_development_switches_reach_the_plan_and_the_launch(monkeypatch):
    """NTK_NTM_FWD_FORM=res / NTK_NTM_BWD_FORM=res (read per call) move the tracker shape from the wave-specialised kernels to the
    resident forms, in the plan and in the launchers alike; other shapes do not notice."""
    L = _lib()
    shape, other = TRACKER + (0,), (128, 20, 4, 2, 200, 1, 2, 0)
    before = _plan(L, other)
    assert _plan(L, shape) == (FWD | BWD, F_WS, 768, B_WS, 768)
    monkeypatch.setenv("NTK_NTM_FWD_FORM", "res")
    assert _plan(L, shape) == (FWD | BWD, F_FIX512, 512, B_WS, 768)
    monkeypatch.setenv("NTK_NTM_BWD_FORM", "res")
    assert _plan(L, shape) == (FWD | BWD, F_FIX512, 512, B_FIX, 640)
    assert _fwd(L, shape) == NTK_ERR_HIP and _bwd(L, shape) == NTK_ERR_HIP
    assert _plan(L, other) == before
    monkeypatch.delenv("NTK_NTM_FWD_FORM")
    assert _plan(L, shape) == (FWD | BWD, F_WS, 768, B_FIX, 640)
    monkeypatch.delenv("NTK_NTM_BWD_FORM")
    assert _plan(L, shape) == (FWD | BWD, F_WS, 768, B_WS, 768)


# Hand evaluation of the launchers (H = R + Wh, SS = 2 shift + 1, P = H Md + 3 H + H SS + 2 Wh Md, PP = align4(P + O), K = R Md + hid):
#   forward T = min(1024, round64(max(H N, 3 hid, hid + max(Md, 4), PP + Md, H Md + H + 1, (ceil(hid / 64) + 1) 64, (H + 1) 64)))
#   BPTT    T = round64(max(round64(max(H N, 3 hid, PP, K)), H Md + Md + 2 Wh Md)), refused above 1024
# (shape, write_first) -> (mask, forward id, forward threads, BPTT id, BPTT threads)
ANCHORS = [
    # the tracker: 5 x 128 = 640 threads of work; the wave-specialised kernels add stream waves (768 threads in the launch)
    (TRACKER, 0, (3, F_WS, 768, B_WS, 768)),
    (TRACKER, 1, (3, F_FIX512, 512, B_G768, 640)),
    ((128, 20, 4, 1, 200, 1, 3), 0, (3, F_G768, 640, B_G768, 640)),           # O = 3
    ((128, 20, 4, 1, 200, 2, 2), 0, (3, F_G768, 640, B_G768, 640)),           # shift_range 2
    ((128, 20, 4, 2, 200, 1, 2), 0, (3, F_G768, 768, B_G768, 768)),           # two write heads: 6 x 128
    ((128, 20, 4, 1, 320, 1, 2), 0, (3, F_G1024, 960, B_G1024, 960)),         # 3 hid = 960
    ((64, 4, 8, 7, 64, 1, 2), 0, (3, F_G1024, 1024, B_G1024, 960)),           # 15 heads: (H + 1) 64 forward, H N = 960 in the BPTT
    ((64, 100, 2, 2, 100, 1, 2), 0, (3, F_G1024, 960, B_G1024, 960)),         # P = 824, PP = 828: PP + Md = 928 forward, PP = 828 BPTT
    # forward only
    ((64, 100, 2, 2, 100, 1, 2), 1, (1, F_G1024, 960, 0, 0)),                 # write_first: a fifth N x (Md | 1) array, 181744 B of LDS
    ((512, 16, 1, 1, 256, 1, 4), 0, (1, F_G1024, 1024, 0, 0)),                # H N = 1024 fits the BPTT's threads, its LDS (203152 B) not
    ((1024, 8, 1, 1, 64, 1, 2), 0, (1, F_G1024, 1024, 0, 0)),                 # H N = 2048 > T forward; > 1024 refused in the BPTT
    ((256, 40, 3, 1, 200, 1, 2), 0, (1, F_G1024, 1024, 0, 0)),                # N Md = 10240 > 8 x 1024
    ((128, 20, 4, 1, 960, 1, 2), 0, (1, F_G1024, 1024, 0, 0)),                # 3 hid = 2880
    ((192, 13, 2, 1, 77, 1, 2), 0, (1, F_G768, 576, 0, 0)),                   # hid % 4; forward 3 x 192
    # neither
    ((512, 64, 1, 1, 128, 1, 2), 0, (0, 0, 0, 0, 0)),                         # forward state 165056 B of LDS
    ((128, 20, 4, 1, 200, 5, 2), 0, (0, 0, 0, 0, 0)),                         # eleven shift taps
    ((64, 8, 1, 1, 64, 32, 2), 0, (0, 0, 0, 0, 0)),                           # shift space 65 >= mem_size 64
    ((128, 20, 8, 8, 200, 1, 2), 0, (0, 0, 0, 0, 0)),                         # 16 heads
    ((128, 20, 4, 1, 1000, 1, 2), 0, (0, 0, 0, 0, 0)),                        # hidden above 960
    ((100, 20, 4, 1, 200, 1, 2), 0, (0, 0, 0, 0, 0)),                         # mem_size % 64
    ((1088, 8, 1, 1, 64, 1, 2), 0, (0, 0, 0, 0, 0)),
    ((128, 257, 1, 1, 64, 1, 2), 0, (0, 0, 0, 0, 0)),
]


def test_named_shapes_pin_the_plan():
    L = _lib()
    bad = []
    for shape, wf, want in ANCHORS:
        got = _plan(L, shape + (wf,))
        if got != want:
            bad.append("%s write_first=%d: plan %s, by hand %s" % (shape, wf, got, want))
        if want[0] != FWD | BWD and not L.ntk_last_error():
            bad.append("%s write_first=%d: refused without a reason" % (shape, wf))
    assert not bad, "\n  ".join(bad)
    # the reasons name the limit
    for shape, word in (((1024, 8, 1, 1, 64, 1, 2), b"heads*mem_size=2048"), ((192, 13, 2, 1, 77, 1, 2), b"multiple of 4"),
                        ((512, 64, 1, 1, 128, 1, 2), b"LDS"), ((512, 16, 1, 1, 256, 1, 4), b"LDS"), ((128, 20, 4, 1, 960, 1, 2), b"hidden=960")):
        assert _plan(L, shape + (0,))[0] != FWD | BWD
        assert word in L.ntk_last_error(), (shape, L.ntk_last_error())


# deep form: the forward's threads by the single-layer rule; Tb = round64(max(H N, 3 hid, PP, K, 2 hid, H Md + Md + 2 Wh Md))
DEEP_ANCHORS = [
    (TRACKER, 0, 2, (3, D_768, 640, D_768, 640)),
    (TRACKER, 1, 3, (3, D_768, 640, D_768, 640)),
    ((128, 20, 3, 3, 100, 1, 2), 0, 10, (3, D_768, 768, D_768, 768)),          # the reference constructor's default
    ((64, 4, 8, 7, 64, 1, 2), 0, 2, (3, D_1024, 1024, D_1024, 960)),           # Tf 1024 by (H + 1) 64
    ((64, 12, 2, 2, 280, 1, 2), 0, 3, (3, D_1024, 896, D_1024, 896)),          # 3 hid = 840
    ((128, 8, 6, 1, 64, 1, 2), 0, 2, (3, D_1024, 896, D_1024, 896)),           # H N = 896
    ((128, 20, 4, 1, 200, 1, 2), 0, 1, (0, 0, 0, 0, 0)),                       # one layer is the single-layer form
    ((192, 13, 2, 1, 77, 1, 2), 0, 2, (0, 0, 0, 0, 0)),                        # hid % 4 refuses the deep forward too
    ((1024, 8, 1, 1, 64, 1, 2), 0, 2, (0, 0, 0, 0, 0)),
]


def test_deep_entries_agree_with_the_plan():
    """ntk_ntm_seq_fwd_deep / ntk_ntm_seq_bwd_deep for L in 2, 3, 4, 10 against ntk_ntm_seq_deep_plan (one answer for both
    directions); ntk_ntm_seq_deep_supported is the plan at write_first = 0; whatever the deep plan takes, the single-layer forward
    validation takes at the same dims; both instantiations of both kernels are reached."""
    L = _lib()
    fwd, bwd, rel = _Sweep("ntk_ntm_seq_fwd_deep"), _Sweep("ntk_ntm_seq_bwd_deep"), _Sweep("deep plan relations")
    seen_f, seen_b, accepted = set(), set(), 0
    for shape in _grid():
        N, Md, R, Wh, hid, sr, O, wf = shape
        if sr == 4 and (Md in (13, 100) or hid in (256, 340)):           # thin the second shift_range: four layer counts per shape
            continue
        single = _plan(L, shape)[0]
        for layers in (2, 3, 4, 10):
            mask, fk, ft, bk, bt = _deep_plan(L, shape, layers)
            fwd.check(mask == 3, _fwd_deep(L, shape, layers), shape, L=layers)
            bwd.check(mask == 3, _bwd_deep(L, shape, layers), shape, L=layers)
            rel.note(mask in (0, 3), "mask %d" % mask, shape, L=layers)
            rel.note(not mask or bool(single & FWD), "the deep plan takes a shape the single-layer forward refuses", shape, L=layers)
            if not wf:
                rel.note(bool(L.ntk_ntm_seq_deep_supported(BATCH, N, Md, R, Wh, hid, sr, O, layers)) == (mask == 3),
                         "ntk_ntm_seq_deep_supported disagrees with the plan", shape, L=layers)
            if mask:
                rel.note((fk == D_1024) == (ft > 768) and (bk == D_1024) == (bt > 768) and 0 < ft <= 1024 and 0 < bt <= 1024 and
                         ft % 64 == 0 and bt % 64 == 0, "threads %d / %d, ids %d / %d" % (ft, bt, fk, bk), shape, L=layers)
                seen_f.add(fk)
                seen_b.add(bk)
                accepted += 1
    print("deep plan accepts %d (shape, L) pairs" % accepted)
    fwd.verdict()
    bwd.verdict()
    rel.verdict()
    assert seen_f == {D_768, D_1024} and seen_b == {D_768, D_1024}, (seen_f, seen_b)
    bad = ["%s write_first=%d L=%d: plan %s, by hand %s" % (s, wf, layers, _deep_plan(L, s + (wf,), layers), want)
           for s, wf, layers, want in DEEP_ANCHORS if _deep_plan(L, s + (wf,), layers) != want]
    assert not bad, "\n  ".join(bad)


def test_write_first_counts_in_the_deep_plan():
    """A write_first cell keeps one more copy of the memory in the BPTT's LDS.  ntk_ntm_seq_deep_supported has no such argument and
    answers for write_first = 0; the plan takes the flag, and the entries follow the plan.  At mem 256 x 20, 3 read + 1 write head,
    hid 200, L = 2 the difference decides: the BPTT needs 171152 B with write_first, 160 KiB = 163840 B is the bound."""
    L = _lib()
    dims = (256, 20, 3, 1, 200, 1, 2)
    assert L.ntk_ntm_seq_deep_supported(BATCH, *dims, 2) == 1
    assert _deep_plan(L, dims + (0,), 2)[0] == 3 and _deep_plan(L, dims + (1,), 2)[0] == 0
    assert b"LDS" in L.ntk_last_error()
    assert _fwd_deep(L, dims + (0,), 2) == NTK_ERR_HIP and _bwd_deep(L, dims + (0,), 2) == NTK_ERR_HIP
    assert _fwd_deep(L, dims + (1,), 2) == NTK_ERR_UNSUPPORTED and _bwd_deep(L, dims + (1,), 2) == NTK_ERR_UNSUPPORTED
