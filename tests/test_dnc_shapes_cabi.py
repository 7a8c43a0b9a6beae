"""CPU: the shapes ntk_dnc_seq_fwd and ntk_dnc_seq_bwd accept, over a grid with the first values outside every range.

Both entries are called with fake pointers (non-null, 16-byte aligned, never dereferenced): an accepted shape must pass every
host-side check and reach the device calls, which fail without a device (NTK_ERR_HIP); a refused shape must be refused before them
(NTK_ERR_BAD_SHAPE / NTK_ERR_UNSUPPORTED) with a reason in ntk_last_error().  With a device present a wrongly accepted shape would
launch against the fake pointers, so the file runs only where there is none.  What "accepted" means is restated here from the
documented ranges (include/ntmtrack.h) and the kernels' LDS layouts, and pinned by named anchors: every row of the table of
tests/test_dnc_shapes_gpu.py, BASELINE configs 3 and 5, and the largest memory each direction takes at word 16, 4 read heads,
hidden 64.  The cluster planners ask the device for its compute units and stay with the GPU file."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: runs only where no device is visible")

NTK_ERR_BAD_SHAPE, NTK_ERR_UNSUPPORTED, NTK_ERR_HIP = -1, -3, -4
P = ctypes.c_void_p(1 << 20)
BATCH, STEPS = 2, 3
DT, LDS_LIMIT = 1024, 160 * 1024

MEM_SIZE = (0, 4, 6, 16, 260, 340, 1024, 1028)
WORD = (0, 4, 6, 8, 132, 256, 260)
READS = (0, 1, 4, 5)
WRITES = (0, 1, 4, 5, 8, 9)
HIDDEN = (0, 1, 4, 513, 768, 1020, 1024, 1028)
OUTPUTS = (0, 1, 16, 17)


def _lib():
    from ntmtrack import _lib
    return _lib.lib()


def _a4(v):
    return (v + 3) // 4 * 4


def _fwd(L, shape, B=BATCH, S=STEPS):
    return L.ntk_dnc_seq_fwd(B, S, *shape, 20.0, *([P] * 13), *([P] * 18), None)


def _bwd(L, shape, B=BATCH, S=STEPS, ldkT=None, ldhT=None):
    N, W, R, Wn, hid, O = shape
    return L.ntk_dnc_seq_bwd(B, S, *shape, 20.0, P, _a4(R * W + hid) if ldkT is None else ldkT, P, _a4(hid) if ldhT is None else ldhT, P,
                             *([P] * 7), *([P] * 15), *([P] * 6), None, 0, None)


# ---- the launchers' arithmetic, restated: LDS floats of the two kernels (every array rounded up to 4 floats)
def _take(sizes):
    return sum(_a4(n) for n in sizes)


def _ip(W, R, Wn):
    return _a4(3 * Wn * W + R + 2 * Wn + R * (1 + 2 * Wn) + Wn + R * W + R)


def _fwd_lds_bytes(N, W, R, Wn, hid, O):
    IP, RW = _ip(W, R, Wn), R * W
    part = max(max(1, DT // hid) * 4 * hid, max(1, DT // (IP // 4)) * IP, max(1, DT // N) * N, 16 * R * 256,
               min(max(1, DT // (RW // 4)), N) * RW)
    return 4 * _take([part, RW + hid, hid, IP, N, R * N, Wn * N, Wn * N, Wn * N, R * N, N, R * Wn * N, R * Wn * N, 64])


def _bwd_lds_bytes(N, W, R, Wn, hid, O):
    IP, RW, RN, HN, HW = _ip(W, R, Wn), R * W, R * N, Wn * N, Wn * W
    ldkT, ldhT = _a4(RW + hid), _a4(hid)
    part = max(2 * max(1, DT // N) * N, max(1, DT // (ldkT // 4)) * ldkT, max(1, DT // (ldhT // 4)) * ldhT)
    sim = [HN, N] if Wn > 1 else []                        # simulated usages and their gradient: several write heads only
    return 4 * _take([part, IP, IP] + [HN, HN, N, N, HN, HN, HN] + sim[:1] + [N, N, HN, HN, HN, HN, HN, HN, N, N] + sim[1:] +
                     [RN, RN, RN, RN, Wn * RN, Wn * RN, RN, RN, RN, ldkT, RW, RW, HW, HW, HW, hid, hid, 4 * hid, 64])


def fwd_ok(N, W, R, Wn, hid, O):
    return (4 <= N <= 1024 and N % 4 == 0 and 4 <= W <= 256 and W % 4 == 0 and 1 <= R <= 4 and 1 <= Wn <= 8 and 1 <= hid <= 1024 and
            R * W <= 1024 and 1 <= O <= 16 and _fwd_lds_bytes(N, W, R, Wn, hid, O) <= LDS_LIMIT)


def bwd_ok(N, W, R, Wn, hid, O):
    return (4 <= N <= 1024 and N % 4 == 0 and 4 <= W <= 256 and W % 4 == 0 and 1 <= R <= 4 and 1 <= Wn <= 4 and 4 <= hid <= 1024 and
            hid % 4 == 0 and R * W + hid <= 1024 and 1 <= O <= 16 and _bwd_lds_bytes(N, W, R, Wn, hid, O) <= LDS_LIMIT)


class _Sweep(object):
    """Collects every disagreement between the restated ranges and an entry; the failure lists them all."""

    def __init__(self, entry):
        self.entry, self.n, self.accepted, self.bad = entry, 0, 0, []

    def check(self, accepted, rc, shape, **more):
        self.n += 1
        self.accepted += bool(accepted)
        msg = _lib().ntk_last_error() or b""
        what = "N=%d W=%d R=%d Wn=%d hid=%d O=%d" % shape + "".join(" %s=%d" % kv for kv in more.items())
        if accepted and rc != NTK_ERR_HIP:
            self.bad.append("%s: in range, the entry returned %d (%s)" % (what, rc, msg.decode()))
        elif not accepted and rc not in (NTK_ERR_BAD_SHAPE, NTK_ERR_UNSUPPORTED):
            self.bad.append("%s: out of range, the entry returned %d" % (what, rc))
        elif not accepted and not msg:
            self.bad.append("%s: refused with %d and no reason in ntk_last_error()" % (what, rc))

    def verdict(self):
        assert self.n > 0 and 0 < self.accepted < self.n
        print("%s: %d calls checked, %d accepted" % (self.entry, self.n, self.accepted))
        assert not self.bad, "%s: %d of %d checks disagree:\n  %s" % (self.entry, len(self.bad), self.n, "\n  ".join(self.bad[:40]))


def test_entries_agree_with_the_documented_ranges():
    """The full product of the six axes; the BPTT's shapes are a subset of the forward's."""
    L = _lib()
    fwd, bwd = _Sweep("ntk_dnc_seq_fwd"), _Sweep("ntk_dnc_seq_bwd")
    for shape in itertools.product(MEM_SIZE, WORD, READS, WRITES, HIDDEN, OUTPUTS):
        f, b = fwd_ok(*shape), bwd_ok(*shape)
        assert f or not b, shape
        fwd.check(f, _fwd(L, shape), shape)
        bwd.check(b, _bwd(L, shape), shape)
    fwd.verdict()
    bwd.verdict()


def test_batch_steps_and_leading_dimensions():
    L = _lib()
    shape = (256, 64, 4, 1, 200, 2)
    sweep = _Sweep("B = 0 / S = 0 / ldkT / ldhT")
    for kw in (dict(B=0), dict(S=0)):
        sweep.check(False, _fwd(L, shape, **kw), shape, **kw)
        sweep.check(False, _bwd(L, shape, **kw), shape, **kw)
    for ldkT, ldhT, ok in ((456, 200, True), (460, 204, True), (452, 200, False), (458, 200, False), (456, 196, False), (456, 202, False)):
        sweep.check(ok, _bwd(L, shape, ldkT=ldkT, ldhT=ldhT), shape, ldkT=ldkT, ldhT=ldhT)
    sweep.verdict()


# (N, W, R, Wn, hid, O) -> (forward, BPTT), evaluated by hand from the ranges above; a word the refusal must name
ANCHORS = [
    # the table of tests/test_dnc_shapes_gpu.py
    ((4, 4, 1, 1, 4, 1), True, True, None),
    ((16, 256, 4, 1, 16, 2), True, False, b"1040"),                  # K = R W + hid = 1040
    ((16, 128, 4, 1, 512, 2), True, True, None),                     # K = 1024
    ((16, 128, 4, 1, 768, 2), True, False, b"1280"),
    ((16, 8, 2, 1, 1024, 2), True, False, b"1040"),
    ((16, 256, 4, 4, 16, 2), True, False, b"1040"),                  # IP = 4152
    ((16, 256, 1, 5, 16, 2), True, False, b"num_writes=5"),          # IP = 4124
    ((40, 12, 3, 8, 24, 2), True, False, b"num_writes=8"),
    ((260, 8, 2, 2, 20, 3), True, True, None),
    ((340, 12, 3, 1, 340, 2), True, True, None),
    ((1024, 8, 1, 1, 16, 2), True, True, None),
    ((1024, 16, 4, 1, 64, 2), True, False, b"LDS"),                  # forward 153120 B of 163840, BPTT 237568 B
    ((24, 132, 2, 2, 36, 16), True, True, None),
    ((16, 8, 2, 1, 513, 2), True, False, b"multiple of 4"),
    ((64, 16, 1, 1, 4, 2), True, True, None),
    ((192, 20, 3, 1, 36, 2), True, True, None),
    ((64, 256, 4, 1, 32, 2), True, False, b"1056"),
    ((64, 128, 4, 1, 32, 2), True, True, None),
    ((128, 4, 1, 1, 1024, 7), True, False, b"1028"),
    ((512, 16, 2, 1, 40, 2), True, True, None),
    # BASELINE configs 3 and 5
    ((256, 64, 4, 1, 200, 2), True, True, None),
    ((512, 128, 4, 1, 200, 2), True, True, None),
    # word 16, 4 read heads, hidden 64: the forward's LDS still fits at the largest memory_size, the BPTT's up to 676
    ((1024, 16, 4, 1, 64, 2), True, False, b"LDS"),
    ((1028, 16, 4, 1, 64, 2), False, False, b"memory_size=1028"),
    ((676, 16, 4, 1, 64, 2), True, True, None),                      # 163792 B of 163840
    ((680, 16, 4, 1, 64, 2), True, False, b"164640 B of LDS"),
    # the forward's LDS: 8 write heads at the largest memory need 5 x 8 x 1024 + 2 x 4 x 8 x 1024 floats of per-slot state alone
    ((1024, 8, 4, 8, 16, 2), False, False, b"LDS"),
]


def test_named_shapes_pin_the_ranges():
    L = _lib()
    bad = []
    for shape, f, b, word in ANCHORS:
        if (fwd_ok(*shape), bwd_ok(*shape)) != (f, b):
            bad.append("%s: restated ranges say %s, by hand %s" % (shape, (fwd_ok(*shape), bwd_ok(*shape)), (f, b)))
        rf = _fwd(L, shape)
        msg_f = L.ntk_last_error() or b""
        rb = _bwd(L, shape)
        msg_b = L.ntk_last_error() or b""
        if (rf == NTK_ERR_HIP, rb == NTK_ERR_HIP) != (f, b) or not {rf, rb} <= {NTK_ERR_HIP, NTK_ERR_UNSUPPORTED}:
            bad.append("%s: the entries returned %d / %d, by hand %s" % (shape, rf, rb, (f, b)))
        if word is not None and word not in (msg_b if f else msg_f):
            bad.append("%s: the refusal does not name %r: %r" % (shape, word, msg_b if f else msg_f))
    assert not bad, "\n  ".join(bad)
    assert _fwd_lds_bytes(1024, 16, 4, 1, 64, 2) == 153120 and _bwd_lds_bytes(1024, 16, 4, 1, 64, 2) == 237568
    assert _bwd_lds_bytes(676, 16, 4, 1, 64, 2) == 163792 and _bwd_lds_bytes(680, 16, 4, 1, 64, 2) == 164640


# ---- the pointer checks of the two entries (csrc/dnc_common.h: dnc_fwd_check_ptrs / dnc_bwd_check_ptrs).  Every refusal happens on
# the host: nothing is dereferenced, so fake addresses do.
NTK_ERR_BAD_PTR = -2
PTR_SHAPE = (64, 16, 2, 1, 24, 2)
OFF4 = ctypes.c_void_p((1 << 20) + 4)                       # an address = 4 mod 16
FWD_PTRS = ("xproj", "Wr", "Wi", "Wy", "mem", "link", "usage", "rw", "ww", "prec", "reads", "hc", "out")
FWD_RECS = ("rec_z", "rec_gates", "rec_c", "rec_hc", "rec_yin", "rec_ifc", "rec_u", "rec_ww", "rec_rw", "rec_cw", "rec_cr", "rec_al",
            "rec_p", "rec_fwd", "rec_bwd", "rec_M", "rec_L", "rec_ypre")
FWD_ALIGNED = ("xproj", "Wr", "Wi", "mem", "link", "rec_gates", "rec_M", "rec_L")
BWD_PTRS = ("WrT", "WiT", "Wy", "mem0", "link0", "usage0", "rw0", "ww0", "prec0", "hc0", "rec_gates", "rec_c", "rec_ifc", "rec_u",
            "rec_ww", "rec_rw", "rec_cw", "rec_cr", "rec_al", "rec_p", "rec_fwd", "rec_bwd", "rec_M", "rec_L", "rec_ypre", "dout", "gM",
            "gL", "dgates", "dxi", "dypre", "gcarry")
BWD_ALIGNED = ("WrT", "WiT", "rec_gates", "rec_M", "rec_L", "gM", "gL", "dgates", "mem0", "link0")


def _fwd_with(L, **ptrs):
    a = dict.fromkeys(FWD_PTRS + FWD_RECS, P)
    a.update(ptrs)
    return L.ntk_dnc_seq_fwd(BATCH, STEPS, *PTR_SHAPE, 20.0, *[a[n] for n in FWD_PTRS + FWD_RECS], None)


def _bwd_with(L, **ptrs):
    a = dict.fromkeys(BWD_PTRS, P)
    a.update(ptrs)
    N, W, R, Wn, hid, O = PTR_SHAPE
    v = [a[n] for n in BWD_PTRS]
    return L.ntk_dnc_seq_bwd(BATCH, STEPS, *PTR_SHAPE, 20.0, v[0], _a4(R * W + hid), v[1], _a4(hid), *v[2:], 0, None)


def _refused(L, rc, entry, what, bad):
    msg = L.ntk_last_error() or b""
    if rc != NTK_ERR_BAD_PTR or not msg.startswith(entry.encode()):
        bad.append("%s, %s: returned %d, reason %r" % (entry, what, rc, msg))


def test_pointer_checks_of_the_one_workgroup_entries():
    L = _lib()
    assert fwd_ok(*PTR_SHAPE) and bwd_ok(*PTR_SHAPE)
    bad = []
    for n in FWD_PTRS:
        _refused(L, _fwd_with(L, **{n: None}), "ntk_dnc_seq_fwd", n + " null", bad)
    for n in FWD_ALIGNED:
        _refused(L, _fwd_with(L, **{n: OFF4}), "ntk_dnc_seq_fwd", n + " at 4 mod 16", bad)
    none = dict.fromkeys(FWD_RECS, None)
    for n in FWD_RECS:                                       # 1 of 18, and 17 of 18, each record in turn
        _refused(L, _fwd_with(L, **dict(none, **{n: P})), "ntk_dnc_seq_fwd", "only " + n, bad)
        _refused(L, _fwd_with(L, **{n: None}), "ntk_dnc_seq_fwd", "all records but " + n, bad)
    for n in BWD_PTRS[:-1]:
        _refused(L, _bwd_with(L, **{n: None}), "ntk_dnc_seq_bwd", n + " null", bad)
    for n in BWD_ALIGNED:
        _refused(L, _bwd_with(L, **{n: OFF4}), "ntk_dnc_seq_bwd", n + " at 4 mod 16", bad)
    # past every host-side check, to the device call
    for what, rc in (("no records", _fwd_with(L, **none)), ("18 records", _fwd_with(L)), ("BPTT", _bwd_with(L)),
                     ("BPTT without gcarry", _bwd_with(L, gcarry=None))):
        if rc != NTK_ERR_HIP:
            bad.append("%s: returned %d, expected the device call to fail (%d)" % (what, rc, NTK_ERR_HIP))
    assert not bad, "\n  ".join(bad)
