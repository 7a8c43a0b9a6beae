"""CPU: host-side validation of the stand-alone DNC module entries (csrc/dnc_modules.hip), the stand-alone NTM ops
(csrc/ntm_ops.hip) and the image entries (csrc/image_crop.hip).  Conventions of tests/test_gemm_cabi.py: every pointer is
non-null, 16-byte aligned and never dereferenced (the check fires before any launch), and the tests run only where no device is
visible -- should a check ever go missing, the call fails at the launch there instead of handing a made-up address to a kernel.
Each refusal returns the code the header documents and leaves the entry's name in ntk_last_error()."""
import ctypes

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: runs only where no device is visible")

BAD_SHAPE, BAD_PTR, UNSUPPORTED = -1, -2, -3
ONE = ctypes.c_void_p(16)          # non-null, aligned
TWO = ctypes.c_void_p(32)          # a second address, for the entries that refuse aliased buffers


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


class Entry(object):
    """One C entry: `order` names its arguments in call order, `ptrs` the pointer arguments that must not be null, `good` a set of
    integer arguments every check accepts.  call(**changes) runs it with fake pointers and `good` overridden by `changes`."""

    def __init__(self, name, order, ptrs, good):
        self.name, self.order, self.ptrs, self.good = name, order.split(), ptrs.split(), good

    def call(self, L, **changes):
        vals = {p: ONE for p in self.order if p not in self.good}
        vals.update(self.good)
        vals.update(changes)
        return getattr(L, self.name)(*([vals[a] for a in self.order] + [None]))

    def refused(self, L, code, **changes):
        rc = self.call(L, **changes)
        err = L.ntk_last_error()
        assert rc == code, (self.name, changes, rc, err)
        assert self.name.encode() in err, (self.name, changes, err)


f32 = ctypes.c_float
ENTRIES = {e.name: e for e in (
    Entry("ntk_dnc_cosine_weights", "memory keys strengths out B N W H", "memory keys strengths out", dict(B=2, N=8, W=4, H=2)),
    Entry("ntk_dnc_linkage", "prev_link prev_prec ww link prec B N Wn", "prev_link prev_prec ww link prec", dict(B=2, N=8, Wn=2)),
    Entry("ntk_dnc_directional_read_weights", "link prw out B N Wn R forward", "link prw out", dict(B=2, N=8, Wn=2, R=3, forward=1)),
    Entry("ntk_dnc_freeness", "ww free_gate rw prev_usage usage B N Wn R", "ww free_gate rw prev_usage usage", dict(B=2, N=8, Wn=2, R=3)),
    Entry("ntk_dnc_write_allocation_weights", "usage write_gates out B N Wn", "usage out", dict(B=2, N=8, Wn=2)),
    Entry("ntk_dnc_interface_activations", "raw ldr act B N W R Wn", "raw act", dict(ldr=64, B=2, N=8, W=4, R=2, Wn=1)),   # I = 33
    Entry("ntk_dnc_erase_and_write", "memory address reset values out B N W Wn", "memory address reset values out",
          dict(B=2, N=8, W=4, Wn=2)),
    Entry("ntk_dnc_read_words", "rw memory out B N W R", "rw memory out", dict(B=2, N=8, W=4, R=3)),
    Entry("ntk_dnc_access_step_bwd", "raw ldr memory rw ww link prec usage d_reads g_memory g_rw g_link g_prec g_usage d_raw workspace "
          "B N W R Wn", "raw memory rw ww link prec usage d_reads g_memory g_rw g_link g_prec g_usage d_raw workspace",
          dict(ldr=64, B=2, N=8, W=4, R=2, Wn=1)),
    Entry("ntk_ntm_cosine_similarity", "memory keys out B N Md H mode", "memory keys out", dict(B=2, N=8, Md=4, H=2, mode=0)),
    Entry("ntk_ntm_circular_convolution", "w kernel out B H N SS", "w kernel out", dict(out=TWO, B=2, H=2, N=8, SS=3)),
    Entry("ntk_resize_bilinear", "image H W C out OH OW", "image out", dict(H=4, W=5, C=3, OH=6, OW=7)),
    Entry("ntk_crop_and_resize", "image H W C mean y1 x1 y2 x2 out ch cw extrapolation", "image out",
          dict(H=4, W=5, C=3, y1=f32(0), x1=f32(0), y2=f32(1), x2=f32(1), ch=6, cw=7, extrapolation=f32(0))),
)}

# every dimension that must be positive, per entry
DIMS = {
    "ntk_dnc_cosine_weights": "B N W H",
    "ntk_dnc_linkage": "B N Wn",
    "ntk_dnc_directional_read_weights": "B N Wn R",
    "ntk_dnc_freeness": "B N Wn R",
    "ntk_dnc_write_allocation_weights": "B N Wn",
    "ntk_dnc_interface_activations": "B N W R Wn",        # N, W, R, Wn went unchecked into dnc_fill_dims before this suite
    "ntk_dnc_erase_and_write": "B N W Wn",
    "ntk_dnc_read_words": "B N W R",
    "ntk_ntm_cosine_similarity": "B N Md H",
    "ntk_ntm_circular_convolution": "B H N SS",
    "ntk_resize_bilinear": "H W C OH OW",
    "ntk_crop_and_resize": "H W C ch cw",
}


@pytest.mark.parametrize("name,dim,value", [(n, d, v) for n in sorted(DIMS) for d in DIMS[n].split() for v in (0, -1)])
def test_non_positive_dimensions_are_refused(L, name, dim, value):
    ENTRIES[name].refused(L, BAD_SHAPE, **{dim: value})


@pytest.mark.parametrize("name,arg", [(n, p) for n in sorted(ENTRIES) for p in ENTRIES[n].ptrs])
def test_null_pointers_are_refused(L, name, arg):
    ENTRIES[name].refused(L, BAD_PTR, **{arg: None})


def test_cosine_weights_lds_limit(L):
    e = ENTRIES["ntk_dnc_cosine_weights"]
    e.refused(L, BAD_SHAPE, H=1, N=16385)                         # H * N * 4 bytes = 64 KiB + 4
    e.refused(L, BAD_SHAPE, H=5, N=3277)                          # 16385 scores again
    assert e.call(L, H=16, N=1024) not in (BAD_SHAPE, BAD_PTR)    # 16384 scores fit: stops at the launch (no device)


def test_allocation_limits(L):
    e = ENTRIES["ntk_dnc_write_allocation_weights"]
    e.refused(L, BAD_SHAPE, N=8193)                               # 2 N floats of LDS > 64 KiB
    e.refused(L, BAD_PTR, Wn=2, write_gates=None)                 # the second head needs the first one's gate
    assert e.call(L, Wn=1, write_gates=None) not in (BAD_SHAPE, BAD_PTR)
    assert e.call(L, N=8192, Wn=1, write_gates=None) not in (BAD_SHAPE, BAD_PTR)


def test_interface_activations_row_stride(L):
    e = ENTRIES["ntk_dnc_interface_activations"]
    e.refused(L, BAD_SHAPE, ldr=32)                               # interface of (W, R, Wn) = (4, 2, 1) is 33 wide
    assert e.call(L, ldr=33) not in (BAD_SHAPE, BAD_PTR)


@pytest.mark.parametrize("change", [dict(R=5), dict(Wn=5), dict(N=6), dict(W=6), dict(N=0), dict(W=0), dict(R=0), dict(Wn=0)],
                         ids=lambda c: "%s=%d" % list(c.items())[0])
def test_access_step_bwd_range(L, change):
    ENTRIES["ntk_dnc_access_step_bwd"].refused(L, UNSUPPORTED, **change)


def test_ntm_cosine_similarity_mode_and_lds(L):
    e = ENTRIES["ntk_ntm_cosine_similarity"]
    e.refused(L, BAD_SHAPE, mode=2)
    e.refused(L, BAD_SHAPE, mode=-1)
    e.refused(L, UNSUPPORTED, mode=0, Md=4097, H=3)               # (Md + H Md) * 4 = 64 KiB + 16
    e.refused(L, UNSUPPORTED, mode=0, Md=1, H=16384)              # 64 KiB + 4
    assert e.call(L, mode=0, Md=4096, H=3) not in (BAD_SHAPE, BAD_PTR, UNSUPPORTED)    # 64 KiB exactly
    assert e.call(L, mode=0, Md=1, H=16383) not in (BAD_SHAPE, BAD_PTR, UNSUPPORTED)
    assert e.call(L, mode=1, Md=4096, H=4) not in (BAD_SHAPE, BAD_PTR, UNSUPPORTED)    # mode 1 keeps H floats only


def test_circular_convolution_shift_space_and_aliasing(L):
    e = ENTRIES["ntk_ntm_circular_convolution"]
    e.refused(L, BAD_SHAPE, N=8, SS=9)
    e.refused(L, BAD_SHAPE, N=1, SS=2)
    e.refused(L, BAD_PTR, w=ONE, out=ONE)                         # the shifted reads would see the new values
    assert e.call(L, N=8, SS=8) not in (BAD_SHAPE, BAD_PTR)


def test_crop_and_resize_element_count_overflow(L):
    e = ENTRIES["ntk_crop_and_resize"]
    e.refused(L, BAD_SHAPE, ch=46341, cw=46341, C=1)              # 46341^2 = 2^31 + 88713: negative in int
    e.refused(L, BAD_SHAPE, ch=65536, cw=65536, C=1)              # 2^32: zero in int
    assert e.call(L, mean=None) not in (BAD_SHAPE, BAD_PTR)       # a null mean is "subtract nothing"
