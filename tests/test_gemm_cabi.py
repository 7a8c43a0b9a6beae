"""CPU: host-side validation of the plain GEMM entries (csrc/gemm_f32.hip) and of the small kernels that had no refusal
test yet.  Every pointer is non-null, 16-byte aligned and never dereferenced: the shape check fires before any launch.
The refusal tests run only where no device is visible (as the other fake-pointer files do): should a check ever go missing,
the call fails at the launch there instead of handing a made-up address to a kernel."""
import ctypes

import pytest
import torch

no_device = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: runs only where no device is visible")

BAD_SHAPE, BAD_PTR = -1, -2
ONE = ctypes.c_void_p(16)          # non-null, aligned
ODD = ctypes.c_void_p(20)          # non-null, 4-byte aligned only


@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


def gemm_nt(L, M=8, N=8, K=8, lda=None, ldb=None, ldc=None, A=ONE, B=ONE, C=ONE, bias=None):
    return L.ntk_gemm_nt_f32(A, K if lda is None else lda, B, K if ldb is None else ldb, bias, C, N if ldc is None else ldc,
                             M, N, K, None)


def gemm_tn(L, M=8, N=8, K=8, lda=None, ldb=None, ldc=None, splits=1, accumulate=0, A=ONE, B=ONE, C=ONE, ws=ONE):
    return L.ntk_gemm_tn_f32(A, M if lda is None else lda, B, N if ldb is None else ldb, C, N if ldc is None else ldc,
                             M, N, K, splits, accumulate, ws, None)


NT_BAD_SHAPES = {
    "K%4": dict(K=6, lda=8, ldb=8),
    "lda%4": dict(lda=10),
    "ldb%4": dict(ldb=10),
    "lda<K": dict(lda=4),
    "ldb<K": dict(ldb=4),
    "ldc<N": dict(ldc=7),
    "M=0": dict(M=0),
    "N=0": dict(N=0),
    "K=0": dict(K=0),
    "M<0": dict(M=-1),
    "N<0": dict(N=-4),
    "K<0": dict(K=-4),
}


@no_device
@pytest.mark.parametrize("case", sorted(NT_BAD_SHAPES))
def test_gemm_nt_refuses_bad_shapes(L, case):
    assert gemm_nt(L, **NT_BAD_SHAPES[case]) == BAD_SHAPE
    assert b"ntk_gemm_nt_f32" in L.ntk_last_error()


@no_device
@pytest.mark.parametrize("case", ["A_null", "B_null", "C_null", "A_unaligned", "B_unaligned"])
def test_gemm_nt_refuses_bad_pointers(L, case):
    kw = {"A_null": dict(A=None), "B_null": dict(B=None), "C_null": dict(C=None), "A_unaligned": dict(A=ODD),
          "B_unaligned": dict(B=ODD)}[case]
    assert gemm_nt(L, **kw) == BAD_PTR
    assert b"ntk_gemm_nt_f32" in L.ntk_last_error()


TN_BAD_SHAPES = {
    "M%4": dict(M=6, lda=8),
    "N%4": dict(N=6, ldb=8, ldc=8),
    "lda%4": dict(lda=10),
    "ldb%4": dict(ldb=10),
    "lda<M": dict(lda=4),
    "ldb<N": dict(ldb=4),
    "ldc<N": dict(ldc=7),
    "splits=0": dict(splits=0),
    "splits=65536": dict(splits=65536),
    "M=0": dict(M=0),
    "N=0": dict(N=0),
    "K=0": dict(K=0),
    "K<0": dict(K=-1),
}


@no_device
@pytest.mark.parametrize("case", sorted(TN_BAD_SHAPES))
def test_gemm_tn_refuses_bad_shapes(L, case):
    assert gemm_tn(L, **TN_BAD_SHAPES[case]) == BAD_SHAPE
    assert b"ntk_gemm_tn_f32" in L.ntk_last_error()


@no_device
@pytest.mark.parametrize("case", ["A_null", "B_null", "C_null", "ws_null", "A_unaligned", "B_unaligned"])
def test_gemm_tn_refuses_bad_pointers(L, case):
    kw = {"A_null": dict(A=None), "B_null": dict(B=None), "C_null": dict(C=None), "ws_null": dict(ws=None),
          "A_unaligned": dict(A=ODD), "B_unaligned": dict(B=ODD)}[case]
    assert gemm_tn(L, **kw) == BAD_PTR
    assert b"ntk_gemm_tn_f32" in L.ntk_last_error()


def test_workspace_sizes(L):
    for M, N, s in ((4, 4, 1), (128, 132, 7), (260, 260, 15), (800, 516, 1024)):
        assert L.ntk_gemm_tn_workspace_bytes(M, N, s) == 4 * M * N * s
    for M, N, s in ((0, 4, 1), (4, 0, 1), (4, 4, 0), (-4, 4, 1), (4, -4, 1), (4, 4, -1)):
        assert L.ntk_gemm_tn_workspace_bytes(M, N, s) == 0
    for n in (1, 4096, 4097):
        assert L.ntk_global_norm_workspace_bytes(n) == 4 * ((n + 4095) // 4096)


@no_device
def test_small_kernels_refuse_bad_arguments(L):
    f = ctypes.c_float
    assert L.ntk_log_loss(ONE, ONE, ONE, ONE, 0, None) == BAD_SHAPE
    assert b"ntk_log_loss" in L.ntk_last_error()
    assert L.ntk_heatmap_ce_loss(ONE, ONE, ONE, ONE, ONE, 2, 1, 9, None) == BAD_SHAPE            # T = 1: no scored frame
    assert b"ntk_heatmap_ce_loss" in L.ntk_last_error()
    assert L.ntk_two_step_ce_loss(ONE, ONE, ONE, ONE, ONE, 2, 0, 9, None) == BAD_SHAPE
    assert b"ntk_two_step_ce_loss" in L.ntk_last_error()
    assert L.ntk_maxpool2x2(ONE, ONE, 1, 3, 4, 4, None) == BAD_SHAPE                              # odd H
    assert b"ntk_maxpool2x2" in L.ntk_last_error()
    assert L.ntk_maxpool2x2(ONE, ONE, 1, 4, 4, 6, None) == BAD_SHAPE                              # C % 4
    assert L.ntk_transpose_pad(ONE, 8, ONE, 3, 4, 8, None) == BAD_SHAPE                           # ldo < rows
    assert b"ntk_transpose_pad" in L.ntk_last_error()
    assert L.ntk_ntm_init_state(ONE, ONE, 8, 2, 2, None) == BAD_SHAPE                             # act is 0 or 1
    assert b"ntk_ntm_init_state" in L.ntk_last_error()
    assert L.ntk_rmsprop_clip_step(ONE, ONE, ONE, ONE, 8, f(1e-4), f(.95), f(.9), f(1e-10), f(10.0), None, None) == BAD_PTR
    assert b"ntk_rmsprop_clip_step" in L.ntk_last_error()
    assert L.ntk_rmsprop_clip_step_checked(ONE, ONE, ONE, ONE, 8, f(1e-4), f(.95), f(.9), f(1e-10), f(0.0), None, ONE, ONE,
                                           None) == BAD_PTR
    assert b"ntk_rmsprop_clip_step_checked" in L.ntk_last_error()
