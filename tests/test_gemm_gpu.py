"""GPU: the plain fp32 MFMA GEMMs of csrc/gemm_f32.hip (ntk_gemm_nt_f32, ntk_gemm_tn_f32) against numpy float64 matmul.

Exact cases: A, B, bias and the initial C hold integers of [-4, 4] stored as fp32, so every partial sum is an integer
below 16 K + 4 < 2^24 and fp32 arithmetic in ANY summation order is exact: the result must EQUAL the float64 reference.
A dropped, duplicated or misplaced element cannot hide behind a tolerance.  Every operand is a view into a larger
NaN-filled buffer (leading dimension above the extent, guard rows around it): the logical C must be exact, every guard
element must still hold the NaN it was filled with, bit for bit (the operands' guards carry another NaN payload than the
outputs', so a NaN computed from an operand's guard and stored over an output's guard shows).

Real-valued cases: |got - ref64| <= (K + splits + 2) 2^-23 (|A| |B|)_mn per element, the standard forward bound of a
length-K fp32 dot product in any order (unit round-off 2^-24), one factor of two left for the matrix pipe's internal
accumulation order; `splits` further additions in the slab reduction (for gemm_nt: 1, the bias add)."""
import numpy as np
import pytest
import torch

from small_kernel_util import INPUT_NAN, Guarded, nan_tensor, still_guard, to_dev, vptr

pytestmark = pytest.mark.gpu

NT_M = (1, 31, 127, 128, 129, 300)
NT_N = (1, 31, 63, 64, 65, 127, 128, 129, 200)        # 64 / 65: the BN = 64 and BN = 128 instantiations
NT_K = (4, 28, 32, 36, 64, 516)
TN_MN = (4, 124, 128, 132, 260)
TN_K = (1, 7, 31, 32, 33, 65, 300)
GUARD_WORDS = 64


def ints(rng, shape):
    return rng.integers(-4, 5, size=shape).astype(np.float32)


def assert_exact_range(K):
    assert 16 * K + 4 < 2 ** 24


def run_nt(cuda, a, b, bias):
    """ntk_gemm_nt_f32 on padded, NaN-guarded operands.  Returns the logical C; asserts the guards."""
    from ntmtrack import _lib
    (M, K), N = a.shape, b.shape[0]
    A = Guarded(M, K, K + 4, cuda, before=1, after=1, init=a, payload=INPUT_NAN)
    B = Guarded(N, K, K + 8, cuda, before=1, after=1, init=b, payload=INPUT_NAN)
    C = Guarded(M, N, N + 3, cuda, before=1, after=1)
    bv = None
    if bias is not None:
        bv = nan_tensor(N + GUARD_WORDS, cuda, INPUT_NAN)
        bv[:N] = to_dev(bias, cuda)
    _lib.check(_lib.lib().ntk_gemm_nt_f32(A.ptr, A.ld, B.ptr, B.ld, vptr(bv), C.ptr, C.ld, M, N, K, _lib.stream()),
               "ntk_gemm_nt_f32")
    got = C.logical()
    assert C.guards_intact(), "gemm_nt wrote outside C at M=%d N=%d K=%d" % (M, N, K)
    return got


def run_tn(cuda, a, b, splits, accumulate, c0=None):
    """ntk_gemm_tn_f32 (a [K, M], b [K, N] k-major) on padded, NaN-guarded operands with a NaN-prefilled workspace of
    exactly ntk_gemm_tn_workspace_bytes followed by guard words.  Returns the logical C; asserts the guards."""
    from ntmtrack import _lib
    L = _lib.lib()
    (K, M), N = a.shape, b.shape[1]
    A = Guarded(K, M, M + 4, cuda, before=1, after=2, init=a, payload=INPUT_NAN)
    B = Guarded(K, N, N + 8, cuda, before=1, after=2, init=b, payload=INPUT_NAN)
    C = Guarded(M, N, N + 3, cuda, before=1, after=1, init=c0)
    need = L.ntk_gemm_tn_workspace_bytes(M, N, splits)
    assert need == 4 * M * N * splits
    ws = nan_tensor(need // 4 + GUARD_WORDS, cuda)
    _lib.check(L.ntk_gemm_tn_f32(A.ptr, A.ld, B.ptr, B.ld, C.ptr, C.ld, M, N, K, splits, 1 if accumulate else 0, vptr(ws),
                                 _lib.stream()), "ntk_gemm_tn_f32")
    got = C.logical()
    assert C.guards_intact(), "gemm_tn wrote outside C at M=%d N=%d K=%d splits=%d" % (M, N, K, splits)
    assert still_guard(ws[need // 4:]), "gemm_tn wrote behind its workspace at M=%d N=%d K=%d splits=%d" % (M, N, K, splits)
    return got


# ---------------------------------------------------------------------------------------------------------
# C = A B^T + bias
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("with_bias", [False, True], ids=["nobias", "bias"])
@pytest.mark.parametrize("N", NT_N)
def test_gemm_nt_exact_on_integers(cuda, N, with_bias):
    rng = np.random.default_rng(1000 + N)
    for K in NT_K:
        assert_exact_range(K)
        b = ints(rng, (N, K))
        bias = ints(rng, (N,)) if with_bias else None
        a_all = ints(rng, (max(NT_M), K))
        for M in NT_M:
            a = a_all[:M]
            ref = a.astype(np.float64) @ b.astype(np.float64).T
            if with_bias:
                ref = ref + bias.astype(np.float64)
            got = run_nt(cuda, a, b, bias)
            assert np.array_equal(got.astype(np.float64), ref), "M=%d N=%d K=%d: %d elements differ" % (
                M, N, K, int((got != ref).sum()))


def test_gemm_nt_exact_at_the_products_proportions(cuda):
    """The hoisted input projection cut down: B S = 65 * 2 * 2 rows, 4 hid = 800 columns, ldx = 516."""
    M, N, K = 65 * 2 * 2, 800, 516
    assert_exact_range(K)
    rng = np.random.default_rng(7)
    a, b, bias = ints(rng, (M, K)), ints(rng, (N, K)), ints(rng, (N,))
    ref = a.astype(np.float64) @ b.astype(np.float64).T + bias.astype(np.float64)
    assert np.array_equal(run_nt(cuda, a, b, bias).astype(np.float64), ref)


def test_gemm_nt_wrapper_on_contiguous_tensors(cuda):
    """ntm.gemm_nt (contiguous operands, lda = ldb = K, ldc = N), with and without an `out`."""
    from ntmtrack import ntm as G
    rng = np.random.default_rng(8)
    for (M, N, K) in ((129, 65, 36), (31, 64, 516)):
        assert_exact_range(K)
        a, b, bias = ints(rng, (M, K)), ints(rng, (N, K)), ints(rng, (N,))
        ref = a.astype(np.float64) @ b.astype(np.float64).T
        got = G.gemm_nt(to_dev(a, cuda), to_dev(b, cuda))
        assert np.array_equal(got.cpu().numpy().astype(np.float64), ref)
        out = nan_tensor((M, N), cuda)
        assert G.gemm_nt(to_dev(a, cuda), to_dev(b, cuda), bias=to_dev(bias, cuda), out=out) is out
        assert np.array_equal(out.cpu().numpy().astype(np.float64), ref + bias.astype(np.float64))


@pytest.mark.parametrize("N", [64, 200], ids=["BN64", "BN128"])
def test_gemm_nt_real_valued_within_the_forward_bound(cuda, N):
    M, K = 300, max(NT_K)
    rng = np.random.default_rng(20 + N)
    a, b = rng.standard_normal((M, K)).astype(np.float32), rng.standard_normal((N, K)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    a64, b64, bias64 = a.astype(np.float64), b.astype(np.float64), bias.astype(np.float64)
    ref = a64 @ b64.T + bias64
    bound = (K + 1 + 2) * 2.0 ** -23 * (np.abs(a64) @ np.abs(b64).T + np.abs(bias64))
    got = run_nt(cuda, a, b, bias).astype(np.float64)
    ratio = float(np.max(np.abs(got - ref) / bound))
    print("gemm_nt BN=%d M=%d N=%d K=%d: worst |err| / bound = %.4f" % (64 if N <= 64 else 128, M, N, K, ratio))
    assert ratio <= 1.0


# ---------------------------------------------------------------------------------------------------------
# C (+)= A^T B, split-K
# ---------------------------------------------------------------------------------------------------------
def tn_splits(K):
    return (1, 2, 3, 7, (K + 31) // 32 + 5)          # the last: several splits are empty and must contribute exact zeros


@pytest.mark.parametrize("M", TN_MN)
def test_gemm_tn_exact_on_integers(cuda, M):
    rng = np.random.default_rng(2000 + M)
    for K in TN_K:
        assert_exact_range(K)
        a = ints(rng, (K, M))
        b_all = ints(rng, (K, max(TN_MN)))
        for N in TN_MN:
            b = np.ascontiguousarray(b_all[:, :N])
            c0 = ints(rng, (M, N))
            prod = a.astype(np.float64).T @ b.astype(np.float64)
            for splits in tn_splits(K):
                for accumulate in (0, 1):
                    ref = prod + c0.astype(np.float64) if accumulate else prod
                    got = run_tn(cuda, a, b, splits, accumulate, c0)       # without accumulate c0 must be overwritten
                    assert np.isfinite(got).all(), "M=%d N=%d K=%d splits=%d acc=%d: not finite" % (M, N, K, splits, accumulate)
                    assert np.array_equal(got.astype(np.float64), ref), "M=%d N=%d K=%d splits=%d acc=%d: %d elements differ" % (
                        M, N, K, splits, accumulate, int((got != ref).sum()))


@pytest.mark.parametrize("M", TN_MN)
def test_gemm_tn_wrapper_heuristic_splits(cuda, M):
    """ntm.gemm_tn with splits=None on contiguous operands (the only form the wrapper takes), with a NaN workspace of its own."""
    from ntmtrack import ntm as G
    rng = np.random.default_rng(3000 + M)
    for K in TN_K:
        assert_exact_range(K)
        for N in TN_MN:
            a, b, c0 = ints(rng, (K, M)), ints(rng, (K, N)), ints(rng, (M, N))
            prod = a.astype(np.float64).T @ b.astype(np.float64)
            ta, tb = to_dev(a, cuda), to_dev(b, cuda)
            for accumulate in (False, True):
                out = to_dev(c0, cuda)
                ws = nan_tensor(M * N * 2, cuda)                 # the heuristic gives at most ceil(K / 256) = 2 here
                G.gemm_tn(ta, tb, out, accumulate=accumulate, workspace=ws)
                ref = prod + c0.astype(np.float64) if accumulate else prod
                assert np.array_equal(out.cpu().numpy().astype(np.float64), ref), (M, N, K, accumulate)


def test_gemm_tn_is_bit_identical_between_runs(cuda):
    """The fixed-order split-K promise: the same inputs give the same bits (real-valued, so that an order change would show)."""
    M, N, K, splits = 132, 260, 300, 7
    rng = np.random.default_rng(5)
    a, b = rng.standard_normal((K, M)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    first = run_tn(cuda, a, b, splits, 0)
    second = run_tn(cuda, a, b, splits, 0)
    assert np.array_equal(first.view(np.uint32), second.view(np.uint32))


def test_gemm_tn_cached_workspace_larger_than_needed_and_stale(cuda):
    """A large product, then a small one, both without a workspace argument: the cached slab of ntm._WS is larger than the small
    call needs and holds the large call's partial sums (and, the second time, NaN)."""
    from ntmtrack import ntm as G
    rng = np.random.default_rng(6)
    K = 300
    assert_exact_range(K)
    a, b = ints(rng, (K, 260)), ints(rng, (K, 260))
    out = nan_tensor((260, 260), cuda)
    G.gemm_tn(to_dev(a, cuda), to_dev(b, cuda), out, splits=7)
    assert np.array_equal(out.cpu().numpy().astype(np.float64), a.astype(np.float64).T @ b.astype(np.float64))
    slab = G._WS[cuda]
    assert slab.numel() >= 260 * 260 * 7
    for poison in (False, True):
        if poison:
            slab.fill_(float("nan"))
        for (M, N, Ks, splits) in ((4, 4, 33, 3), (124, 132, 65, None), (4, 128, 7, 6)):
            a2, b2 = ints(rng, (Ks, M)), ints(rng, (Ks, N))
            out2 = nan_tensor((M, N), cuda)
            G.gemm_tn(to_dev(a2, cuda), to_dev(b2, cuda), out2, splits=splits)
            assert G._WS[cuda] is slab
            assert np.array_equal(out2.cpu().numpy().astype(np.float64), a2.astype(np.float64).T @ b2.astype(np.float64)), (M, N, Ks, splits)


def test_gemm_tn_real_valued_within_the_forward_bound(cuda):
    M, N, K = 260, 260, max(TN_K)
    rng = np.random.default_rng(30)
    a, b = rng.standard_normal((K, M)).astype(np.float32), rng.standard_normal((K, N)).astype(np.float32)
    c0 = rng.standard_normal((M, N)).astype(np.float32)
    a64, b64 = a.astype(np.float64), b.astype(np.float64)
    for splits, accumulate in ((1, 0), (3, 0), (7, 1)):
        ref = a64.T @ b64 + (c0.astype(np.float64) if accumulate else 0.0)
        mag = np.abs(a64).T @ np.abs(b64) + (np.abs(c0.astype(np.float64)) if accumulate else 0.0)
        bound = (K + splits + 2) * 2.0 ** -23 * mag
        got = run_tn(cuda, a, b, splits, accumulate, c0).astype(np.float64)
        ratio = float(np.max(np.abs(got - ref) / bound))
        print("gemm_tn M=%d N=%d K=%d splits=%d accumulate=%d: worst |err| / bound = %.4f" % (M, N, K, splits, accumulate, ratio))
        assert ratio <= 1.0
