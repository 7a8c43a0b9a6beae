// Plain fp32 MFMA GEMMs around the recurrence, on the tile of mfma_tile.h:
//   * C = A * B^T (+bias)               -- hoisted LSTM input projection
//   * C (+)= A^T * B (k-major, split-K) -- BPTT weight-gradient contractions
// fp32 MFMA runs at 64 cycles per instruction per SIMD, so one K-tile is ~4096 MFMA cycles per wave against 8 x 16-byte loads
// per thread: the loop is matrix-pipe bound by construction.
#include "mfma_tile.h"

namespace {

// ---------------------------------------------------------------------------
// C[M,N] = A[M,K] * B[N,K]^T + bias
// ---------------------------------------------------------------------------
template <int BN>
__global__ __launch_bounds__(256, 2) void gemm_nt_kernel(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
    const float* __restrict__ bias, float* __restrict__ C, int ldc, int M, int N, int K) {
    constexpr int TN = BN / 64;
    __shared__ __attribute__((aligned(16))) float lds[2 * (BM + BN) * LDT];
    const int tid = threadIdx.x;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BN;
    const int lrow = tid >> 3, kg = tid & 7;
    auto la = [&](int s, int kt) -> f32x4 {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int m = m0 + lrow + 32 * s, k = kt * BK + kg * 4;
        if (m < M && k < K) v = *reinterpret_cast<const f32x4*>(A + (size_t)m * lda + k);
        return v;
    };
    auto lb = [&](int s, int kt) -> f32x4 {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int n = n0 + lrow + 32 * s, k = kt * BK + kg * 4;
        if (n < N && k < K) v = *reinterpret_cast<const f32x4*>(B + (size_t)n * ldb + k);
        return v;
    };
    f32x16 acc[2][TN];
    acc_clear(acc);
    gemm_pipeline<BN>(la, lb, (K + BK - 1) / BK, lds, acc);

    const int lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int kh = lane >> 5, col = lane & 31;
#pragma unroll
    for (int tn = 0; tn < TN; ++tn) {
        const int n = n0 + wn * (BN / 2) + tn * 32 + col;
        if (n >= N) continue;
        const float bv = bias ? bias[n] : 0.f;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = frag_row(m0 + wm * 64 + tm * 32, kh, r);
                if (m < M) C[(size_t)m * ldc + n] = acc[tm][tn][r] + bv;
            }
    }
}

// ---------------------------------------------------------------------------
// slab[z][M,N] = sum_{k in split z} A[k,M]^T B[k,N]   (operands k-major)
// LDS images [BK][128+4]: row index contiguous, fragments by ds_read_b32
// (32 consecutive lanes -> 32 consecutive banks).
// ---------------------------------------------------------------------------
constexpr int LDM = BM + 4;

__global__ __launch_bounds__(256, 2) void gemm_tn_kernel(
    const float* __restrict__ A, int lda, const float* __restrict__ B, int ldb,
    float* __restrict__ slab, int M, int N, int K, int kchunk) {
    __shared__ __attribute__((aligned(16))) float lds[2 * 2 * BK * LDM];
    constexpr int TILE = 2 * BK * LDM;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int m0 = blockIdx.x * BM, n0 = blockIdx.y * BM;
    const int kbeg = blockIdx.z * kchunk;
    const int kend = min(K, kbeg + kchunk);
    const int nk = kend > kbeg ? (kend - kbeg + BK - 1) / BK : 0;
    const int lk = tid >> 5, cg = tid & 31;   // k row (0..7)+8*s, column group of 4

    auto ld = [&](const float* P, int ldp, int c0, int lim, int s, int kt) -> f32x4 {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        const int k = kbeg + kt * BK + lk + 8 * s, c = c0 + cg * 4;
        if (k < kend && c < lim) v = *reinterpret_cast<const f32x4*>(P + (size_t)k * ldp + c);
        return v;
    };
    f32x16 acc[2][2];
    acc_clear(acc);

    f32x4 ra[4], rb[4];
    auto fetch = [&](int kt) {
#pragma unroll
        for (int s = 0; s < 4; ++s) { ra[s] = ld(A, lda, m0, M, s, kt); rb[s] = ld(B, ldb, n0, N, s, kt); }
    };
    auto stash = [&](int buf) {
        float* As = lds + buf * TILE;
        float* Bs = As + BK * LDM;
#pragma unroll
        for (int s = 0; s < 4; ++s) {
            *reinterpret_cast<f32x4*>(As + (lk + 8 * s) * LDM + cg * 4) = ra[s];
            *reinterpret_cast<f32x4*>(Bs + (lk + 8 * s) * LDM + cg * 4) = rb[s];
        }
    };
    if (nk > 0) { fetch(0); stash(0); }
    __syncthreads();
    const int i = lane & 31, kh = lane >> 5;
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = kt + 1 < nk;
        if (more) fetch(kt + 1);
        const float* As = lds + (kt & 1) * TILE;
        const float* Bs = As + BK * LDM;
#pragma unroll
        for (int s = 0; s < BK / 2; ++s) {
            float a[2], b[2];
#pragma unroll
            for (int t = 0; t < 2; ++t) {
                a[t] = As[(2 * s + kh) * LDM + wm * 64 + t * 32 + i];
                b[t] = Bs[(2 * s + kh) * LDM + wn * 64 + t * 32 + i];
            }
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < 2; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm], b[tn], acc[tm][tn], 0, 0, 0);
        }
        if (more) stash((kt + 1) & 1);
        __syncthreads();
    }
    float* out = slab + (size_t)blockIdx.z * M * N;
    const int col = lane & 31;
#pragma unroll
    for (int tn = 0; tn < 2; ++tn) {
        const int n = n0 + wn * 64 + tn * 32 + col;
        if (n >= N) continue;
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int r = 0; r < 16; ++r) {
                const int m = frag_row(m0 + wm * 64 + tm * 32, kh, r);
                if (m < M) out[(size_t)m * N + n] = acc[tm][tn][r];
            }
    }
}

__global__ void slab_reduce_kernel(const float* __restrict__ slab, float* __restrict__ C, int ldc,
                                   int M, int N, int splits, int accumulate) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= M * N) return;
    const int m = idx / N, n = idx - m * N;
    float s = 0.f;
    for (int z = 0; z < splits; ++z) s += slab[(size_t)z * M * N + idx];
    float* c = C + (size_t)m * ldc + n;
    *c = accumulate ? (*c + s) : s;
}

}  // namespace

extern "C" int ntk_gemm_nt_f32(const float* A, int lda, const float* B, int ldb, const float* bias,
                               float* C, int ldc, int M, int N, int K, void* stream) {
    NTK_REQUIRE(A && B && C, NTK_ERR_BAD_PTR, "ntk_gemm_nt_f32: null pointer");
    NTK_REQUIRE(ntk_aligned16(A) && ntk_aligned16(B), NTK_ERR_BAD_PTR, "ntk_gemm_nt_f32: A, B must be 16-byte aligned");
    NTK_REQUIRE(M > 0 && N > 0 && K > 0 && (K % 4) == 0 && (lda % 4) == 0 && (ldb % 4) == 0 && lda >= K &&
                    ldb >= K && ldc >= N,
                NTK_ERR_BAD_SHAPE, "ntk_gemm_nt_f32: M=%d N=%d K=%d lda=%d ldb=%d ldc=%d (K, lda, ldb multiples of 4)",
                M, N, K, lda, ldb, ldc);
    hipStream_t st = (hipStream_t)stream;
    if (N > 64) {
        dim3 grid((M + BM - 1) / BM, (N + 127) / 128);
        gemm_nt_kernel<128><<<grid, 256, 0, st>>>(A, lda, B, ldb, bias, C, ldc, M, N, K);
    } else {
        dim3 grid((M + BM - 1) / BM, 1);
        gemm_nt_kernel<64><<<grid, 256, 0, st>>>(A, lda, B, ldb, bias, C, ldc, M, N, K);
    }
    NTK_CHECK_LAUNCH("ntk_gemm_nt_f32");
    return NTK_OK;
}

extern "C" size_t ntk_gemm_tn_workspace_bytes(int M, int N, int splits) {
    if (M <= 0 || N <= 0 || splits <= 0) return 0;
    return (size_t)M * N * splits * sizeof(float);
}

extern "C" int ntk_gemm_tn_f32(const float* A, int lda, const float* B, int ldb, float* C, int ldc,
                               int M, int N, int K, int splits, int accumulate, float* workspace,
                               void* stream) {
    NTK_REQUIRE(A && B && C && workspace, NTK_ERR_BAD_PTR, "ntk_gemm_tn_f32: null pointer");
    NTK_REQUIRE(ntk_aligned16(A) && ntk_aligned16(B), NTK_ERR_BAD_PTR, "ntk_gemm_tn_f32: A, B must be 16-byte aligned");
    NTK_REQUIRE(M > 0 && N > 0 && K > 0 && splits > 0 && splits <= 65535 && (M % 4) == 0 && (N % 4) == 0 &&
                    (lda % 4) == 0 && (ldb % 4) == 0 && lda >= M && ldb >= N && ldc >= N,
                NTK_ERR_BAD_SHAPE,
                "ntk_gemm_tn_f32: M=%d N=%d K=%d splits=%d lda=%d ldb=%d ldc=%d (M, N, lda, ldb multiples of 4)",
                M, N, K, splits, lda, ldb, ldc);
    hipStream_t st = (hipStream_t)stream;
    int kchunk = (K + splits - 1) / splits;
    kchunk = ((kchunk + BK - 1) / BK) * BK;
    dim3 grid((M + BM - 1) / BM, (N + BM - 1) / BM, splits);
    gemm_tn_kernel<<<grid, 256, 0, st>>>(A, lda, B, ldb, workspace, M, N, K, kchunk);
    NTK_CHECK_LAUNCH("ntk_gemm_tn_f32");
    const int total = M * N;
    slab_reduce_kernel<<<(total + 255) / 256, 256, 0, st>>>(workspace, C, ldc, M, N, splits, accumulate);
    NTK_CHECK_LAUNCH("ntk_gemm_tn_f32(reduce)");
    return NTK_OK;
}
