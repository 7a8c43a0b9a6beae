// The fp32 MFMA tile (v_mfma_f32_32x32x2_f32) that the plain GEMMs (gemm_f32.hip) and the direct conv (conv_direct.hip) share:
// 128 x BN x 32 per 256-thread workgroup, 4 waves as 2x2, each wave a 64 x BN/2 block of 32x32 fragments held as acc[2][BN/64].
// Operands are staged global -> VGPR -> LDS; the next K-tile's global loads are in flight while the current tile's MFMAs issue.
#pragma once
#include "common.h"

constexpr int BM = 128;
constexpr int BK = 32;
constexpr int LDT = BK + 4;   // LDS row stride (floats): conflict-free ds_read_b128 (36*i mod 64 distinct slots)

template <int TM, int TN>
__device__ __forceinline__ void acc_clear(f32x16 (&acc)[TM][TN]) {
#pragma unroll
    for (int tm = 0; tm < TM; ++tm)
#pragma unroll
        for (int tn = 0; tn < TN; ++tn)
#pragma unroll
            for (int r = 0; r < 16; ++r) acc[tm][tn][r] = 0.f;
}

// Row that accumulator register r of a lane holds, in a 32x32 fragment whose first row is `base` (kh = lane >> 5; the column is
// lane & 31): four consecutive registers are four consecutive rows.
__device__ __forceinline__ constexpr int frag_row(int base, int kh, int r) { return base + 4 * kh + (r & 3) + 8 * (r >> 2); }

// ---------------------------------------------------------------------------
// one K-tile of MFMAs from LDS images As[BM][LDT], Bs[BN][LDT] (K contiguous)
// lane l supplies A[row l&31][k] and B[k][col l&31] with k picked by l>>5.
// ---------------------------------------------------------------------------
template <int BN>
__device__ __forceinline__ void mma_ktile(const float* __restrict__ As, const float* __restrict__ Bs,
                                          f32x16 (&acc)[2][BN / 64], int wm, int wn, int lane) {
    constexpr int TN = BN / 64;
    const int i = lane & 31, kh = lane >> 5;
    const float* ap = As + (wm * 64 + i) * LDT + kh * 4;
    const float* bp = Bs + (wn * (BN / 2) + i) * LDT + kh * 4;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        f32x4 a[2], b[TN];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) a[tm] = *reinterpret_cast<const f32x4*>(ap + tm * 32 * LDT + q * 8);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) b[tn] = *reinterpret_cast<const f32x4*>(bp + tn * 32 * LDT + q * 8);
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][e], b[tn][e], acc[tm][tn], 0, 0, 0);
    }
}

// generic pipelines.  LA/LB: functors  f32x4 operator()(int slot, int kt)
// slot = which of the thread's rows (A: 4 rows, B: BN/32 rows); LDS row = (tid>>3) + 32*slot, k-group = tid&7
template <int BN, class LA, class LB>
__device__ __forceinline__ void gemm_pipeline_sb(LA& la, LB& lb, int nk, float* lds, f32x16 (&acc)[2][BN / 64]) {
    // single LDS buffer: registers hold tile kt+1 while tile kt is consumed; two barriers per K-tile,
    // half the LDS footprint -> one more workgroup per CU
    constexpr int NB = BN / 32;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = tid >> 3, kg = tid & 7;
    float* As = lds;
    float* Bs = lds + BM * LDT;
    f32x4 ra[4], rb[NB];
#pragma unroll
    for (int s = 0; s < 4; ++s) ra[s] = la(s, 0);
#pragma unroll
    for (int s = 0; s < NB; ++s) rb[s] = lb(s, 0);
    for (int kt = 0; kt < nk; ++kt) {
#pragma unroll
        for (int s = 0; s < 4; ++s) *reinterpret_cast<f32x4*>(As + (lrow + 32 * s) * LDT + kg * 4) = ra[s];
#pragma unroll
        for (int s = 0; s < NB; ++s) *reinterpret_cast<f32x4*>(Bs + (lrow + 32 * s) * LDT + kg * 4) = rb[s];
        __syncthreads();
        if (kt + 1 < nk) {
#pragma unroll
            for (int s = 0; s < 4; ++s) ra[s] = la(s, kt + 1);
#pragma unroll
            for (int s = 0; s < NB; ++s) rb[s] = lb(s, kt + 1);
        }
        mma_ktile<BN>(As, Bs, acc, wm, wn, lane);
        __syncthreads();
    }
}

// two LDS buffers (the plain GEMM kernels: their tiles are small and they run at 2 workgroups/CU)
template <int BN, class LA, class LB>
__device__ __forceinline__ void gemm_pipeline(LA& la, LB& lb, int nk, float* lds, f32x16 (&acc)[2][BN / 64]) {
    constexpr int NB = BN / 32;
    constexpr int TILE = (BM + BN) * LDT;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int lrow = tid >> 3, kg = tid & 7;
    f32x4 ra[4], rb[NB];
#pragma unroll
    for (int s = 0; s < 4; ++s) ra[s] = la(s, 0);
#pragma unroll
    for (int s = 0; s < NB; ++s) rb[s] = lb(s, 0);
    {
        float* As = lds;
        float* Bs = lds + BM * LDT;
#pragma unroll
        for (int s = 0; s < 4; ++s) *reinterpret_cast<f32x4*>(As + (lrow + 32 * s) * LDT + kg * 4) = ra[s];
#pragma unroll
        for (int s = 0; s < NB; ++s) *reinterpret_cast<f32x4*>(Bs + (lrow + 32 * s) * LDT + kg * 4) = rb[s];
    }
    __syncthreads();
    for (int kt = 0; kt < nk; ++kt) {
        const bool more = (kt + 1 < nk);
        if (more) {
#pragma unroll
            for (int s = 0; s < 4; ++s) ra[s] = la(s, kt + 1);
#pragma unroll
            for (int s = 0; s < NB; ++s) rb[s] = lb(s, kt + 1);
        }
        const float* As = lds + (kt & 1) * TILE;
        mma_ktile<BN>(As, As + BM * LDT, acc, wm, wn, lane);
        if (more) {
            float* An = lds + ((kt + 1) & 1) * TILE;
            float* Bn = An + BM * LDT;
#pragma unroll
            for (int s = 0; s < 4; ++s) *reinterpret_cast<f32x4*>(An + (lrow + 32 * s) * LDT + kg * 4) = ra[s];
#pragma unroll
            for (int s = 0; s < NB; ++s) *reinterpret_cast<f32x4*>(Bn + (lrow + 32 * s) * LDT + kg * 4) = rb[s];
        }
        __syncthreads();
    }
}
