// Direct implicit-GEMM conv3x3 SAME + bias + ReLU (+ fused 2x2/2 max-pool) over NHWC activations -- VGG conv1_1..conv4_3
// (vgg.py:155-161).  The default trunk runs other forms (conv_bf16p.hip, conv_wino43.hip, conv_wino.hip); this file takes what
// they do not: algo="direct", tiny-Cin / odd shapes, conv1_1 when the stem is separate, and the tile form of BASELINE config 5
// ("bf16 MFMA conv + fp32 memory").
//
// Tile: 128 rows x BN columns per 256-thread workgroup (mfma_tile.h), rows in 4x4-pixel patch order so that the pool is four
// consecutive accumulator registers, row tiles dealt to the XCDs.  Three kernels share the row-tile prologue and the epilogue:
//   * the LDS-DMA tile kernel, fp32 (v_mfma_f32_32x32x2_f32) or bf16 operands (v_mfma_f32_32x32x16_bf16, fp32 accumulation,
//     output rounded once on store): global_load_lds_dwordx4 frees the staging VGPRs -> 128 VGPRs, 32 KB LDS, FOUR workgroups
//     per CU.  Measured on MI355X (profiles/): co-resident waves of one SIMD run in lockstep and stall at their
//     barriers together, so occupancy decides the matrix pipe's duty cycle: 132-133 TFLOP/s per fp32 layer against 126-128 for
//     VGPR staging at 3 workgroups per CU (two LDS buffers at 2 workgroups/CU, static wave priority, 4 workgroups/CU with spills
//     were measured slower and removed);
//   * the VGPR-staged kernel, kept for tiny Cin (the whole K = 9*Cin in one K-tile, scalar gather);
//   * conv1_1's row kernel (3 -> 64 channels, W % 32 == 0, no pool).
#include "mfma_tile.h"

// Ablation switches for scripts/dev_wino_variant.sh (timing only; never defined in the product build): bit 0 no global -> LDS
// staging after the first K-tile, bit 1 no MFMAs, bit 2 no barriers in the K loop, bit 3 no output stores.
#ifndef CONV_DIRECT_ABL
#define CONV_DIRECT_ABL 0
#endif

namespace {

typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));

__device__ __forceinline__ bf16x8 as_bf16x8(const f32x4& v) {
    union { f32x4 f; bf16x8 b; } u;
    u.f = v;
    return u.b;
}

// ---------------------------------------------------------------------------
// Row tile.  GEMM row m <-> output pixel, ordered so that the 4 pixels of every 2x2 pooling window are 4 consecutive rows
// (= the 4 consecutive accumulator registers r&3 of one lane): rows are grouped in 4x4 pixel patches, patch-major over
// (frame, py, px); inside a patch q = m & 15 -> window (q>>3, (q>>2)&1), pixel-in-window ((q>>1)&1, q&1).
// ---------------------------------------------------------------------------
struct ConvRows {     // a tile's BM rows, in LDS (a kernel that never reads one of the tables does not keep it)
    int* pix;       // linear pixel index (n*H + y)*W + x, or -1 past the end
    int* yx;        // y << 16 | x
    int* ppix;      // pooled linear pixel index (n*H/2 + y/2)*(W/2) + x/2
};

// Workgroup id -> (m0, n0), false past the last row tile; fills the tile's row table.  XCD-aware tile order (1-D grid):
// workgroups b, b+8, b+16, ... share an XCD (round-robin dispatch, speed only).  Inside an XCD consecutive workgroups take the
// column tiles of ONE row tile, so the A rows that every column tile re-reads are served by that XCD's L2 instead of being fetched
// once per column tile.
template <int BN>
__device__ __forceinline__ bool conv_row_tile(const ConvRows& rows, int npatch, int H, int W, int Cout, int& m0, int& n0) {
    const int tid = threadIdx.x;
    const int ctiles = Cout / BN;
    const int xcd = blockIdx.x & 7, li = blockIdx.x >> 3;
    m0 = ((li / ctiles) * 8 + xcd) * BM;
    n0 = (li % ctiles) * BN;
    if (m0 >= npatch * 16) return false;
    if (tid < BM) {
        const int m = m0 + tid, patch = m >> 4, q = m & 15;
        int pix = -1, yx = 0, ppix = -1;
        if (patch < npatch) {
            const int PW = W >> 2, PH = H >> 2;
            const int px = patch % PW;
            const int t = patch / PW;
            const int py = t % PH;
            const int n = t / PH;
            const int y = py * 4 + (q >> 3) * 2 + ((q >> 1) & 1);
            const int x = px * 4 + ((q >> 2) & 1) * 2 + (q & 1);
            pix = (n * H + y) * W + x;
            yx = (y << 16) | x;
            ppix = (n * (H >> 1) + (y >> 1)) * (W >> 1) + (x >> 1);
        }
        rows.pix[tid] = pix; rows.yx[tid] = yx; rows.ppix[tid] = ppix;
    }
    __syncthreads();
    return true;
}

// bias + ReLU (+ 2x2 max over the 4 consecutive rows of a window), rounded to OutT (float or __bf16) on store
template <int BN, bool POOL, class OutT>
__device__ __forceinline__ void conv_epilogue(const f32x16 (&acc)[2][BN / 64], const ConvRows& rows, const float* __restrict__ bias,
                                              OutT* __restrict__ out, int Cout, int n0) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    const int kh = lane >> 5, col = lane & 31;
#pragma unroll
    for (int tn = 0; tn < BN / 64; ++tn) {
        const int n = n0 + wn * (BN / 2) + tn * 32 + col;
        const float bv = bias[n];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) {
            const int mbase = wm * 64 + tm * 32;
            if constexpr (!POOL) {
#pragma unroll
                for (int r = 0; r < 16; ++r) {
                    const int pix = rows.pix[frag_row(mbase, kh, r)];
                    if (pix >= 0 && ((CONV_DIRECT_ABL & 8) == 0 || acc[tm][tn][r] == 12345.f))
                        out[(size_t)pix * Cout + n] = (OutT)fmaxf(acc[tm][tn][r] + bv, 0.f);
                }
            } else {
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    const int pp = rows.ppix[frag_row(mbase, kh, 4 * g)];
                    const float v = fmaxf(fmaxf(acc[tm][tn][4 * g], acc[tm][tn][4 * g + 1]),
                                          fmaxf(acc[tm][tn][4 * g + 2], acc[tm][tn][4 * g + 3]));
                    if (pp >= 0 && ((CONV_DIRECT_ABL & 8) == 0 || v == 12345.f))
                        out[(size_t)pp * Cout + n] = (OutT)fmaxf(v + bv, 0.f);
                }
            }
        }
    }
}

// ---------------------------------------------------------------------------
// LDS-DMA tile kernel: operands go global -> LDS by global_load_lds_dwordx4 (no VGPR staging, no ds_write), one un-padded
// XOR-swizzled LDS buffer.  A K-tile is 128 B per row for either operand type; LDS image: row r at byte r*128, its 16-byte
// chunk c stored in slot c ^ ((r >> 1) & 7): every ds_read_b128 lane group of the fragment reads then touches 16 distinct
// 4-bank slots (rows of one parity x 8 slots).  One DMA wave-instruction fills 8 rows (1 KB, lane-linear), so the swizzle is
// applied to the per-lane SOURCE address.  Zero padding (image border, rows past the end) is fetched from a zero page.
// K order: KT-channel chunk outer, the 9 taps inner -- the nine shifted reads of one channel chunk are consecutive K-tiles, so
// their overlapping 128-B lines are re-read while still L2 (mostly L1) resident.
// ---------------------------------------------------------------------------
// Operand traits: element type, elements per 16-byte chunk and per K-tile, and the MFMAs that consume one ds_read_b128 per
// fragment (a bf16 MFMA takes what four fp32 MFMAs do).
struct OperandF32 {
    using T = float;
    static constexpr int CHUNK = 4, KT = 32;
    template <int TN>
    static __device__ __forceinline__ void mma(const f32x4 (&a)[2], const f32x4 (&b)[TN], f32x16 (&acc)[2][TN]) {
#pragma unroll
        for (int e = 0; e < 4; ++e)
#pragma unroll
            for (int tm = 0; tm < 2; ++tm)
#pragma unroll
                for (int tn = 0; tn < TN; ++tn)
                    acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x2f32(a[tm][e], b[tn][e], acc[tm][tn], 0, 0, 0);
    }
};
struct OperandBf16 {
    using T = __bf16;
    static constexpr int CHUNK = 8, KT = 64;
    template <int TN>
    static __device__ __forceinline__ void mma(const f32x4 (&a)[2], const f32x4 (&b)[TN], f32x16 (&acc)[2][TN]) {
#pragma unroll
        for (int tm = 0; tm < 2; ++tm)
#pragma unroll
            for (int tn = 0; tn < TN; ++tn)
                acc[tm][tn] = __builtin_amdgcn_mfma_f32_32x32x16_bf16(as_bf16x8(a[tm]), as_bf16x8(b[tn]), acc[tm][tn], 0, 0, 0);
    }
};

constexpr int ROWF = 32;      // floats per LDS row (128 bytes)

__device__ __attribute__((aligned(128))) float g_zero_page[32];

__device__ __forceinline__ void lds_dma16(const void* src, float* lds_wave_base) {
    __builtin_amdgcn_global_load_lds((const __attribute__((address_space(1))) void*)src,
                                     (__attribute__((address_space(3))) void*)lds_wave_base, 16, 0, 0);
}

template <class Op, int BN>
__device__ __forceinline__ void mma_ktile_swz(const float* __restrict__ As, const float* __restrict__ Bs,
                                              f32x16 (&acc)[2][BN / 64], int wm, int wn, int lane) {
    constexpr int TN = BN / 64;
    const int i = lane & 31, kh = lane >> 5, f = (i >> 1) & 7;
    const float* ap = As + (wm * 64 + i) * ROWF;
    const float* bp = Bs + (wn * (BN / 2) + i) * ROWF;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
        const int slot = ((2 * q + kh) ^ f) * 4;
        f32x4 a[2], b[TN];
#pragma unroll
        for (int tm = 0; tm < 2; ++tm) a[tm] = *reinterpret_cast<const f32x4*>(ap + tm * 32 * ROWF + slot);
#pragma unroll
        for (int tn = 0; tn < TN; ++tn) b[tn] = *reinterpret_cast<const f32x4*>(bp + tn * 32 * ROWF + slot);
        Op::template mma<TN>(a, b, acc);
    }
}

template <class Op, int BN, bool POOL, class OutT>
__global__ __launch_bounds__(256, 4) void conv3x3_relu_dma_kernel(
    const typename Op::T* __restrict__ in, const typename Op::T* __restrict__ wp, const float* __restrict__ bias,
    OutT* __restrict__ out, int npatch, int H, int W, int Cin, int Cout, int Kp) {
    constexpr int TN = BN / 64, NBI = BN / 32;      // B DMA instructions per wave
    __shared__ __attribute__((aligned(1024))) float lds[(BM + BN) * ROWF];
    __shared__ int s_pix[BM], s_yx[BM], s_ppix[BM];
    const ConvRows rows = {s_pix, s_yx, s_ppix};

    int m0, n0;
    if (!conv_row_tile<BN>(rows, npatch, H, W, Cout, m0, n0)) return;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int wm = wave >> 1, wn = wave & 1;
    // DMA roles: instruction jj of this wave fills tile rows (wave*4 + jj)*8 .. +7; lane -> (row = lane>>3, slot = lane&7)
    const int lr = lane >> 3, slot = lane & 7;
    int rpix[4], ry[4], rx[4], achunk[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
        const int r = (wave * 4 + jj) * 8 + lr;
        rpix[jj] = rows.pix[r];
        const int yx = rows.yx[r];
        ry[jj] = yx >> 16; rx[jj] = yx & 0xffff;
        achunk[jj] = (slot ^ ((r >> 1) & 7)) * Op::CHUNK;
    }
    const typename Op::T* bsrc[NBI];
#pragma unroll
    for (int jj = 0; jj < NBI; ++jj) {
        const int r = (wave * NBI + jj) * 8 + lr;
        bsrc[jj] = wp + (size_t)(n0 + r) * Kp + (slot ^ ((r >> 1) & 7)) * Op::CHUNK;
    }
    float* As = lds;
    float* Bs = lds + BM * ROWF;
    f32x16 acc[2][TN];
    acc_clear(acc);

    const int nk = Kp / Op::KT;
    for (int kt = 0; kt < nk; ++kt) {
        const int chunk = kt / 9, tap = kt - chunk * 9;
        const int c0 = chunk * Op::KT;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        if ((CONV_DIRECT_ABL & 4) == 0 && kt > 0) __syncthreads();      // every wave has finished reading the previous tile
        if ((CONV_DIRECT_ABL & 1) == 0 || kt == 0) {
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) {
                const int yy = ry[jj] + dy, xx = rx[jj] + dx;
                const bool ok = rpix[jj] >= 0 && (unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W;
                const void* src = ok ? (const void*)(in + (size_t)(rpix[jj] + dy * W + dx) * Cin + c0 + achunk[jj])
                                     : (const void*)(g_zero_page + (lane & 7) * 4);
                lds_dma16(src, As + (wave * 4 + jj) * 8 * ROWF);
            }
#pragma unroll
            for (int jj = 0; jj < NBI; ++jj) lds_dma16(bsrc[jj] + kt * Op::KT, Bs + (wave * NBI + jj) * 8 * ROWF);
        }
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        if ((CONV_DIRECT_ABL & 4) == 0) __syncthreads();                // all four waves' DMA has landed
        if ((CONV_DIRECT_ABL & 2) == 0) mma_ktile_swz<Op, BN>(As, Bs, acc, wm, wn, lane);
    }
    conv_epilogue<BN, POOL>(acc, rows, bias, out, Cout, n0);
}

// ---------------------------------------------------------------------------
// Tiny Cin (conv1_1, Cin = 3): the whole K = 9*Cin, k = tap*Cin + c, fits one K-tile; operands staged global -> VGPR -> LDS
// (scalar gather) in one LDS buffer, 3 workgroups per CU.
// ---------------------------------------------------------------------------
template <int BN, bool POOL, class OutT>
__global__ __launch_bounds__(256, 3) void conv3x3_relu_smallc_kernel(
    const float* __restrict__ in, const float* __restrict__ wp, const float* __restrict__ bias,
    OutT* __restrict__ out, int npatch, int H, int W, int Cin, int Cout, int Kp) {
    __shared__ __attribute__((aligned(16))) float lds[(BM + BN) * LDT];
    __shared__ int s_pix[BM], s_yx[BM], s_ppix[BM];
    const ConvRows rows = {s_pix, s_yx, s_ppix};

    int m0, n0;
    if (!conv_row_tile<BN>(rows, npatch, H, W, Cout, m0, n0)) return;
    const int tid = threadIdx.x;
    const int lrow = tid >> 3, kg = tid & 7;
    int rpix[4], ry[4], rx[4];
#pragma unroll
    for (int s = 0; s < 4; ++s) {
        rpix[s] = rows.pix[lrow + 32 * s];
        const int yx = rows.yx[lrow + 32 * s];
        ry[s] = yx >> 16; rx[s] = yx & 0xffff;
    }

    auto la = [&](int s, int kt) -> f32x4 {
        f32x4 v = {0.f, 0.f, 0.f, 0.f};
        if (rpix[s] >= 0) {
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int k = kg * 4 + e;
                if (k < 9 * Cin) {
                    const int tap = k / Cin, c = k - tap * Cin;
                    const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
                    const int yy = ry[s] + dy, xx = rx[s] + dx;
                    if ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W)
                        v[e] = in[(size_t)(rpix[s] + dy * W + dx) * Cin + c];
                }
            }
        }
        return v;
    };
    auto lb = [&](int s, int kt) -> f32x4 {
        return *reinterpret_cast<const f32x4*>(wp + (size_t)(n0 + lrow + 32 * s) * Kp + kt * BK + kg * 4);
    };

    f32x16 acc[2][BN / 64];
    acc_clear(acc);
    gemm_pipeline_sb<BN>(la, lb, Kp / BK, lds, acc);
    conv_epilogue<BN, POOL>(acc, rows, bias, out, Cout, n0);
}

// ---------------------------------------------------------------------------
// conv1_1 (Cin = 3 -> Cout = 64, no pool): dedicated persistent kernel.  The layer is bound by its 12.8 MB/frame
// of output stores, not by its 27-deep contraction, so the generic tile kernel's per-workgroup set-up (250 000
// workgroups for a 640-frame batch) is what it pays for.  Here a wave owns 32 consecutive pixels of one image row x
// all 64 channels: K = 27 (+1 zero) = 14 steps of v_mfma_f32_32x32x2_f32 x 2 column blocks, the A operand gathered
// straight from the 3-channel frame (L1 hits: every input value is used by 9 taps of 3 rows), the 28 x 64 weights
// resident in registers for the whole kernel, and waves stride over the row segments of the batch.
// Same arithmetic as the tile kernel: a k-ordered fp32 MFMA chain over k = tap * 3 + c.
// ---------------------------------------------------------------------------
template <bool OUTBF16>        // OUTBF16: conv1_1 of the bf16 trunk (config 5): the same fp32 arithmetic, rounded once on store
__global__ __launch_bounds__(256, 4) void conv_c3_rows_kernel(const float* __restrict__ in, const float* __restrict__ wp,
                                                              const float* __restrict__ bias, float* __restrict__ out,
                                                              int nseg, int H, int W) {
    const int lane = threadIdx.x & 63, m = lane & 31, kh = lane >> 5;
    const int gw = blockIdx.x * 4 + (threadIdx.x >> 6), nw = gridDim.x * 4;
    float b0[14], b1[14];
    int off[14], dyv[14], dxv[14];
#pragma unroll
    for (int s = 0; s < 14; ++s) {
        const int k = 2 * s + kh;                       // < 28; k = 27 is the zero pad column of the packed weights
        b0[s] = wp[m * 32 + k];
        b1[s] = wp[(32 + m) * 32 + k];
        const int tap = k / 3, c = k - tap * 3;
        const int dy = tap / 3 - 1, dx = tap - (tap / 3) * 3 - 1;
        dyv[s] = (k < 27) ? dy : 4;                     // 4: never inside the image
        dxv[s] = dx;
        off[s] = (dy * W + dx) * 3 + c;
    }
    const float bv0 = bias[m], bv1 = bias[32 + m];
    const int spr = W >> 5;                             // 32-pixel segments per row
    for (int seg = gw; seg < nseg; seg += nw) {
        const int xs = seg % spr;
        const int t = seg / spr;
        const int y = t % H;                            // t = f * H + y
        const int x = xs * 32 + m;
        const float* base = in + ((size_t)t * W + x) * 3;
        f32x16 acc0, acc1;
#pragma unroll
        for (int r = 0; r < 16; ++r) { acc0[r] = 0.f; acc1[r] = 0.f; }
        float av[14];
#pragma unroll
        for (int s = 0; s < 14; ++s) {
            const int yy = y + dyv[s], xx = x + dxv[s];
            av[s] = ((unsigned)yy < (unsigned)H && (unsigned)xx < (unsigned)W) ? base[off[s]] : 0.f;
        }
#pragma unroll
        for (int s = 0; s < 14; ++s) {
            acc0 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], b0[s], acc0, 0, 0, 0);
            acc1 = __builtin_amdgcn_mfma_f32_32x32x2f32(av[s], b1[s], acc1, 0, 0, 0);
        }
        const size_t o0 = ((size_t)t * W + xs * 32) * 64;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
            const int mm = frag_row(0, kh, r);
            const float v0 = fmaxf(acc0[r] + bv0, 0.f), v1 = fmaxf(acc1[r] + bv1, 0.f);
            if constexpr (OUTBF16) {
                __bf16* orow = reinterpret_cast<__bf16*>(out) + o0;
                orow[(size_t)mm * 64 + m] = (__bf16)v0;
                orow[(size_t)mm * 64 + 32 + m] = (__bf16)v1;
            } else {
                float* orow = out + o0;
                // non-temporal: 8.2 GB of activations per 640-frame pass that the next launch re-reads from HBM anyway (2.53 -> 2.46 ms)
                __builtin_nontemporal_store(v0, orow + (size_t)mm * 64 + m);
                __builtin_nontemporal_store(v1, orow + (size_t)mm * 64 + 32 + m);
            }
        }
    }
}

// HWIO [3,3,Cin,Cout] -> [Cout][Kp].  Cin % 32 == 0: k = (c/32)*288 + tap*32 + c%32 (chunk outer, tap inner);
// tiny Cin (conv1_1): k = tap*Cin + c, zero padded to Kp.
__global__ void pack_weights_kernel(const float* __restrict__ w, float* __restrict__ wp, int Cin, int Cout, int Kp) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Cout * Kp) return;
    const int n = idx / Kp, k = idx - n * Kp;
    float v = 0.f;
    if (k < 9 * Cin) {
        int tap, c;
        if ((Cin % BK) == 0) { const int chunk = k / (9 * BK), r = k - chunk * 9 * BK; tap = r / BK; c = chunk * BK + (r - tap * BK); }
        else { tap = k / Cin; c = k - tap * Cin; }
        v = w[(size_t)(tap * Cin + c) * Cout + n];   // HWIO flat index = (tap*Cin + c)*Cout + n
    }
    wp[idx] = v;
}

// HWIO fp32 [3,3,Cin,Cout] -> bf16 [Cout][Kp], k = (c/64)*576 + tap*64 + c%64 (Cin % 64 == 0)
__global__ void pack_weights_bf16_kernel(const float* __restrict__ w, __bf16* __restrict__ wp, int Cin, int Cout, int Kp) {
    constexpr int KT = OperandBf16::KT;
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= Cout * Kp) return;
    const int n = idx / Kp, k = idx - n * Kp;
    const int chunk = k / (9 * KT), r = k - chunk * 9 * KT;
    const int tap = r / KT, c = chunk * KT + (r - tap * KT);
    wp[idx] = (__bf16)w[(size_t)(tap * Cin + c) * Cout + n];
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
// What the three conv entries ask of every call: pointers, frame shape, and a row index that stays below 2^31.
int conv_check_frames(const char* who, bool ptrs_ok, bool aligned, int frames, int H, int W, long& npatch) {
    NTK_REQUIRE(ptrs_ok, NTK_ERR_BAD_PTR, "%s: null pointer", who);
    NTK_REQUIRE(aligned, NTK_ERR_BAD_PTR, "%s: pointers must be 16-byte aligned", who);
    NTK_REQUIRE(frames > 0 && H > 0 && W > 0 && (H % 4) == 0 && (W % 4) == 0 && H < 32768 && W < 32768, NTK_ERR_BAD_SHAPE,
                "%s: frames=%d H=%d W=%d (H, W must be multiples of 4)", who, frames, H, W);
    npatch = (long)frames * (H / 4) * (W / 4);
    NTK_REQUIRE(npatch * 16 < 2147483647L - BM, NTK_ERR_BAD_SHAPE, "%s: %ld pixels exceed the 2^31 row index range", who, npatch * 16);
    return NTK_OK;
}

// row tiles rounded up to the eight XCDs x column tiles (conv_row_tile)
dim3 conv_grid(long npatch, int ctiles) {
    const long rtiles = (npatch * 16 + BM - 1) / BM;
    return dim3((unsigned)(((rtiles + 7) / 8) * 8 * ctiles));
}

template <class Op, class OutT>
void launch_dma(const void* in, const void* wp, const float* bias, void* out, long npatch, int H, int W, int cin, int cout,
                int Kp, int pool, hipStream_t st) {
    auto go = [&](auto kernel, int bn) {
        kernel<<<conv_grid(npatch, cout / bn), 256, 0, st>>>((const typename Op::T*)in, (const typename Op::T*)wp, bias, (OutT*)out,
                                                              (int)npatch, H, W, cin, cout, Kp);
    };
    if ((cout % 128) == 0) pool ? go(conv3x3_relu_dma_kernel<Op, 128, true, OutT>, 128) : go(conv3x3_relu_dma_kernel<Op, 128, false, OutT>, 128);
    else pool ? go(conv3x3_relu_dma_kernel<Op, 64, true, OutT>, 64) : go(conv3x3_relu_dma_kernel<Op, 64, false, OutT>, 64);
}

// conv1_1's row kernel: 256 CUs x 4 workgroups, waves stride over segments (4 096 / 16 384 shorter-lived workgroups measured the
// same, alone and in the step)
template <bool OUTBF16>
int launch_c3_rows(const char* who, const float* in, const float* wp, const float* bias, void* out, int frames, int H, int W,
                   hipStream_t st) {
    const long nseg = (long)frames * H * (W / 32);
    NTK_REQUIRE(nseg < 2147483647L, NTK_ERR_BAD_SHAPE, "%s: %ld row segments", who, nseg);
    const int wgs = (int)((nseg + 3) / 4 < 1024 ? (nseg + 3) / 4 : 1024);
    conv_c3_rows_kernel<OUTBF16><<<wgs, 256, 0, st>>>(in, wp, bias, reinterpret_cast<float*>(out), (int)nseg, H, W);
    return NTK_OK;
}

}  // namespace

// ---------------------------------------------------------------------------
// C ABI
// ---------------------------------------------------------------------------
extern "C" int ntk_vgg_packed_k(int cin) { return ((9 * cin + BK - 1) / BK) * BK; }

extern "C" int ntk_vgg_pack_weights(const float* w_hwio, float* w_packed, int cin, int cout, void* stream) {
    NTK_REQUIRE(w_hwio && w_packed, NTK_ERR_BAD_PTR, "ntk_vgg_pack_weights: null pointer");
    NTK_REQUIRE(cin > 0 && cout > 0, NTK_ERR_BAD_SHAPE, "ntk_vgg_pack_weights: cin=%d cout=%d", cin, cout);
    const int Kp = ntk_vgg_packed_k(cin);
    const int total = cout * Kp;
    pack_weights_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(w_hwio, w_packed, cin, cout, Kp);
    NTK_CHECK_LAUNCH("ntk_vgg_pack_weights");
    return NTK_OK;
}

extern "C" int ntk_vgg_pack_weights_bf16(const float* w_hwio, void* w_packed_bf16, int cin, int cout, void* stream) {
    NTK_REQUIRE(w_hwio && w_packed_bf16, NTK_ERR_BAD_PTR, "ntk_vgg_pack_weights_bf16: null pointer");
    NTK_REQUIRE(cin > 0 && (cin % OperandBf16::KT) == 0 && cout > 0, NTK_ERR_BAD_SHAPE, "ntk_vgg_pack_weights_bf16: cin=%d (multiple of 64) cout=%d", cin, cout);
    const int Kp = 9 * cin, total = cout * Kp;
    pack_weights_bf16_kernel<<<(total + 255) / 256, 256, 0, (hipStream_t)stream>>>(w_hwio, reinterpret_cast<__bf16*>(w_packed_bf16), cin, cout, Kp);
    NTK_CHECK_LAUNCH("ntk_vgg_pack_weights_bf16");
    return NTK_OK;
}

extern "C" int ntk_vgg_conv3x3_relu_f32(const float* in, const float* w_packed, const float* bias,
                                        float* out, int frames, int H, int W, int cin, int cout,
                                        int fuse_pool, void* stream) {
    const char* who = "ntk_vgg_conv3x3_relu_f32";
    long npatch;
    if (int rc = conv_check_frames(who, in && w_packed && bias && out, ntk_aligned16(in) && ntk_aligned16(w_packed) && ntk_aligned16(out),
                                   frames, H, W, npatch)) return rc;
    NTK_REQUIRE(cout > 0 && (cout % 64) == 0, NTK_ERR_BAD_SHAPE,
                "ntk_vgg_conv3x3_relu_f32: cout=%d must be a multiple of 64", cout);
    const bool smallc = (cin % 32) != 0;
    NTK_REQUIRE(cin > 0 && (!smallc || 9 * cin <= BK), NTK_ERR_BAD_SHAPE,
                "ntk_vgg_conv3x3_relu_f32: cin=%d must be <= 3 or a multiple of 32", cin);
    const int Kp = ntk_vgg_packed_k(cin);
    hipStream_t st = (hipStream_t)stream;
    if (cin == 3 && cout == 64 && !fuse_pool && (W % 32) == 0) {
        if (int rc = launch_c3_rows<false>(who, in, w_packed, bias, out, frames, H, W, st)) return rc;
    } else if (!smallc) {
        launch_dma<OperandF32, float>(in, w_packed, bias, out, npatch, H, W, cin, cout, Kp, fuse_pool, st);
    } else {
        auto go = [&](auto kernel, int bn) {
            kernel<<<conv_grid(npatch, cout / bn), 256, 0, st>>>(in, w_packed, bias, out, (int)npatch, H, W, cin, cout, Kp);
        };
        if ((cout % 128) == 0) fuse_pool ? go(conv3x3_relu_smallc_kernel<128, true, float>, 128) : go(conv3x3_relu_smallc_kernel<128, false, float>, 128);
        else fuse_pool ? go(conv3x3_relu_smallc_kernel<64, true, float>, 64) : go(conv3x3_relu_smallc_kernel<64, false, float>, 64);
    }
    NTK_CHECK_LAUNCH("ntk_vgg_conv3x3_relu_f32");
    return NTK_OK;
}

// conv1_1 of the bf16 trunk: fp32 frames in, bf16 activations out (same arithmetic, rounded once on store)
extern "C" int ntk_vgg_conv3x3_relu_f32_to_bf16(const float* in, const float* w_packed, const float* bias, void* out_bf16,
                                                int frames, int H, int W, int cin, int cout, void* stream) {
    const char* who = "ntk_vgg_conv3x3_relu_f32_to_bf16";
    long npatch;
    if (int rc = conv_check_frames(who, in && w_packed && bias && out_bf16, /* asks no alignment */ true, frames, H, W, npatch)) return rc;
    NTK_REQUIRE(cin > 0 && 9 * cin <= BK && cout == 64, NTK_ERR_BAD_SHAPE,
                "ntk_vgg_conv3x3_relu_f32_to_bf16: cin=%d cout=%d (cin <= 3, cout == 64)", cin, cout);
    hipStream_t st = (hipStream_t)stream;
    if (cin == 3 && (W % 32) == 0) {            // the row kernel (4.06 -> store-bound at half the bytes: bit-identical results)
        if (int rc = launch_c3_rows<true>(who, in, w_packed, bias, out_bf16, frames, H, W, st)) return rc;
    } else {
        conv3x3_relu_smallc_kernel<64, false, __bf16><<<conv_grid(npatch, 1), 256, 0, st>>>(
            in, w_packed, bias, reinterpret_cast<__bf16*>(out_bf16), (int)npatch, H, W, cin, cout, ntk_vgg_packed_k(cin));
    }
    NTK_CHECK_LAUNCH("ntk_vgg_conv3x3_relu_f32_to_bf16");
    return NTK_OK;
}

extern "C" int ntk_vgg_conv3x3_relu_bf16(const void* in_bf16, const void* w_packed_bf16, const float* bias, void* out,
                                         int frames, int H, int W, int cin, int cout, int fuse_pool, int out_f32,
                                         void* stream) {
    long npatch;
    if (int rc = conv_check_frames("ntk_vgg_conv3x3_relu_bf16", in_bf16 && w_packed_bf16 && bias && out,
                                   ntk_aligned16(in_bf16) && ntk_aligned16(w_packed_bf16) && ntk_aligned16(out), frames, H, W, npatch))
        return rc;
    NTK_REQUIRE(cin > 0 && (cin % OperandBf16::KT) == 0 && cout > 0 && (cout % 64) == 0, NTK_ERR_BAD_SHAPE,
                "ntk_vgg_conv3x3_relu_bf16: cin=%d must be a multiple of 64, cout=%d a multiple of 64", cin, cout);
    hipStream_t st = (hipStream_t)stream;
    if (out_f32) launch_dma<OperandBf16, float>(in_bf16, w_packed_bf16, bias, out, npatch, H, W, cin, cout, 9 * cin, fuse_pool, st);
    else launch_dma<OperandBf16, __bf16>(in_bf16, w_packed_bf16, bias, out, npatch, H, W, cin, cout, 9 * cin, fuse_pool, st);
    NTK_CHECK_LAUNCH("ntk_vgg_conv3x3_relu_bf16");
    return NTK_OK;
}
