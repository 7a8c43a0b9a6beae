// NTM sequence backward (full BPTT, no truncation -- what tf.gradients through
// the tf.while_loop of LoopNTMTracker computes, direct_offset_output.py:611-621).
// One persistent workgroup per sequence walks the steps in reverse with the
// carried gradients (dM, dw, dread, dh, dc) resident in LDS.  The forward pass
// recorded every tensor the step derivative needs (ntm_seq_fwd.hip), so nothing
// is recomputed except cheap elementwise terms; the next step's records are
// prefetched into registers while the current step computes.
//
// Outputs: per-step raw (pre-activation) gradients of the LSTM gates and of the
// unpack/output linear -- the weight gradients are then three k-major GEMMs over
// all B*S rows (ntk_gemm_tn_f32) -- and the gradient of the initial state.
//
// Gradient semantics: pow: d/dx = y*x^(y-1), d/dy = x^y*log(x)
// with log(x) -> 0 for x <= 0; l2_normalize differentiates through
// rsqrt(max(sum x^2, 1e-12)) (zero through the norm when clamped).
//
// The head / memory / unpack half of a step (phases X1 .. B9, ntm_bwd_heads_step), the record prefetch / commit, the per-head
// reductions and the set-up of the carried dM / dw / dread are in ntm_phases.h, shared with ntm_seq_deep.hip; the step takes this
// kernel's stamped barrier as a callable.  This file's own: the LSTM backward B10, the gate-weight product B11 with its
// wave-specialised form (stream waves, resident rows), the plan and the launcher.  The argument struct, the pointer check, the LDS
// carve-up and the workgroup-size rule are in ntm_seq_args.h, shared with ntm_seq_deep.hip.
#include "ntm_common.h"
#include "ntm_phases.h"
#include <stdlib.h>
#include <type_traits>

// Diagnostic build only (-DNTK_CL_PROF): s_memtime shares between consecutive workgroup barriers of a step (LDS accumulators)
#ifdef NTK_CL_PROF
__device__ unsigned long long g_ntm_bwd_prof[16];
#define NTMB_STAMP(i)                                                       \
    do {                                                                    \
        if (blockIdx.x == 0 && tid == 0) {                                  \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();   \
            s_prof[i] += now_ - s_prof[15];                                 \
            s_prof[15] = now_;                                              \
        }                                                                   \
    } while (0)
extern "C" int ntk_ntm_bwd_prof(unsigned long long* out16) {
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_ntm_bwd_prof), 16 * sizeof(unsigned long long)) == hipSuccess ? NTK_OK : NTK_ERR_HIP;
}
#else
#define NTMB_STAMP(i) do { } while (0)
#endif

// WS (benchmark shape only, 768 threads): the h columns of B11 -- d h_{t-1} = dgates_t . Wr^T[:, 80:280], 71 % of the kernel's
// largest weight stream (42 % of a BPTT step) -- are NOT needed until the LSTM cell backward of the NEXT iteration, ten phases
// later; only the 80 read columns feed the top of the next iteration.  Waves 10, 11 ("stream", 100 of 128 lanes = one float4
// column group x one half of the 800 rows) walk those columns in a circle, one lap per step, through a ring of row registers
// that is never drained, beside the phases of the 640 compute threads, and hand the product over (2 x 200 floats in LDS)
// before the barrier in front of B10.  Both kinds of wave run the same twelve workgroup barriers per step; the stream waves
// consume a fixed number of 4-row groups between consecutive barriers (kBwdWsGroups).  Same idea as ntm_seq_fwd_ws.hip.
constexpr int BWS_RING = 20, BWS_LAP = 400, BWS_NG = BWS_LAP / 4;
// groups consumed before barriers 1 .. 9 of an iteration (X1, X2, R2, R3, R4, the three parts of B7 / B8, B9), then after
// barriers 10 and 11 (beside the read columns of B11 and the carry / commit): 100 in all
constexpr int kBwdWsGroups[11] = {14, 16, 7, 4, 10, 14, 7, 9, 6, 6, 7};
constexpr int bws_sum(int n) { int s = 0; for (int i = 0; i < n; ++i) s += kBwdWsGroups[i]; return s; }
static_assert(bws_sum(11) == BWS_NG && BWS_LAP % BWS_RING == 0, "one lap per step; the ring's phase is static");

// SIM (NTM_SIM_*): the similarity of the content addressing, a compile-time mode as in ntm_seq_fwd.hip.  Smooth cosine
// recomputes sim = k.M_prev[n] / (|k||M_prev[n]| + 1e-3) from the same records and differentiates it through both norms, with
// the gradient of a norm at exactly zero defined as 0 (the pow convention above; autograd yields NaN there).
template <int MAXT, bool FIX, bool WS = false, int SIM = NTM_SIM_AS_CODED>
__global__ __launch_bounds__(MAXT) void ntm_seq_bwd_kernel(NtmBwdArgs a, NtmBwdLds L) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    static_assert(!WS || FIX, "the wave-specialised form exists for the benchmark shape only");
    constexpr bool SMOOTH = SIM == NTM_SIM_SMOOTH_COSINE;
    static_assert(!WS || !SMOOTH, "the wave-specialised form is as coded only");
    const int b = blockIdx.x, tid0 = threadIdx.x, T = FIX ? 640 : blockDim.x;
    const int N = FIX ? 128 : a.d.N, Md = FIX ? 20 : a.d.Md, MP = Md | 1, R = FIX ? 4 : a.d.R, Wh = FIX ? 1 : a.d.Wh;
    const int H = R + Wh, hid = FIX ? 200 : a.d.hid, SS = FIX ? 3 : a.d.SS;
    const int S = a.d.S, RM = R * Md, K = RM + hid, NMd = N * Md, HN = H * N;
    const NtmCtl d = ntm_ctl(Md, R, Wh, hid, SS, FIX ? 2 : a.d.O, FIX ? 0 : a.d.write_first);
    const int PP = d.PP;
    const int ldkT = FIX ? 280 : a.ldkT, ldhT = FIX ? 200 : a.ldhT;
    const NtmBwdSt c = ntm_bwd_state(smem, L, b, S, T, N, Md, R, Wh, hid, SS, PP, ldhT);      // LDS pointers + decomposition of X1 .. B9
    float* const sPart = c.sPart; float* const sdM = c.sdM; float* const sdW = c.sdW; float* const sDG = c.sDG;
    float* const sdZ = c.sdZ; float* const sdC = c.sdC; float* const sGt = c.sGt; float* const sCt = c.sCt; float* const sCp = c.sCp;
    f32x4* sPart4 = reinterpret_cast<f32x4*>(sPart);
    // WS: d h_{t-1} partials of the stream waves, [2 row halves][200] floats, behind the resident rows of Wa^T
    float* sPartH = smem + L.total + 32 + NTMB_RES_WA * 600 * 4;

    if constexpr (WS) {
        if (tid0 >= 640) {
            // =========================================================== stream waves (see the note above the kernel)
            const int sidx = min(tid0 - 640, 99);
            const int cgs = sidx % 50, sls = sidx / 50;              // float4 column group of the h columns, half of the rows
            const __amdgpu_buffer_rsrc_t wrs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a.WrT + 80), 0,
                                                                                  (800 * 280 - 80) * (int)sizeof(float), 0x00020000);
            const unsigned voff = (unsigned)cgs * 16u + (unsigned)sls * (unsigned)(BWS_LAP * 280 * sizeof(float));
            auto wrow = [&](int r) { return __builtin_bit_cast(f32x4, __builtin_amdgcn_raw_buffer_load_b128(wrs, voff, r * (280 * (int)sizeof(float)), 0)); };
            const float* dgp = sDG + BWS_LAP * sls;                  // this half's dgates (written by B10, read after barrier 10)
            constexpr int G0 = kBwdWsGroups[9] + kBwdWsGroups[10];   // groups of a lap consumed in the iteration that starts it
            f32x4 ring[BWS_RING];
#pragma unroll
            for (int q = 0; q < BWS_RING; ++q) ring[(4 * G0 + q) % BWS_RING] = wrow((4 * G0 + q) % BWS_LAP);
            // the first iteration's "product of the step after the last" is the gradient of the final state: dgates are zero
            // there (the compute waves clear them), so the groups it still runs add nothing to this initial value
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            if (sls == 0 && a.dcs_fin) acc = *reinterpret_cast<const f32x4*>(a.dcs_fin + (size_t)b * 2 * hid + hid + 4 * cgs);
            auto group = [&](auto gc) {                              // rows 4 g .. 4 g + 3 of this lane's half
                constexpr int r = 4 * decltype(gc)::value;
                const f32x4 hv = *reinterpret_cast<const f32x4*>(dgp + r);
#pragma unroll
                for (int q = 0; q < 4; ++q) {
                    acc += hv[q] * ring[(r + q) % BWS_RING];
                    ring[(r + q) % BWS_RING] = wrow((r + q + BWS_RING) % BWS_LAP);
                }
                __builtin_amdgcn_sched_barrier(0);                   // keep the groups in program order (ntm_seq_fwd_ws.hip)
            };
            auto finish_lap = [&]() {                                // groups G0 .. 99 with the barriers 1 .. 8 between them, then the hand-over
                constexpr int c0 = G0, c1 = c0 + kBwdWsGroups[0], c2 = c1 + kBwdWsGroups[1], c3 = c2 + kBwdWsGroups[2],
                              c4 = c3 + kBwdWsGroups[3], c5 = c4 + kBwdWsGroups[4], c6 = c5 + kBwdWsGroups[5],
                              c7 = c6 + kBwdWsGroups[6], c8 = c7 + kBwdWsGroups[7];
                static_assert(c8 + kBwdWsGroups[8] == BWS_NG, "lap");
                ntk_static_for<c0, c1>(group); __syncthreads();             // 1
                ntk_static_for<c1, c2>(group); __syncthreads();             // 2
                ntk_static_for<c2, c3>(group); __syncthreads();             // 3
                ntk_static_for<c3, c4>(group); __syncthreads();             // 4
                ntk_static_for<c4, c5>(group); __syncthreads();             // 5
                ntk_static_for<c5, c6>(group); __syncthreads();             // 6
                ntk_static_for<c6, c7>(group); __syncthreads();             // 7
                ntk_static_for<c7, c8>(group); __syncthreads();             // 8
                ntk_static_for<c8, BWS_NG>(group);
                // every lane stores (lanes 100 .. 127 shadow lane 99: same address, same value; see ntm_seq_fwd_ws.hip)
                reinterpret_cast<f32x4*>(sPartH)[sls * 50 + cgs] = acc;
                acc = f32x4{0.f, 0.f, 0.f, 0.f};
            };
            __syncthreads();                                         // initial state, records of the last step committed
            __syncthreads();                                         // resident rows of Wa^T
            for (int t = S - 1; t >= 0; --t) {
                finish_lap();
                __syncthreads();                                     // 9: the partials of d h_t are in LDS
                __syncthreads();                                     // 10: dgates_t are in LDS
                ntk_static_for<0, kBwdWsGroups[9]>(group);
                __syncthreads();                                     // 11
                ntk_static_for<kBwdWsGroups[9], G0>(group);
                __syncthreads();                                     // 12
            }
            finish_lap();                                            // d h_{-1}: the gradient of the initial controller state
            __syncthreads();                                         // (its barriers 1 .. 8 are matched by the compute waves' epilogue)
            return;
        }
    }

    const int kg4 = ldkT >> 2, hg4 = c.hg4;
    const int nslZ = max(1, T / kg4), nperZ = (4 * hid + nslZ - 1) / nslZ;
    const int nslH = c.nslH, nperH = c.nperH;

    // ---- carried gradients start from the (optional) gradient of the final state; the records of the last step
    ntm_bwd_init_carried(c, a, tid0);
    for (int i = RM + tid0; i < ldkT; i += T) sdZ[i] = (i < K && a.dcs_fin) ? a.dcs_fin[(size_t)b * 2 * hid + hid + (i - RM)] : 0.f;
    for (int i = tid0; i < hid; i += T) sdC[i] = a.dcs_fin ? a.dcs_fin[(size_t)b * 2 * hid + i] : 0.f;
    if constexpr (WS) {
        for (int i = tid0; i < 4 * hid; i += T) sDG[i] = 0.f;         // the stream waves' first (partial) lap multiplies these
    }
    NtmBwdRecs rec = {};                                 // prefetch registers for one step's records
    const float* const c_init = a.cs0 + (size_t)b * 2 * hid;
    {
        const NtmBwdWho w = ntm_bwd_who(tid0, N, H);
        ntm_bwd_prefetch(c, d, a, w, rec, S - 1, c_init);
        ntm_bwd_commit(c, d, w, rec);
    }
    __syncthreads();

    // benchmark shape: 7 of the 15 rows of Wa^T a thread multiplies in B9 stay in LDS for the whole sequence (67 KB of the 74 KB
    // the state leaves free); B9's stream runs at ~67 GB/s, the worst of the kernel's three weight streams
    if constexpr (FIX) {
        if (tid0 < nslH * hg4) {
            const int cg = tid0 % hg4, sl = tid0 / hg4;
            const int c0 = sl * nperH, c1 = min(PP, c0 + nperH);
            f32x4* wl = reinterpret_cast<f32x4*>(smem + L.total + 32);
            for (int q = 0; q < NTMB_RES_WA; ++q)
                wl[q * (nslH * hg4) + tid0] = (c0 + q < c1) ? reinterpret_cast<const f32x4*>(a.WaT)[(size_t)(c0 + q) * hg4 + cg] : f32x4{0.f, 0.f, 0.f, 0.f};
        }
        __syncthreads();
    }
    // WS: the first NTMB_RES_B11 rows of every compute thread's 25-row slice of B11's read columns stay in registers for the whole
    // launch (the kernel has 146 of the 168 registers twelve waves allow): 51 of the 256 KB that product draws from L2 per step
    constexpr int NTMB_RES_B11 = 5;
    f32x4 wres11[NTMB_RES_B11];
    if constexpr (WS) {
        const int cg = tid0 % 20, sl = tid0 / 20;
#pragma unroll
        for (int q = 0; q < NTMB_RES_B11; ++q) wres11[q] = reinterpret_cast<const f32x4*>(a.WrT)[(size_t)(sl * 25 + q) * kg4 + cg];
    }
#ifdef NTK_CL_PROF
    unsigned long long* s_prof = reinterpret_cast<unsigned long long*>(smem + L.total);      // 128 B behind the state (the launch adds them)
    if (threadIdx.x == 0) { for (int i = 0; i < 15; ++i) s_prof[i] = 0; s_prof[15] = __builtin_amdgcn_s_memtime(); }
#endif
    for (int t = S - 1; t >= 0; --t) {
        // opaque thread id: keeps loop-invariant index/address expressions from being hoisted out of the
        // t-loop (they would be spilled to scratch and reloaded every step)
        int tid_op = tid0;
        asm volatile("" : "+v"(tid_op));
        const NtmBwdWho w = ntm_bwd_who(tid_op, N, H);
        const int tid = w.tid;
        const size_t bt = (size_t)b * S + t;
        if (t > 0) ntm_bwd_prefetch(c, d, a, w, rec, t - 1, c_init);

        // ------------------------------------------------ X1 .. B9 (ntm_phases.h): heads, memory, unpack; nine barriers, stamps 0 .. 8
        ntm_bwd_heads_step<MAXT, FIX, SMOOTH>(c, d, a, w, bt, [&](int i) { __syncthreads(); NTMB_STAMP(i); }, [&](int i) { NTMB_STAMP(i); });
        // ------------------------------------------------ B10: LSTM cell backward
        if (tid < hid) {
            float dh = WS ? sPartH[tid] + sPartH[hid + tid] : sdZ[RM + tid];
            for (int sl = 0; sl < nslH; ++sl) dh += sPart[sl * ldhT + tid];
            const f32x4 g = reinterpret_cast<const f32x4*>(sGt)[tid];
            const float gi = g[0], gj = g[1], gf = g[2], go = g[3];
            const float tc = tanhf(sCt[tid]);
            const float dct = sdC[tid] + dh * go * (1.0f - tc * tc);
            f32x4 dg;
            dg[0] = dct * gj * gi * (1.0f - gi);
            dg[1] = dct * gi * (1.0f - gj * gj);
            dg[2] = dct * sCp[tid] * gf * (1.0f - gf);
            dg[3] = dh * tc * go * (1.0f - go);
            sdC[tid] = dct * gf;
            reinterpret_cast<f32x4*>(sDG)[tid] = dg;
            reinterpret_cast<f32x4*>(a.dgates)[bt * hid + tid] = dg;
        }
        __syncthreads();
        NTMB_STAMP(9);
        // ------------------------------------------------ B11: d[read_prev; h_prev] = dgates . Wr^T
        if constexpr (WS) {
            // the 80 read columns only (20 float4 column groups x 32 row slices of 25): the h columns are the stream waves'
            const int cg = tid % 20, sl = tid / 20;
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int q = 0; q < NTMB_RES_B11; ++q) acc += sDG[sl * 25 + q] * wres11[q];       // (same order of the 25 rows as before)
            sPart4[sl * 20 + cg] = ntk_stream_matvec_exact<4>(reinterpret_cast<const f32x4*>(a.WrT) + cg, kg4, sDG, sl * 25 + NTMB_RES_B11, sl * 25 + 25, acc);
        } else if (tid < nslZ * kg4) {
            const int cg = tid % kg4, sl = tid / kg4;
            const int r0 = sl * nperZ, r1 = min(4 * hid, r0 + nperZ);
            sPart4[sl * kg4 + cg] = ntk_stream_matvec<(MAXT > 768 ? 2 : 8)>(reinterpret_cast<const f32x4*>(a.WrT) + cg, kg4, sDG, r0, r1, 4 * hid - 1);
        }
        __syncthreads();
        NTMB_STAMP(10);
        if constexpr (WS) {
            if (tid < RM) {
                float s = 0.f;
#pragma unroll 8
                for (int sl = 0; sl < 32; ++sl) s += sPart[sl * RM + tid];
                sdZ[tid] = s;
            }
        } else if (tid < K) {
            float s = 0.f;
            for (int sl = 0; sl < nslZ; ++sl) s += sPart[sl * ldkT + tid];
            sdZ[tid] = s;
        }
        if (t > 0) ntm_bwd_commit(c, d, w, rec);       // next (earlier) step's records: every reader of the old ones has passed a barrier
        __syncthreads();
        NTMB_STAMP(11);
    }

#ifdef NTK_CL_PROF
    if (blockIdx.x == 0 && threadIdx.x == 0) for (int i = 0; i < 16; ++i) g_ntm_bwd_prof[i] = s_prof[i];
#endif
    // ---- gradient of the initial state
    for (int i = tid0; i < NMd; i += T) a.dM0[(size_t)b * NMd + i] = sdM[(i / Md) * MP + (i % Md)];
    for (int i = tid0; i < HN; i += T) a.dw0[(size_t)b * HN + i] = sdW[i];
    for (int i = tid0; i < RM; i += T) a.dread0[(size_t)b * RM + i] = sdZ[i];
    if constexpr (WS) {
        // the stream waves finish the last lap (d h_{-1}) behind eight more barriers and one for the hand-over
#pragma unroll
        for (int i = 0; i < 9; ++i) __syncthreads();
    }
    for (int i = tid0; i < hid; i += T) {
        a.dcs0[(size_t)b * 2 * hid + i] = sdC[i];
        a.dcs0[(size_t)b * 2 * hid + hid + i] = WS ? sPartH[i] + sPartH[hid + i] : sdZ[RM + i];
    }
}

// [rows][cols] -> [cols][ldo] (zero padded), used for WrT / WaT once per optimiser step
__global__ void transpose_pad_kernel(const float* __restrict__ in, int ldi, float* __restrict__ out, int ldo,
                                     int rows, int cols) {
    __shared__ float tile[32][33];
    const int c0 = blockIdx.x * 32, r0 = blockIdx.y * 32;
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        const int r = r0 + i, c = c0 + threadIdx.x;
        tile[i][threadIdx.x] = (r < rows && c < cols) ? in[(size_t)r * ldi + c] : 0.f;
    }
    __syncthreads();
    for (int i = threadIdx.y; i < 32; i += blockDim.y) {
        const int c = c0 + i, r = r0 + threadIdx.x;
        if (c < cols && r < ldo) out[(size_t)c * ldo + r] = (r < rows) ? tile[threadIdx.x][i] : 0.f;
    }
}

extern "C" int ntk_transpose_pad(const float* in, int ldi, float* out, int ldo, int rows, int cols, void* stream) {
    NTK_REQUIRE(in && out, NTK_ERR_BAD_PTR, "ntk_transpose_pad: null pointer");
    NTK_REQUIRE(rows > 0 && cols > 0 && ldi >= cols && ldo >= rows, NTK_ERR_BAD_SHAPE,
                "ntk_transpose_pad: rows=%d cols=%d ldi=%d ldo=%d", rows, cols, ldi, ldo);
    dim3 grid((cols + 31) / 32, (ldo + 31) / 32), block(32, 8);
    transpose_pad_kernel<<<grid, block, 0, (hipStream_t)stream>>>(in, ldi, out, ldo, rows, cols);
    NTK_CHECK_LAUNCH("ntk_transpose_pad");
    return NTK_OK;
}

// every limit of the BPTT kernels and the kernel a shape takes, host arithmetic only
static int ntm_bwd_plan(const NtmDims& d, int ldkT, int ldhT, NtmBwdPlan& p, const char* who) {
    int rc = ntm_validate_dims(d, who);
    if (rc != NTK_OK) return rc;
    NTK_REQUIRE((d.hid % 4) == 0, NTK_ERR_UNSUPPORTED, "%s: hidden=%d must be a multiple of 4", who, d.hid);
    NTK_REQUIRE(ldkT >= d.K && (ldkT % 4) == 0 && ldhT >= d.hid && (ldhT % 4) == 0, NTK_ERR_BAD_SHAPE,
                "%s: ldkT=%d (K=%d) ldhT=%d (hid=%d)", who, ldkT, d.K, ldhT, d.hid);
    NTK_REQUIRE(d.SS + 1 <= NQ, NTK_ERR_UNSUPPORTED, "%s: shift_range=%d too wide", who, (d.SS - 1) / 2);
    // a thread prefetches at most MAXM elements of the memory: a wide memory under few heads (64 x 72 under two) takes the threads
    // it needs for that, where it was refused (this kernel's own clause; the deep BPTT refuses such a memory)
    const int T = ntm_bwd_threads(d, (d.N * d.Md + MAXM - 1) / MAXM);
    NTK_REQUIRE(T <= 1024 && d.H * d.N <= 1024 && d.N * d.Md <= MAXM * T, NTK_ERR_UNSUPPORTED,
                "%s: heads*mem_size=%d (max 1024) / mem_size*mem_dim=%d (max %d per thread of %d) / hidden=%d (3*hidden <= 1024) exceed "
                "one workgroup", who, d.H * d.N, d.N * d.Md, MAXM, T, d.hid);
    // this kernel's own users of `part`: the partials of B11 over the ldkT columns of Wr^T and, in the wave-specialised form, its read
    // columns in 32 row slices; the carried dZ is one step input wide (ldkT), dC one layer's cells
    ntm_bwd_lds(d, T, ldhT, ntm_imax(ntm_bwd_part_floats(T, ldkT), 32 * d.R * d.Md), ldkT, d.hid, p.L);
    const bool fix = (d.N == 128 && d.Md == 20 && d.R == 4 && d.Wh == 1 && d.hid == 200 && d.SS == 3 && d.O == 2 &&
                      T == 640 && !d.write_first && ldkT == 280 && ldhT == 200);
    p.lds_bytes = (size_t)p.L.total * sizeof(float) + 128;                // + the diagnostic build's stamp words
    if (fix) p.lds_bytes += (size_t)NTMB_RES_WA * (T / (ldhT / 4)) * (ldhT / 4) * sizeof(f32x4);     // resident rows of Wa^T
    // benchmark shape: the form whose h columns of Wr^T stream beside the step (NTK_NTM_BWD_FORM=res: round 2's kernel, for comparison)
    const char* form_env = getenv("NTK_NTM_BWD_FORM");               // read per call (development switch)
    const bool ws = fix && d.similarity == NTM_SIM_AS_CODED && !(form_env && form_env[0] == 'r');     // (no wave-specialised smooth-cosine form)
    if (ws) p.lds_bytes += (size_t)2 * d.hid * sizeof(float);
    NTK_REQUIRE(p.lds_bytes <= 160 * 1024, NTK_ERR_UNSUPPORTED, "%s: needs %zu B of LDS (> 160 KiB)", who, p.lds_bytes);
    p.kernel = ws ? NTK_NTM_BWD_WS : fix ? NTK_NTM_BWD_FIX : T <= 768 ? NTK_NTM_BWD_GENERIC768 : NTK_NTM_BWD_GENERIC1024;
    p.T = T;
    p.threads = ws ? 768 : T;
    return NTK_OK;
}

extern "C" int ntk_ntm_seq_plan_sim(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int write_first,
                                    int similarity,
                                    int ldkT, int ldhT, int* fwd_kernel, int* fwd_threads, int* bwd_kernel, int* bwd_threads) {
    NTM_REQUIRE_SIMILARITY(similarity, "ntk_ntm_seq_plan");
    const NtmDims d = ntm_dims(B, 1, N, Md, R, Wh, hid, shift_range, O, write_first, similarity);
    if (ldkT <= 0) ldkT = ntm_align4(d.K);
    if (ldhT <= 0) ldhT = ntm_align4(hid);
    NtmBwdPlan pb;
    NtmFwdPlan pf;
    // the BPTT first: where both refuse, ntk_last_error() keeps the forward's reason
    const bool bwd = ntm_bwd_plan(d, ldkT, ldhT, pb, "ntk_ntm_seq_bwd") == NTK_OK;
    const bool fwd = ntm_fwd_plan(d, pf, "ntk_ntm_seq_fwd") == NTK_OK;
    if (fwd_kernel) *fwd_kernel = fwd ? pf.kernel : 0;
    if (fwd_threads) *fwd_threads = fwd ? pf.T : 0;
    if (bwd_kernel) *bwd_kernel = bwd ? pb.kernel : 0;
    if (bwd_threads) *bwd_threads = bwd ? pb.threads : 0;
    return (fwd ? NTK_NTM_PLAN_FWD : 0) | (bwd ? NTK_NTM_PLAN_BWD : 0);
}

extern "C" int ntk_ntm_seq_plan(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int write_first,
                                int ldkT, int ldhT, int* fwd_kernel, int* fwd_threads, int* bwd_kernel, int* bwd_threads) {
    return ntk_ntm_seq_plan_sim(B, N, Md, R, Wh, hid, shift_range, O, write_first, NTM_SIM_AS_CODED, ldkT, ldhT, fwd_kernel, fwd_threads,
                                bwd_kernel, bwd_threads);
}

// ntk_ntm_seq_bwd behind its plain, *_sim and step entries: similarity, then shape and plan, then pointers, then the launch
int ntm_seq_bwd_run(const NtmBwdArgs& a, void* stream) {
    const char* who = "ntk_ntm_seq_bwd";
    NTM_REQUIRE_SIMILARITY(a.d.similarity, who);
    NtmBwdPlan p;
    int rc = ntm_bwd_plan(a.d, a.ldkT, a.ldhT, p, who);
    if (rc != NTK_OK) return rc;
    rc = ntm_bwd_check_ptrs(a, who);
    if (rc != NTK_OK) return rc;
    typedef void (*kern_t)(NtmBwdArgs, NtmBwdLds);
    constexpr int AC = NTM_SIM_AS_CODED, SC = NTM_SIM_SMOOTH_COSINE;
    static const NtmKernelRow<kern_t> rows[] = {
        {NTK_NTM_BWD_WS, AC, ntm_seq_bwd_kernel<768, true, true>},           // (as coded only)
        {NTK_NTM_BWD_FIX, AC, ntm_seq_bwd_kernel<768, true>},                {NTK_NTM_BWD_FIX, SC, ntm_seq_bwd_kernel<768, true, false, SC>},
        {NTK_NTM_BWD_GENERIC768, AC, ntm_seq_bwd_kernel<768, false>},        {NTK_NTM_BWD_GENERIC768, SC, ntm_seq_bwd_kernel<768, false, false, SC>},
        {NTK_NTM_BWD_GENERIC1024, AC, ntm_seq_bwd_kernel<1024, false>},      {NTK_NTM_BWD_GENERIC1024, SC, ntm_seq_bwd_kernel<1024, false, false, SC>}};
    static NtkLdsAttrCache lds_cache;
    kern_t fn;
    rc = ntm_find_kernel(lds_cache, rows, p.kernel, a.d.similarity, who, fn);
    if (rc != NTK_OK) return rc;
    fn<<<a.d.B, p.threads, p.lds_bytes, (hipStream_t)stream>>>(a, p.L);
    NTK_CHECK_LAUNCH(who);
    return NTK_OK;
}

extern "C" int ntk_ntm_seq_bwd_sim(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O,
                               int write_first, int similarity,
                               const float* WrT, int ldkT, const float* WaT, int ldhT,
                               const float* M0, const float* w0, const float* cs0,
                               const float* st_gates, const float* st_c, const float* st_u,
                               const float* st_wc, const float* st_wv, const float* st_w, const float* st_M,
                               const float* dlogits,
                               const float* dM_fin, const float* dw_fin, const float* dread_fin, const float* dcs_fin,
                               float* dgates, float* du, float* dM0, float* dw0, float* dread0, float* dcs0,
                               void* stream) {
    return ntm_seq_bwd_run({ntm_dims(B, S, N, Md, R, Wh, hid, shift_range, O, write_first, similarity), WrT, WaT, ldkT, ldhT, M0, w0, cs0,
                            st_gates, st_c, st_u, st_wc, st_wv, st_w, st_M, dlogits, dM_fin, dw_fin, dread_fin, dcs_fin,
                            dgates, du, dM0, dw0, dread0, dcs0}, stream);
}

extern "C" int ntk_ntm_seq_bwd(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O,
                               int write_first,
                               const float* WrT, int ldkT, const float* WaT, int ldhT,
                               const float* M0, const float* w0, const float* cs0,
                               const float* st_gates, const float* st_c, const float* st_u,
                               const float* st_wc, const float* st_wv, const float* st_w, const float* st_M,
                               const float* dlogits,
                               const float* dM_fin, const float* dw_fin, const float* dread_fin, const float* dcs_fin,
                               float* dgates, float* du, float* dM0, float* dw0, float* dread0, float* dcs0,
                               void* stream) {
    return ntm_seq_bwd_run({ntm_dims(B, S, N, Md, R, Wh, hid, shift_range, O, write_first, NTM_SIM_AS_CODED), WrT, WaT, ldkT, ldhT, M0, w0,
                            cs0, st_gates, st_c, st_u, st_wc, st_wv, st_w, st_M, dlogits, dM_fin, dw_fin, dread_fin, dcs_fin,
                            dgates, du, dM0, dw0, dread0, dcs0}, stream);
}

