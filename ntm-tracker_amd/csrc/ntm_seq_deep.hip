// NTM sequence kernels for a deep controller: a MultiRNNCell of L >= 2 BasicLSTMCell layers (ntm_cell.py:45-50, :101-105)
// inside the persistent forward and BPTT walks of ntm_seq_fwd.hip / ntm_seq_bwd.hip (their generic, runtime-dimension forms).
// One workgroup per sequence; every layer's c and h stay resident in LDS beside M, w and the reads.
//
//   layer 0      reads [x_t ; read_{t-1}] and h_0(t-1)   (the x part is hoisted: one GEMM over all B*S rows)
//   layer k >= 1 reads h_{k-1}(t) and h_k(t-1)
//   h_{L-1}(t) drives the unpack / output linear; addressing, memory update and read are those of the single-layer kernels.
//
// LDS holds z = [read (R*Md) | h_0 | h_1 | ... | h_{L-1}] (hid each), so layer 0's recurrent input is z[0 .. R*Md+hid) and
// layer k's is z[R*Md+(k-1)*hid .. R*Md+(k+1)*hid): updating h_k in place, layer by layer, hands layer k+1 the new h_k and
// its own old h_{k+1}.  The BPTT keeps the carried gradients in the same layout.
//
// Shared with the single-layer kernels (ntm_phases.h): the control layout, P2's memory normaliser and P3 .. P8 of the forward step,
// X1 .. B9 of the BPTT step with its record prefetch / commit, per-head reductions and carried-gradient set-up; (ntm_seq_args.h): the
// argument structs (NtmDeepFwdArgs, NtmDeepBwdArgs), the pointer checks, both LDS carve-ups and the workgroup-size rules.  This
// file's own: the layer loops (P1 / P2 per layer forward, B10 / B11 per layer in the BPTT), the records of the lower layers, the
// pack kernel of the weight layouts, the plan and the launchers.
#include "ntm_phases.h"

// ------------------------------------------------------------------------------------------------ packed layouts
// (Wx0 / Wf / Wb and NtmDeepShape: ntm_seq_args.h)
static inline __host__ __device__ size_t ntm_deep_nwx0(const NtmDeepShape& s) { return (size_t)4 * s.hid * s.ldx; }
static inline __host__ __device__ size_t ntm_deep_nwf(const NtmDeepShape& s) { return (size_t)4 * s.hid * (s.rf0 + (size_t)(s.L - 1) * s.rf1); }
static inline __host__ __device__ size_t ntm_deep_nwb(const NtmDeepShape& s) { return (size_t)4 * s.hid * (s.cb0 + (size_t)(s.L - 1) * s.cb1); }

// element (row k, column n') of forward block l, read from the stacked cell's own layout
__device__ __forceinline__ float ntm_deep_wf(const NtmDeepShape& s, const float* lowerT, const float* topWxT, const float* topWr,
                                             int l, int k, int n) {
    const int hid = s.hid, j = n >> 2, g = n & 3, rtf = g * hid + j;     // TF row of the lower matrices
    if (l == 0) return (k <= s.RM + hid) ? lowerT[(size_t)rtf * s.ld0 + s.D + k] : 0.f;
    if (l < s.L - 1) {
        const float* W = lowerT + (size_t)4 * hid * s.ld0 + (size_t)(l - 1) * 4 * hid * s.ld1;
        return (k <= 2 * hid) ? W[(size_t)rtf * s.ld1 + k] : 0.f;
    }
    if (k < hid) return topWxT[(size_t)n * s.ldxt + k];
    if (k <= 2 * hid) return topWr[(size_t)(s.RM + k - hid) * 4 * hid + n];      // h rows, then the bias row RM + hid
    return 0.f;
}

__global__ void ntm_deep_pack_kernel(NtmDeepShape s, const float* __restrict__ lowerT, const float* __restrict__ topWxT,
                                     const float* __restrict__ topWr, float* __restrict__ Wx0, float* __restrict__ Wf,
                                     float* __restrict__ Wb) {
    const int hid = s.hid, G = 4 * hid;
    const size_t nx = ntm_deep_nwx0(s), nf = ntm_deep_nwf(s), nb = ntm_deep_nwb(s);
    for (size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x; i < nx + nf + nb; i += (size_t)gridDim.x * blockDim.x) {
        if (i < nx) {
            const int n = (int)(i / s.ldx), c = (int)(i % s.ldx), j = n >> 2, g = n & 3;
            Wx0[i] = (c < s.D) ? lowerT[(size_t)(g * hid + j) * s.ld0 + c] : 0.f;
        } else if (i < nx + nf) {
            const size_t e = i - nx, row = e / G;
            const int n = (int)(e % G);
            const int l = (row < (size_t)s.rf0) ? 0 : 1 + (int)((row - s.rf0) / s.rf1);
            const int k = (l == 0) ? (int)row : (int)((row - s.rf0) % s.rf1);
            Wf[e] = ntm_deep_wf(s, lowerT, topWxT, topWr, l, k, n);
        } else {
            const size_t e = i - nx - nf, b0 = (size_t)G * s.cb0;
            int l, n, c;
            if (e < b0) {
                l = 0; n = (int)(e / s.cb0); c = (int)(e % s.cb0);
            } else {
                const size_t e1 = e - b0, blk = (size_t)G * s.cb1;
                l = 1 + (int)(e1 / blk); n = (int)((e1 % blk) / s.cb1); c = (int)(e1 % s.cb1);
            }
            const int Kl = (l == 0) ? s.RM + hid : 2 * hid;
            Wb[e] = (c < Kl) ? ntm_deep_wf(s, lowerT, topWxT, topWr, l, c, n) : 0.f;
        }
    }
}

// ------------------------------------------------------------------------------------------------ forward
template <int MAXT, int SIM = NTM_SIM_AS_CODED>             // SIM: the similarity of the content addressing, as ntm_seq_fwd.hip
__global__ __launch_bounds__(MAXT) void ntm_seq_fwd_deep_kernel(NtmFwdArgs a, NtmDeepFwdArgs dp, NtmLds L) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr bool SMOOTH = SIM == NTM_SIM_SMOOTH_COSINE;
    const int b = blockIdx.x, tid0 = threadIdx.x, T = blockDim.x;
    const int N = a.d.N, Md = a.d.Md, MP = Md | 1, R = a.d.R, Wh = a.d.Wh;
    const int H = R + Wh, hid = a.d.hid, SS = a.d.SS, NL = dp.s.L;
    const int S = a.d.S, RM = R * Md, K = RM + hid;
    const size_t BS = (size_t)a.d.B * S;
    const NtmCtl d = ntm_ctl(Md, R, Wh, hid, SS, a.d.O, a.d.write_first);
    const int PP = d.PP;
    const NtmDeepShape& sh = dp.s;
    const NtmFwdSt c = ntm_fwd_state(smem, L, T, N, Md, R, Wh, hid, SS, PP, RM + (NL - 1) * hid);
    float* const sPart = c.sPart; float* const sM = c.sM; float* const sW = c.sW;
    float* const sZ = c.sZ;                 // [read | h_0 | .. | h_{L-1}]
    float* const sC = smem + L.C;           // [c_0 | .. | c_{L-1}]
    float* sHtop = sZ + RM + (NL - 1) * hid;

    const int nsl = max(1, T / hid);        // K-slices of the gate products
    const int cs_ld = 2 * hid * NL;

    for (int i = tid0; i < N * Md; i += T) sM[(i / Md) * MP + (i % Md)] = a.M0[(size_t)b * N * Md + i];
    for (int i = tid0; i < H * N; i += T) sW[i] = a.w0[(size_t)b * H * N + i];
    for (int i = tid0; i < RM; i += T) sZ[i] = a.read0[(size_t)b * RM + i];
    for (int i = tid0; i < NL * hid; i += T) {
        const int l = i / hid, j = i - l * hid;
        sC[i] = dp.cs0[(size_t)b * cs_ld + 2 * hid * l + j];
        sZ[RM + i] = dp.cs0[(size_t)b * cs_ld + 2 * hid * l + hid + j];
    }
    __syncthreads();

    const f32x4* Wf4 = reinterpret_cast<const f32x4*>(dp.Wf);
    const f32x4* Wa4 = reinterpret_cast<const f32x4*>(a.Wa);
    f32x4* sPart4 = reinterpret_cast<f32x4*>(sPart);

    for (int t = 0; t < S; ++t) {
        int tid_op = tid0;                  // opaque thread id (see ntm_seq_fwd.hip)
        asm volatile("" : "+v"(tid_op));
        const int tid = tid_op;
        const int lane = tid & 63;
        const int wave = tid >> 6;
        const size_t bt = (size_t)b * S + t;
        // ------------------------------------------------------------ P1 / P2 of ntm_seq_fwd.hip, once per layer
        for (int l = 0; l < NL; ++l) {
            const int Kl = (l == 0) ? K : 2 * hid;
            const int rows = (l == 0) ? sh.rf0 : sh.rf1;
            const float* zin = sZ + ((l == 0) ? 0 : RM + (l - 1) * hid);
            const f32x4* Wl4 = Wf4 + (size_t)((l == 0) ? 0 : sh.rf0 + (l - 1) * sh.rf1) * hid;
            f32x4 xg = {0.f, 0.f, 0.f, 0.f};
            if (tid < hid) {                // bias row (+ this step's input projection at layer 0)
                xg = Wl4[(size_t)Kl * hid + tid];
                if (l == 0) xg += reinterpret_cast<const f32x4*>(a.xproj)[bt * hid + tid];
            }
            if (l < NL - 1) {
                if (l == 0 && dp.st_buf0) {
                    for (int i = tid; i < sh.ld0; i += T)
                        dp.st_buf0[bt * sh.ld0 + i] = (i < sh.D) ? dp.X[bt * sh.ldx + i] : (i < sh.D + K) ? sZ[i - sh.D] : (i == sh.D + K ? 1.f : 0.f);
                } else if (l > 0 && dp.st_bufk) {
                    float* rb = dp.st_bufk + ((size_t)(l - 1) * BS + bt) * sh.ld1;
                    for (int i = tid; i < sh.ld1; i += T) rb[i] = (i < 2 * hid) ? zin[i] : (i == 2 * hid ? 1.f : 0.f);
                }
            } else {
                if (a.st_z) {               // the top layer's record in the single-layer layout (its read rows are unused)
                    for (int i = tid; i < d.ldz; i += T)
                        a.st_z[bt * d.ldz + i] = (i < RM) ? sZ[i] : (i < K ? sHtop[i - RM] : (i == K ? 1.f : 0.f));
                }
                if (dp.st_xtop) {
                    for (int i = tid; i < sh.ldxt; i += T) dp.st_xtop[bt * sh.ldxt + i] = (i < hid) ? zin[i] : 0.f;
                }
            }
            if (tid < nsl * hid) {
                const int j = tid % hid, ks = tid / hid;
                const int kper = (Kl + nsl - 1) / nsl;
                const int k0 = ks * kper, k1 = min(Kl, k0 + kper);
                sPart4[ks * hid + j] = ntk_stream_matvec<(MAXT > 768 ? 2 : 4)>(Wl4 + j, hid, zin, k0, k1, rows - 1);
            }
            __syncthreads();
            if (tid < hid) {
                f32x4 g = xg;
                for (int ks = 0; ks < nsl; ++ks) g += sPart4[ks * hid + tid];
                const float gi = ntm_sigmoid(g[0]);
                const float gj = ntm_tanh(g[1]);
                const float gf = ntm_sigmoid(g[2]);      // forget_bias = 0.0 (ntm_cell.py:47)
                const float go = ntm_sigmoid(g[3]);
                const float c2 = sC[l * hid + tid] * gf + gi * gj;
                const float h2 = ntm_tanh(c2) * go;
                sC[l * hid + tid] = c2;
                sZ[RM + l * hid + tid] = h2;
                const f32x4 ga = {gi, gj, gf, go};
                if (l < NL - 1) {
                    if (dp.st_lgates) reinterpret_cast<f32x4*>(dp.st_lgates)[((size_t)l * BS + bt) * hid + tid] = ga;
                    if (dp.st_lc) dp.st_lc[((size_t)l * BS + bt) * hid + tid] = c2;
                } else {
                    if (a.st_gates) {
                        reinterpret_cast<f32x4*>(a.st_gates)[bt * hid + tid] = ga;
                        a.st_c[bt * hid + tid] = c2;
                    }
                    if (a.st_h) a.st_h[bt * d.ldh + tid] = h2;
                }
            } else if (l == NL - 1 && a.st_h && tid < d.ldh) {
                a.st_h[bt * d.ldh + tid] = (tid == hid) ? 1.f : 0.f;
            }
            if (l == NL - 1) ntm_fwd_mem_norms<SMOOTH>(c, tid);      // the waves not running the top LSTM
            __syncthreads();
        }
        // ------------------------------------------------------------ P3 .. P8 of ntm_seq_fwd.hip on h_{L-1} (ntm_phases.h)
        ntm_fwd_unpack_partials<(MAXT > 768 ? 2 : 4)>(c, d, Wa4, tid);
        __syncthreads();
        ntm_fwd_controls(c, d, a, tid, bt);
        __syncthreads();
        if (wave < H) ntm_fwd_head_wave<SMOOTH, NTM_MAX_SHIFT_TAPS>(c, d, a, wave, lane, bt);
        else if (wave == H && lane == 0 && a.outputs) ntm_fwd_output_softmax(c, d, a, bt);
        __syncthreads();
        if (d.write_first) { ntm_fwd_update_M(c, d, a, tid, bt); __syncthreads(); }
        ntm_fwd_read_partials(c, tid);
        __syncthreads();
        if (!d.write_first) ntm_fwd_update_M(c, d, a, tid, bt);
        ntm_fwd_read_finish(c, a, tid, bt);
        __syncthreads();
    }

    for (int i = tid0; i < N * Md; i += T) a.M_out[(size_t)b * N * Md + i] = sM[(i / Md) * MP + (i % Md)];
    for (int i = tid0; i < H * N; i += T) a.w_out[(size_t)b * H * N + i] = sW[i];
    for (int i = tid0; i < RM; i += T) a.read_out[(size_t)b * RM + i] = sZ[i];
    for (int i = tid0; i < NL * hid; i += T) {
        const int l = i / hid, j = i - l * hid;
        dp.cs_out[(size_t)b * cs_ld + 2 * hid * l + j] = sC[i];
        dp.cs_out[(size_t)b * cs_ld + 2 * hid * l + hid + j] = sZ[RM + i];
    }
}

// ------------------------------------------------------------------------------------------------ BPTT
// Phases X1 .. B9 (heads, memory, unpack) are ntm_bwd_heads_step of ntm_phases.h in its generic form; then the LSTM backward once
// per layer, top first: B10 (cell backward; the top layer adds dU . Wa^T to its carried dh) and B11 (d[input ; h_prev] = dpre . W^T,
// streamed).  Layer k's input gradient is added to the carried dh_{k-1} (which layer k-1 consumes next), its h_prev part replaces
// the carried dh_k; layer 0's splits into the carried dread and dh_0.  Fixed summation order, no atomics: bitwise reproducible.
template <int MAXT, int SIM = NTM_SIM_AS_CODED>             // SIM: as ntm_seq_bwd.hip
__global__ __launch_bounds__(MAXT) void ntm_seq_bwd_deep_kernel(NtmDeepBwdArgs a, NtmBwdLds L) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr bool SMOOTH = SIM == NTM_SIM_SMOOTH_COSINE;
    const int b = blockIdx.x, tid0 = threadIdx.x, T = blockDim.x;
    const int N = a.d.N, Md = a.d.Md, MP = Md | 1, R = a.d.R, Wh = a.d.Wh;
    const int H = R + Wh, hid = a.d.hid, SS = a.d.SS, NL = a.s.L;
    const int S = a.d.S, RM = R * Md, NMd = N * Md, HN = H * N;
    const size_t BS = (size_t)a.d.B * S;
    const NtmCtl d = ntm_ctl(Md, R, Wh, hid, SS, a.d.O, a.d.write_first);
    const int PP = d.PP;
    const int ldhT = a.ldhT, cs_ld = 2 * hid * NL;
    const NtmBwdSt c = ntm_bwd_state(smem, L, b, S, T, N, Md, R, Wh, hid, SS, PP, ldhT);
    float* const sPart = c.sPart; float* const sdM = c.sdM; float* const sdW = c.sdW; float* const sDG = c.sDG;
    float* const sdZ = c.sdZ;  // carried [dread | dh_0 | .. | dh_{L-1}]
    float* const sdC = c.sdC;  // carried [dc_0 | .. | dc_{L-1}]
    float* const sGt = c.sGt; float* const sCt = c.sCt; float* const sCp = c.sCp;
    f32x4* sPart4 = reinterpret_cast<f32x4*>(sPart);
    const f32x4* Wb4 = reinterpret_cast<const f32x4*>(a.Wb);
    const int nslH = c.nslH;

    // ---- carried gradients start from the (optional) gradient of the final state; the records of the last step
    ntm_bwd_init_carried(c, a, tid0);
    for (int i = tid0; i < NL * hid; i += T) {
        const int l = i / hid, j = i - l * hid;
        sdZ[RM + i] = a.dcs_fin ? a.dcs_fin[(size_t)b * cs_ld + 2 * hid * l + hid + j] : 0.f;
        sdC[i] = a.dcs_fin ? a.dcs_fin[(size_t)b * cs_ld + 2 * hid * l + j] : 0.f;
    }
    NtmBwdRecs rec = {};                                 // prefetch registers for one step's records (the top layer's and the heads')
    const float* const c_init = a.cs0 + (size_t)b * cs_ld + 2 * hid * (NL - 1);
    {
        const NtmBwdWho w = ntm_bwd_who(tid0, N, H);
        ntm_bwd_prefetch(c, d, a, w, rec, S - 1, c_init);
        ntm_bwd_commit(c, d, w, rec);
    }
    __syncthreads();

    for (int t = S - 1; t >= 0; --t) {
        int tid_op = tid0;                  // opaque thread id (see ntm_seq_bwd.hip)
        asm volatile("" : "+v"(tid_op));
        const NtmBwdWho w = ntm_bwd_who(tid_op, N, H);
        const int tid = w.tid;
        const size_t bt = (size_t)b * S + t;
        if (t > 0) ntm_bwd_prefetch(c, d, a, w, rec, t - 1, c_init);

        // ------------------------------------------------ X1 .. B9 (the B9 partials are left for the top layer's B10)
        ntm_bwd_heads_step<MAXT, false, SMOOTH>(c, d, a, w, bt, [](int) { __syncthreads(); }, [](int) {});

        // ------------------------------------------------ B10 / B11 once per layer, top first
        for (int l = NL - 1; l >= 0; --l) {
            if (tid < hid) {       // B10: LSTM cell backward
                float dh = sdZ[RM + l * hid + tid];
                f32x4 g;
                float ct, cp;
                if (l == NL - 1) {
                    for (int sl = 0; sl < nslH; ++sl) dh += sPart[sl * ldhT + tid];
                    g = reinterpret_cast<const f32x4*>(sGt)[tid]; ct = sCt[tid]; cp = sCp[tid];
                } else {
                    const size_t r = (size_t)l * BS + bt;
                    g = reinterpret_cast<const f32x4*>(a.st_lgates)[r * hid + tid];
                    ct = a.st_lc[r * hid + tid];
                    cp = (t > 0) ? a.st_lc[(r - 1) * hid + tid] : a.cs0[(size_t)b * cs_ld + 2 * hid * l + tid];
                }
                const float gi = g[0], gj = g[1], gf = g[2], go = g[3];
                const float tc = tanhf(ct);
                const float dct = sdC[l * hid + tid] + dh * go * (1.0f - tc * tc);
                f32x4 dg;
                dg[0] = dct * gj * gi * (1.0f - gi);
                dg[1] = dct * gi * (1.0f - gj * gj);
                dg[2] = dct * cp * gf * (1.0f - gf);
                dg[3] = dh * tc * go * (1.0f - go);
                sdC[l * hid + tid] = dct * gf;
                reinterpret_cast<f32x4*>(sDG)[tid] = dg;
                if (l == NL - 1) {
                    reinterpret_cast<f32x4*>(a.dgates)[bt * hid + tid] = dg;
                } else {
                    float* dp = a.dpre + ((size_t)l * BS + bt) * 4 * hid;
                    dp[tid] = dg[0]; dp[hid + tid] = dg[1]; dp[2 * hid + tid] = dg[2]; dp[3 * hid + tid] = dg[3];
                }
            }
            __syncthreads();
            // B11: d[input ; h_prev] = dpre . W^T over this layer's block of Wb
            const int cb = (l == 0) ? a.s.cb0 : a.s.cb1, kg4 = cb >> 2;
            const int nslZ = max(1, T / kg4), nperZ = (4 * hid + nslZ - 1) / nslZ;
            const f32x4* Wl4 = Wb4 + ((l == 0) ? 0 : (size_t)hid * a.s.cb0 + (size_t)(l - 1) * hid * a.s.cb1);
            if (tid < nslZ * kg4) {
                const int cg = tid % kg4, sl = tid / kg4;
                const int r0 = sl * nperZ, r1 = min(4 * hid, r0 + nperZ);
                sPart4[sl * kg4 + cg] = ntk_stream_matvec<(MAXT > 768 ? 2 : 4)>(Wl4 + cg, kg4, sDG, r0, r1, 4 * hid - 1);
            }
            __syncthreads();
            const int base = (l == 0) ? 0 : RM + (l - 1) * hid, Kl = (l == 0) ? RM + hid : 2 * hid;
            if (tid < Kl) {
                float s = 0.f;
                for (int sl = 0; sl < nslZ; ++sl) s += sPart[sl * cb + tid];
                if (l > 0 && tid < hid) sdZ[base + tid] += s;     // d h_{l-1}(t): added to what step t+1 carried
                else sdZ[base + tid] = s;                           // d h_l(t-1) (layer 0: d read_{t-1} and d h_0(t-1))
            }
            if (l == NL - 1 && t > 0) ntm_bwd_commit(c, d, w, rec);  // next (earlier) step's records: every reader of the old ones has passed a barrier
            __syncthreads();
        }
    }

    // ---- gradient of the initial state
    for (int i = tid0; i < NMd; i += T) a.dM0[(size_t)b * NMd + i] = sdM[(i / Md) * MP + (i % Md)];
    for (int i = tid0; i < HN; i += T) a.dw0[(size_t)b * HN + i] = sdW[i];
    for (int i = tid0; i < RM; i += T) a.dread0[(size_t)b * RM + i] = sdZ[i];
    for (int i = tid0; i < NL * hid; i += T) {
        const int l = i / hid, j = i - l * hid;
        a.dcs0[(size_t)b * cs_ld + 2 * hid * l + j] = sdC[i];
        a.dcs0[(size_t)b * cs_ld + 2 * hid * l + hid + j] = sdZ[RM + i];
    }
}

// ------------------------------------------------------------------------------------------------ host side
// the instantiation a workgroup size takes (both deep kernels): the launchers and ntk_ntm_seq_deep_plan read it here
static inline int ntm_deep_kernel_id(int T) { return T <= 768 ? NTK_NTM_DEEP_768 : NTK_NTM_DEEP_1024; }

// the deep BPTT's LDS: its own users of `part` are the partials of B11 over the columns of a layer's block of Wb (cb0, cb1); the
// carried dZ holds every layer's dh behind dread, dC every layer's dc
static void ntm_deep_bwd_lds(const NtmDims& d, const NtmDeepShape& s, int T, int ldhT, NtmBwdLds& L) {
    ntm_bwd_lds(d, T, ldhT, ntm_imax(ntm_bwd_part_floats(T, s.cb0), ntm_bwd_part_floats(T, s.cb1)), s.RM + s.L * d.hid, s.L * d.hid, L);
}

// every limit of the two deep kernels, host arithmetic only
static int ntm_deep_plan(const NtmDims& d, const NtmDeepShape& s, NtmDeepPlan& p, const char* who) {
    NTK_REQUIRE(s.L >= 2, NTK_ERR_BAD_SHAPE, "%s: L=%d layers (the deep kernels take L >= 2; one layer is ntk_ntm_seq_fwd/bwd)", who, s.L);
    int rc = ntm_validate_dims(d, who);
    if (rc != NTK_OK) return rc;
    NTK_REQUIRE((d.hid % 4) == 0, NTK_ERR_UNSUPPORTED, "%s: hidden=%d must be a multiple of 4", who, d.hid);
    NTK_REQUIRE(d.SS + 1 <= NQ, NTK_ERR_UNSUPPORTED, "%s: shift space %d too wide", who, d.SS);
    p.Tf = ntm_pick_threads(d);                 // the forward takes the single-layer kernels' workgroup size
    NTK_REQUIRE(p.Tf >= d.N, NTK_ERR_UNSUPPORTED, "%s: mem_size %d exceeds the workgroup", who, d.N);
    // the BPTT's own clause: the 2*hid columns of a layer's input gradient (3*hid of the common rule already covers them).  Unlike
    // ntk_ntm_seq_bwd it does not grow the workgroup for a memory of more than MAXM elements per thread: that is refused below
    p.Tb = ntm_bwd_threads(d, 2 * d.hid);
    NTK_REQUIRE(p.Tb <= 1024 && d.H * d.N <= 1024 && d.N * d.Md <= MAXM * p.Tb, NTK_ERR_UNSUPPORTED,
                "%s: heads*mem_size=%d (max 1024) / mem_size*mem_dim=%d exceed one workgroup", who, d.H * d.N, d.N * d.Md);
    ntm_fwd_lds(d, p.Tf, p.Lf, s.L);
    ntm_deep_bwd_lds(d, s, p.Tb, ntm_align4(d.hid), p.Lb);
    p.lds_f = (size_t)p.Lf.total * sizeof(float);
    p.lds_b = (size_t)p.Lb.total * sizeof(float);
    NTK_REQUIRE(p.lds_f <= 160 * 1024 && p.lds_b <= 160 * 1024, NTK_ERR_UNSUPPORTED,
                "%s: %d layers of hidden=%d need %zu / %zu B of LDS (forward / BPTT; > 160 KiB)", who, s.L, d.hid, p.lds_f, p.lds_b);
    return NTK_OK;
}

extern "C" int ntk_ntm_seq_deep_supported(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L) {
    NtmDeepPlan p;                              // (answers for write_first = 0, as coded)
    return ntm_deep_plan(ntm_dims(B, 1, N, Md, R, Wh, hid, shift_range, O, 0, NTM_SIM_AS_CODED), ntm_deep_shape(1, R * Md, hid, L), p,
                         "ntk_ntm_seq_deep_supported") == NTK_OK ? 1 : 0;
}

extern "C" int ntk_ntm_seq_deep_plan_sim(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L, int write_first,
                                         int similarity, int* fwd_kernel, int* fwd_threads, int* bwd_kernel, int* bwd_threads) {
    NTM_REQUIRE_SIMILARITY(similarity, "ntk_ntm_seq_deep_plan");
    NtmDeepPlan p;
    const bool ok = ntm_deep_plan(ntm_dims(B, 1, N, Md, R, Wh, hid, shift_range, O, write_first, similarity), ntm_deep_shape(1, R * Md, hid, L),
                                  p, "ntk_ntm_seq_deep_plan") == NTK_OK;
    if (fwd_kernel) *fwd_kernel = !ok ? 0 : ntm_deep_kernel_id(p.Tf);
    if (fwd_threads) *fwd_threads = ok ? p.Tf : 0;
    if (bwd_kernel) *bwd_kernel = !ok ? 0 : ntm_deep_kernel_id(p.Tb);
    if (bwd_threads) *bwd_threads = ok ? p.Tb : 0;
    return ok ? (NTK_NTM_PLAN_FWD | NTK_NTM_PLAN_BWD) : 0;
}

extern "C" int ntk_ntm_seq_deep_plan(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L, int write_first,
                                     int* fwd_kernel, int* fwd_threads, int* bwd_kernel, int* bwd_threads) {
    return ntk_ntm_seq_deep_plan_sim(B, N, Md, R, Wh, hid, shift_range, O, L, write_first, NTM_SIM_AS_CODED, fwd_kernel, fwd_threads,
                                     bwd_kernel, bwd_threads);
}

extern "C" int ntk_ntm_seq_deep_packed_floats(int D, int R, int Md, int hid, int L, size_t* n_wx0, size_t* n_wf, size_t* n_wb) {
    NTK_REQUIRE(D >= 1 && R >= 1 && Md >= 1 && hid >= 1 && L >= 2, NTK_ERR_BAD_SHAPE,
                "ntk_ntm_seq_deep_packed_floats: D=%d R=%d Md=%d hid=%d L=%d", D, R, Md, hid, L);
    const NtmDeepShape s = ntm_deep_shape(D, R * Md, hid, L);
    if (n_wx0) *n_wx0 = ntm_deep_nwx0(s);
    if (n_wf) *n_wf = ntm_deep_nwf(s);
    if (n_wb) *n_wb = ntm_deep_nwb(s);
    return NTK_OK;
}

extern "C" int ntk_ntm_seq_deep_pack(int D, int R, int Md, int hid, int L, const float* lowerT, const float* top_WxT,
                                     const float* top_Wr, float* Wx0, float* Wf, float* Wb, void* stream) {
    NTK_REQUIRE(D >= 1 && R >= 1 && Md >= 1 && hid >= 1 && L >= 2, NTK_ERR_BAD_SHAPE,
                "ntk_ntm_seq_deep_pack: D=%d R=%d Md=%d hid=%d L=%d", D, R, Md, hid, L);
    NTK_REQUIRE((hid % 4) == 0, NTK_ERR_UNSUPPORTED, "ntk_ntm_seq_deep_pack: hidden=%d must be a multiple of 4", hid);
    NTK_REQUIRE(lowerT && top_WxT && top_Wr && Wx0 && Wf && Wb, NTK_ERR_BAD_PTR, "ntk_ntm_seq_deep_pack: null pointer");
    NTK_REQUIRE(ntk_aligned16(Wx0) && ntk_aligned16(Wf) && ntk_aligned16(Wb), NTK_ERR_BAD_PTR,
                "ntk_ntm_seq_deep_pack: Wx0/Wf/Wb must be 16-byte aligned");
    const NtmDeepShape s = ntm_deep_shape(D, R * Md, hid, L);
    const size_t n = ntm_deep_nwx0(s) + ntm_deep_nwf(s) + ntm_deep_nwb(s);
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    ntm_deep_pack_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(s, lowerT, top_WxT, top_Wr, Wx0, Wf, Wb);
    NTK_CHECK_LAUNCH("ntk_ntm_seq_deep_pack");
    return NTK_OK;
}


// ntk_ntm_seq_fwd_deep behind its plain and *_sim entries: similarity, then shape and plan, then pointers, then the launch.
// a.Wr, a.cs0 and a.cs_out come null: Wf and the L-layer state are in dp.
static int ntm_seq_fwd_deep_run(const NtmFwdArgs& a, NtmDeepFwdArgs dp, void* stream) {
    const char* who = "ntk_ntm_seq_fwd_deep";
    if (dp.s.L <= 2) dp.st_bufk = nullptr;                  // the record of layers 1 .. L-2
    NTM_REQUIRE_SIMILARITY(a.d.similarity, who);
    NTK_REQUIRE(dp.s.D >= 1, NTK_ERR_BAD_SHAPE, "%s: D=%d", who, dp.s.D);
    NtmDeepPlan p;
    int rc = ntm_deep_plan(a.d, dp.s, p, who);
    if (rc != NTK_OK) return rc;
    rc = ntm_fwd_check_ptrs(a, &dp, who);
    if (rc != NTK_OK) return rc;
    typedef void (*kern_t)(NtmFwdArgs, NtmDeepFwdArgs, NtmLds);
    constexpr int AC = NTM_SIM_AS_CODED, SC = NTM_SIM_SMOOTH_COSINE;
    static const NtmKernelRow<kern_t> rows[] = {
        {NTK_NTM_DEEP_768, AC, ntm_seq_fwd_deep_kernel<768>},   {NTK_NTM_DEEP_768, SC, ntm_seq_fwd_deep_kernel<768, SC>},
        {NTK_NTM_DEEP_1024, AC, ntm_seq_fwd_deep_kernel<1024>}, {NTK_NTM_DEEP_1024, SC, ntm_seq_fwd_deep_kernel<1024, SC>}};
    static NtkLdsAttrCache lds_cache;
    kern_t fn;
    rc = ntm_find_kernel(lds_cache, rows, ntm_deep_kernel_id(p.Tf), a.d.similarity, who, fn);
    if (rc != NTK_OK) return rc;
    fn<<<a.d.B, p.Tf, p.lds_f, (hipStream_t)stream>>>(a, dp, p.Lf);
    NTK_CHECK_LAUNCH(who);
    return NTK_OK;
}

// ntk_ntm_seq_bwd_deep likewise
static int ntm_seq_bwd_deep_run(const NtmDeepBwdArgs& a, void* stream) {
    const char* who = "ntk_ntm_seq_bwd_deep";
    NTM_REQUIRE_SIMILARITY(a.d.similarity, who);
    NtmDeepPlan p;
    int rc = ntm_deep_plan(a.d, a.s, p, who);
    if (rc != NTK_OK) return rc;
    NTK_REQUIRE(a.ldhT >= a.d.hid && (a.ldhT % 4) == 0, NTK_ERR_BAD_SHAPE, "%s: ldhT=%d (hid=%d)", who, a.ldhT, a.d.hid);
    rc = ntm_bwd_check_ptrs(a, who);
    if (rc != NTK_OK) return rc;
    if (a.ldhT != ntm_align4(a.d.hid)) ntm_deep_bwd_lds(a.d, a.s, p.Tb, a.ldhT, p.Lb);        // the plan laid it out for the smallest ldhT
    const size_t lds_bytes = (size_t)p.Lb.total * sizeof(float);
    NTK_REQUIRE(lds_bytes <= 160 * 1024, NTK_ERR_UNSUPPORTED, "%s: needs %zu B of LDS (> 160 KiB)", who, lds_bytes);
    typedef void (*kern_t)(NtmDeepBwdArgs, NtmBwdLds);
    constexpr int AC = NTM_SIM_AS_CODED, SC = NTM_SIM_SMOOTH_COSINE;
    static const NtmKernelRow<kern_t> rows[] = {
        {NTK_NTM_DEEP_768, AC, ntm_seq_bwd_deep_kernel<768>},   {NTK_NTM_DEEP_768, SC, ntm_seq_bwd_deep_kernel<768, SC>},
        {NTK_NTM_DEEP_1024, AC, ntm_seq_bwd_deep_kernel<1024>}, {NTK_NTM_DEEP_1024, SC, ntm_seq_bwd_deep_kernel<1024, SC>}};
    static NtkLdsAttrCache lds_cache;
    kern_t fn;
    rc = ntm_find_kernel(lds_cache, rows, ntm_deep_kernel_id(p.Tb), a.d.similarity, who, fn);
    if (rc != NTK_OK) return rc;
    fn<<<a.d.B, p.Tb, lds_bytes, (hipStream_t)stream>>>(a, p.Lb);
    NTK_CHECK_LAUNCH(who);
    return NTK_OK;
}

extern "C" int ntk_ntm_seq_fwd_deep_sim(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L,
                                    int write_first, int similarity, int D,
                                    const float* X, const float* xproj, const float* Wf, const float* Wa,
                                    const float* M0, const float* w0, const float* read0, const float* cs0,
                                    float* logits, float* outputs,
                                    float* M_out, float* w_out, float* read_out, float* cs_out,
                                    float* st_z, float* st_gates, float* st_c, float* st_h, float* st_u,
                                    float* st_wc, float* st_wv, float* st_w, float* st_M, float* st_read,
                                    float* st_xtop, float* st_buf0, float* st_bufk, float* st_lgates, float* st_lc,
                                    void* stream) {
    return ntm_seq_fwd_deep_run({ntm_dims(B, S, N, Md, R, Wh, hid, shift_range, O, write_first, similarity), xproj, nullptr, Wa, M0, w0, read0,
                                 nullptr, logits, outputs, M_out, w_out, read_out, nullptr, st_z, st_gates, st_c, st_h, st_u, st_wc, st_wv,
                                 st_w, st_M, st_read},
                                {ntm_deep_shape(D, R * Md, hid, L), X, Wf, cs0, cs_out, st_xtop, st_buf0, st_bufk, st_lgates, st_lc}, stream);
}

extern "C" int ntk_ntm_seq_fwd_deep(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L,
                                    int write_first, int D,
                                    const float* X, const float* xproj, const float* Wf, const float* Wa,
                                    const float* M0, const float* w0, const float* read0, const float* cs0,
                                    float* logits, float* outputs,
                                    float* M_out, float* w_out, float* read_out, float* cs_out,
                                    float* st_z, float* st_gates, float* st_c, float* st_h, float* st_u,
                                    float* st_wc, float* st_wv, float* st_w, float* st_M, float* st_read,
                                    float* st_xtop, float* st_buf0, float* st_bufk, float* st_lgates, float* st_lc,
                                    void* stream) {
    return ntm_seq_fwd_deep_run({ntm_dims(B, S, N, Md, R, Wh, hid, shift_range, O, write_first, NTM_SIM_AS_CODED), xproj, nullptr, Wa, M0, w0,
                                 read0, nullptr, logits, outputs, M_out, w_out, read_out, nullptr, st_z, st_gates, st_c, st_h, st_u, st_wc,
                                 st_wv, st_w, st_M, st_read},
                                {ntm_deep_shape(D, R * Md, hid, L), X, Wf, cs0, cs_out, st_xtop, st_buf0, st_bufk, st_lgates, st_lc}, stream);
}

extern "C" int ntk_ntm_seq_bwd_deep_sim(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L,
                                    int write_first, int similarity,
                                    const float* Wb, const float* WaT, int ldhT,
                                    const float* M0, const float* w0, const float* cs0,
                                    const float* st_gates, const float* st_c, const float* st_u,
                                    const float* st_wc, const float* st_wv, const float* st_w, const float* st_M,
                                    const float* st_lgates, const float* st_lc,
                                    const float* dlogits,
                                    const float* dM_fin, const float* dw_fin, const float* dread_fin, const float* dcs_fin,
                                    float* dgates, float* dpre, float* du, float* dM0, float* dw0, float* dread0, float* dcs0,
                                    void* stream) {
    return ntm_seq_bwd_deep_run({ntm_dims(B, S, N, Md, R, Wh, hid, shift_range, O, write_first, similarity), ntm_deep_shape(1, R * Md, hid, L),
                                 Wb, WaT, ldhT, M0, w0, cs0, st_gates, st_c, st_u, st_wc, st_wv, st_w, st_M, st_lgates, st_lc, dlogits,
                                 dM_fin, dw_fin, dread_fin, dcs_fin, dgates, dpre, du, dM0, dw0, dread0, dcs0}, stream);
}

extern "C" int ntk_ntm_seq_bwd_deep(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L,
                                    int write_first,
                                    const float* Wb, const float* WaT, int ldhT,
                                    const float* M0, const float* w0, const float* cs0,
                                    const float* st_gates, const float* st_c, const float* st_u,
                                    const float* st_wc, const float* st_wv, const float* st_w, const float* st_M,
                                    const float* st_lgates, const float* st_lc,
                                    const float* dlogits,
                                    const float* dM_fin, const float* dw_fin, const float* dread_fin, const float* dcs_fin,
                                    float* dgates, float* dpre, float* du, float* dM0, float* dw0, float* dread0, float* dcs0,
                                    void* stream) {
    return ntm_seq_bwd_deep_run({ntm_dims(B, S, N, Md, R, Wh, hid, shift_range, O, write_first, NTM_SIM_AS_CODED),
                                 ntm_deep_shape(1, R * Md, hid, L), Wb, WaT, ldhT, M0, w0, cs0, st_gates, st_c, st_u, st_wc, st_wv, st_w, st_M,
                                 st_lgates, st_lc, dlogits, dM_fin, dw_fin, dread_fin, dcs_fin, dgates, dpre, du, dM0, dw0, dread0, dcs0}, stream);
}
