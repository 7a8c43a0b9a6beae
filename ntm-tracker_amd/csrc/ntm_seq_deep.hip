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
// The single-layer kernels are not touched: these are kernels of their own, with argument structs of their own.
#include "ntm_common.h"
#include "ntm_fwd_args.h"
#include <initializer_list>

// ------------------------------------------------------------------------------------------------ packed layouts
// (hid % 4 == 0, see ntk_ntm_seq_deep_supported)
//   Wx0 [4*hid][ldx]              layer 0's x part, rows n' = unit*4 + gate, columns x (zero padded to ldx = align4(D))
//   Wf  forward recurrent blocks, columns n' = unit*4 + gate:
//       layer 0    [rf0][4*hid]   rows read (R*Md) | h_0 (hid) | bias | 0..       rf0 = align4(R*Md + hid + 1)
//       layer k>=1 [rf1][4*hid]   rows h_{k-1} (hid) | h_k (hid) | bias | 0..     rf1 = align4(2*hid + 1)
//   Wb  the same blocks transposed (for d[input ; h_prev] = dpre . W^T), rows n' = unit*4 + gate, no bias:
//       layer 0    [4*hid][cb0]   columns read | h_0 | 0..                        cb0 = align4(R*Md + hid)
//       layer k>=1 [4*hid][cb1]   columns h_{k-1} | h_k                          cb1 = 2*hid
// Source (StackedNTMCell's flat buffer): lowerT = the L-1 lower matrices back to back, layer 0 [4*hid][ld0]
// (columns x | read | h_0 | bias | 0.., ld0 = align4(D + R*Md + hid + 1)), layers 1..L-2 [4*hid][ld1] (columns
// h_{k-1} | h_k | bias | 0.., ld1 = align4(2*hid + 1)), rows g*hid + unit (TF gate-major); the top layer as the
// single-layer cell's WxT [4*hid][align4(hid)] (its input h_{L-2}) and Wr [align4(R*Md+hid+1)][4*hid] (read rows unused).
struct NtmDeepShape {
    int D, RM, hid, L, ldx, ld0, ld1, ldxt, rf0, rf1, cb0, cb1;
};

static inline void ntm_deep_shape(NtmDeepShape& s, int D, int RM, int hid, int L) {
    s.D = D; s.RM = RM; s.hid = hid; s.L = L;
    s.ldx = ntm_align4(D);
    s.ld0 = ntm_align4(D + RM + hid + 1);
    s.ld1 = ntm_align4(2 * hid + 1);
    s.ldxt = ntm_align4(hid);
    s.rf0 = ntm_align4(RM + hid + 1);
    s.rf1 = ntm_align4(2 * hid + 1);
    s.cb0 = ntm_align4(RM + hid);
    s.cb1 = 2 * hid;
}

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
struct NtmDeepFwdArgs {
    NtmDeepShape s;
    const float* X;        // [B,S,ldx] input rows (read for the st_buf0 record only)
    const float* Wf;       // forward blocks (above)
    const float* cs0;      // [B,2*hid*L]  c_0, h_0, c_1, h_1, ...
    float* cs_out;         // [B,2*hid*L]
    // per-step records of the lower layers and of the top layer's input (all nullable)
    float* st_xtop;        // [B,S,ldxt]         h_{L-2}(t), zero padded
    float* st_buf0;        // [B,S,ld0]          [x_t | read_{t-1} | h_0(t-1) | 1 | 0..]
    float* st_bufk;        // [L-2][B,S,ld1]     layer k = 1..L-2: [h_{k-1}(t) | h_k(t-1) | 1 | 0..]
    float* st_lgates;      // [L-1][B,S,hid,4]   activated gates i, j, f, o of layers 0..L-2
    float* st_lc;          // [L-1][B,S,hid]     c_k(t) of layers 0..L-2
};

static inline void ntm_deep_fwd_lds(const NtmDims& d, int NL, int T, NtmLds& L) {
    const int MP = d.Md | 1;
    const int nsl = ntm_imax(1, T / d.hid);
    const int ncg = d.PP / 4;
    const int nslB = ntm_imin(ntm_imax(1, T / ncg), d.hid);
    const int RM = d.R * d.Md;
    const int nslR = ntm_imin(ntm_imax(1, T / RM), d.N);
    int o = 0;
    L.part = o; o += ntm_align4(ntm_imax(ntm_imax(nsl * 4 * d.hid, nslB * d.PP), nslR * RM));
    L.M = o; o += ntm_align4(d.N * MP);
    L.W = o; o += ntm_align4(d.H * d.N);
    L.Wg = o; o += ntm_align4(d.H * d.N);
    L.Z = o; o += ntm_align4(RM + NL * d.hid);
    L.C = o; o += ntm_align4(NL * d.hid);
    L.U = o; o += ntm_align4(d.PP);
    L.Ks = o; o += ntm_align4(d.H * d.Md);
    L.Cn = o; o += ntm_align4(ntm_norm_floats(d));
    L.Pw = o; o += ntm_align4(d.H * d.N);
    L.total = o;
}

template <int MAXT, int SIM = NTM_SIM_AS_CODED>             // SIM: the similarity of the content addressing, as ntm_seq_fwd.hip
__global__ __launch_bounds__(MAXT) void ntm_seq_fwd_deep_kernel(NtmFwdArgs a, NtmDeepFwdArgs dp, NtmLds L) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr bool SMOOTH = SIM == NTM_SIM_SMOOTH_COSINE;
    const int b = blockIdx.x, tid0 = threadIdx.x, T = blockDim.x;
    const int N = a.d.N, Md = a.d.Md, MP = Md | 1, R = a.d.R, Wh = a.d.Wh;
    const int H = R + Wh, hid = a.d.hid, SS = a.d.SS, NL = dp.s.L;
    const int S = a.d.S, RM = R * Md, K = RM + hid;
    const size_t BS = (size_t)a.d.B * S;
    struct {
        int O, oK, oB, oG, oS, oY, oE, oA, P, PP, ldz, ldh, write_first;
    } d;
    d.O = a.d.O;
    d.oK = 0; d.oB = H * Md; d.oG = d.oB + H; d.oS = d.oG + H; d.oY = d.oS + H * SS; d.oE = d.oY + H;
    d.oA = d.oE + Wh * Md; d.P = d.oA + Wh * Md;
    d.PP = (d.P + d.O + 3) & ~3; d.ldz = (K + 1 + 3) & ~3; d.ldh = (hid + 1 + 3) & ~3;
    d.write_first = a.d.write_first;
    const int PP = d.PP;
    const NtmDeepShape& sh = dp.s;

    float* sPart = smem + L.part;
    float* sM = smem + L.M;
    float* sW = smem + L.W;
    float* sWg = smem + L.Wg;
    float* sZ = smem + L.Z;                 // [read | h_0 | .. | h_{L-1}]
    float* sC = smem + L.C;                 // [c_0 | .. | c_{L-1}]
    float* sU = smem + L.U;
    float* sKs = smem + L.Ks;
    float* sCn = smem + L.Cn;
    float* sPw = smem + L.Pw;
    float* sHtop = sZ + RM + (NL - 1) * hid;

    const int nsl = max(1, T / hid);        // K-slices of the gate products
    const int ncg = PP >> 2;
    const int nslB = min(max(1, T / ncg), hid);
    const int kperB = (hid + nslB - 1) / nslB;
    const int nslR = min(max(1, T / RM), N);
    const int nperR = (N + nslR - 1) / nslR;
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
        const int wave = tid >> 6, nwaves = T >> 6;
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
            if (l == NL - 1) {  // waves not running the LSTM normalise the feature columns of M over the slots (ops.py:150)
                const int w0 = (hid + 63) >> 6;
                if constexpr (SMOOTH) {     // smooth cosine: the row norms |M[n]|, a lane per slot, no clamp
                    if (wave >= w0) {
                        for (int n = (wave - w0) * 64 + lane; n < N; n += (nwaves - w0) * 64) {
                            float sq = 0.f;
                            for (int m = 0; m < Md; ++m) { const float v = sM[n * MP + m]; sq += v * v; }
                            sCn[n] = sqrtf(sq);
                        }
                    }
                } else
                if (wave >= w0) {
                    for (int m = wave - w0; m < Md; m += nwaves - w0) {
                        float sq = 0.f;
                        for (int n = lane; n < N; n += 64) { const float v = sM[n * MP + m]; sq += v * v; }
                        sq = wave_sum(sq);
                        if (lane == 0) sCn[m] = 1.0f / sqrtf(fmaxf(sq, 1e-12f));
                    }
                }
            }
            __syncthreads();
        }
        // ------------------------------------------------------------ P3: unpack / output partials on h_{L-1}
        if (tid < nslB * ncg) {
            const int cg = tid % ncg, ks = tid / ncg;
            const int k0 = ks * kperB, k1 = min(hid, k0 + kperB);
            sPart4[ks * ncg + cg] = ntk_stream_matvec<(MAXT > 768 ? 2 : 4)>(Wa4 + cg, ncg, sHtop, k0, k1, hid);
        }
        __syncthreads();
        // ------------------------------------------------------------ P4: control activations
        if (tid < PP) {
            float v = a.Wa[(size_t)hid * PP + tid];
            for (int ks = 0; ks < nslB; ++ks) v += sPart[ks * PP + tid];
            float r = v;
            if (tid < d.oB) r = ntm_tanh(v);
            else if (tid < d.oG) r = ntm_softplus(v);
            else if (tid < d.oS) r = ntm_sigmoid(v);
            else if (tid < d.oY) r = v;
            else if (tid < d.oE) r = ntm_softplus(v) + 1.0f;
            else if (tid < d.oA) r = ntm_sigmoid(v);
            else if (tid < d.P) r = ntm_tanh(v);
            sU[tid] = r;
            if (a.st_u) a.st_u[bt * PP + tid] = r;
            if (tid >= d.P && tid < d.P + d.O) a.logits[bt * d.O + (tid - d.P)] = v;
        }
        __syncthreads();
        // ------------------------------------------------------------ P5-P7: addressing, one wave per head (ntm_seq_fwd.hip)
        if (wave < H) {
            const int h = wave;
            float kss = 0.f;
            for (int m = 0; m < Md; ++m) { const float kv = sU[d.oK + h * Md + m]; kss += kv * kv; }
            const float kn = sqrtf(kss);                           // |k|, smooth cosine only
            if constexpr (SMOOTH) {
                for (int m = lane; m < Md; m += 64) sKs[h * Md + m] = sU[d.oK + h * Md + m];
            } else {
                const float kinv = 1.0f / sqrtf(fmaxf(kss, 1e-12f));
                for (int m = lane; m < Md; m += 64) sKs[h * Md + m] = sU[d.oK + h * Md + m] * kinv * sCn[m];
            }
            const float beta = sU[d.oB + h], g = sU[d.oG + h], gamma = sU[d.oY + h];
            float swv[NTM_MAX_SHIFT_TAPS];
            {
                float mx = -INFINITY;
#pragma unroll
                for (int j = 0; j < NTM_MAX_SHIFT_TAPS; ++j) if (j < SS) mx = fmaxf(mx, sU[d.oS + h * SS + j]);
                float sum = 0.f;
#pragma unroll
                for (int j = 0; j < NTM_MAX_SHIFT_TAPS; ++j) { swv[j] = (j < SS) ? ntm_exp(sU[d.oS + h * SS + j] - mx) : 0.f; sum += swv[j]; }
#pragma unroll
                for (int j = 0; j < NTM_MAX_SHIFT_TAPS; ++j) swv[j] = swv[j] / sum;
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            float mxv = -INFINITY;
            for (int n = lane; n < N; n += 64) {
                float sim = 0.f;
                for (int m = 0; m < Md; ++m) sim += sKs[h * Md + m] * sM[n * MP + m];
                if constexpr (SMOOTH) sim = sim / (sCn[n] * kn + 1e-3f);
                const float v = sim * beta;
                sWg[h * N + n] = v;
                mxv = fmaxf(mxv, v);
            }
            mxv = wave_max(mxv);
            float sum = 0.f;
            for (int n = lane; n < N; n += 64) { const float e = ntm_exp(sWg[h * N + n] - mxv); sWg[h * N + n] = e; sum += e; }
            sum = wave_sum(sum);
            for (int n = lane; n < N; n += 64) {
                const float wc = sWg[h * N + n] / sum;
                if (a.st_wc) a.st_wc[(bt * H + h) * N + n] = wc;
                sWg[h * N + n] = wc * g + sW[h * N + n] * (1.0f - g);
            }
            __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
            __builtin_amdgcn_wave_barrier();
            const int start = -((SS + 1) >> 1);                    // Py2 floor of -SS/2 (Q2)
            float psum = 0.f;
            for (int n = lane; n < N; n += 64) {
                float wv = 0.f;
#pragma unroll
                for (int j = 0; j < NTM_MAX_SHIFT_TAPS; ++j) {
                    if (j < SS) {
                        int src = n + start + j;
                        src = (src % N + N) % N;
                        wv += swv[j] * sWg[h * N + src];
                    }
                }
                if (a.st_wv) a.st_wv[(bt * H + h) * N + n] = wv;
                const float pw = ntm_pow(wv, gamma);
                sPw[h * N + n] = pw;
                psum += pw;
            }
            psum = wave_sum(psum);
            for (int n = lane; n < N; n += 64) {
                const float w = sPw[h * N + n] / (psum + 1e-3f);
                sW[h * N + n] = w;
                if (a.st_w) a.st_w[(bt * H + h) * N + n] = w;
            }
        } else if (wave == H && lane == 0 && a.outputs) {
            float mx = -INFINITY;
            for (int j = 0; j < d.O; ++j) mx = fmaxf(mx, sU[d.P + j]);
            float sum = 0.f;
            for (int j = 0; j < d.O; ++j) sum += expf(sU[d.P + j] - mx);
            for (int j = 0; j < d.O; ++j) a.outputs[bt * d.O + j] = expf(sU[d.P + j] - mx) / sum;
        }
        __syncthreads();
        // ------------------------------------------------------------ P8: write + read
        auto update_M = [&]() {
            for (int idx = tid; idx < N * Md; idx += T) {
                const int n = idx / Md, m = idx - n * Md;
                float E = 1.f, A = 0.f;
                for (int j = 0; j < Wh; ++j) {
                    const float ww = sW[(R + j) * N + n];
                    E *= (1.0f - ww * sU[d.oE + j * Md + m]);
                    A += ww * sU[d.oA + j * Md + m];
                }
                const float nm = sM[n * MP + m] * E + A;
                sM[n * MP + m] = nm;
                if (a.st_M) a.st_M[bt * N * Md + idx] = nm;
            }
        };
        if (d.write_first) { update_M(); __syncthreads(); }
        if (tid < nslR * RM) {
            const int o = tid % RM, sl = tid / RM;
            const int i = o / Md, m = o - i * Md;
            const int n0 = sl * nperR, n1 = min(N, n0 + nperR);
            float s0 = 0.f, s1 = 0.f;
            int n = n0;
            for (; n + 1 < n1; n += 2) {
                s0 += sW[i * N + n] * sM[n * MP + m];
                s1 += sW[i * N + n + 1] * sM[(n + 1) * MP + m];
            }
            if (n < n1) s0 += sW[i * N + n] * sM[n * MP + m];
            sPart[sl * RM + o] = s0 + s1;
        }
        __syncthreads();
        if (!d.write_first) update_M();
        if (tid < RM) {
            float sr = 0.f;
            for (int sl = 0; sl < nslR; ++sl) sr += sPart[sl * RM + tid];
            sZ[tid] = sr;
            if (a.st_read) a.st_read[bt * RM + tid] = sr;
        }
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
// The generic form of ntm_seq_bwd_kernel (phases X1 .. B9 unchanged: heads, memory, unpack), then the LSTM backward once per
// layer, top first: B10 (cell backward; the top layer adds dU . Wa^T to its carried dh) and B11 (d[input ; h_prev] = dpre . W^T,
// streamed).  Layer k's input gradient is added to the carried dh_{k-1} (which layer k-1 consumes next), its h_prev part replaces
// the carried dh_k; layer 0's splits into the carried dread and dh_0.  Fixed summation order, no atomics: bitwise reproducible.
struct NtmDeepBwdArgs {
    NtmDims d;
    NtmDeepShape s;
    const float* Wb;       // transposed recurrent blocks (above)
    const float* WaT;      // [PP][ldhT]
    int ldhT;
    const float* M0; const float* w0;
    const float* cs0;      // [B,2*hid*L]
    const float* st_gates; const float* st_c; const float* st_u;       // the top layer and the heads, as ntm_seq_bwd.hip
    const float* st_wc; const float* st_wv; const float* st_w; const float* st_M;
    const float* st_lgates; const float* st_lc;                        // [L-1][B,S,hid,4], [L-1][B,S,hid]
    const float* dlogits;  // [B,S,O]
    const float* dM_fin; const float* dw_fin; const float* dread_fin; const float* dcs_fin;     // nullable; dcs [B,2*hid*L]
    float* dgates;         // [B,S,4*hid]       top layer, n' = unit*4 + gate
    float* dpre;           // [L-1][B,S,4*hid]  layers 0..L-2, TF gate-major (g*hid + unit)
    float* du;             // [B,S,PP]
    float* dM0; float* dw0; float* dread0; float* dcs0;                // dcs0 [B,2*hid*L]
};

struct NtmDeepBwdLds {
    int part, dM, G, Mp, Mt, dW, Wp, Wt, Wc, Wv, Wg, Dwv, Dsim, U, DU, DG, dZ, dC, Gt, Ct, Cp,
        Khat, Ks, Kinv, Kss, Cinv, Css, C2, Dkhat, Sw, Red, Dmh, total;
};

// per-head reduction slots and the record prefetch depth, as ntm_seq_bwd.hip
constexpr int DNQ = 1 + NTM_MAX_SHIFT_TAPS;
constexpr int DQR1 = 0, DQR2 = 2, DQR3 = DQR2 + DNQ, DQR4 = DQR3 + 2;
constexpr int DNQT = DQR4 + 1;    // (smooth cosine: one more, DQR4 + 1 = sum_n b rn)
constexpr int DMAXM = 8;

static void ntm_deep_bwd_lds(const NtmDims& d, const NtmDeepShape& s, int T, int ldhT, NtmDeepBwdLds& L) {
    const int MP = d.Md | 1, NM = d.N * MP, HN = d.H * d.N;
    const int nout = d.H * d.Md + 2 * d.Wh * d.Md;
    const int nslP = ntm_imin(ntm_imax(1, T / nout), d.N);
    const int nslH = ntm_imax(1, T / (ldhT / 4));
    const int nslC = ntm_imax(1, T / d.Md);
    int part = ntm_imax(nslP * nout, nslH * ldhT);
    part = ntm_imax(part, nslC * d.Md);
    for (int cb : {s.cb0, s.cb1}) part = ntm_imax(part, ntm_imax(1, T / (cb / 4)) * cb);
    int o = 0;
    auto take = [&](int n) { int r = o; o += ntm_align4(n); return r; };
    L.part = take(part);
    L.dM = take(NM); L.G = take(NM); L.Mp = take(NM); L.Mt = take(d.write_first ? NM : 4);
    L.dW = take(HN); L.Wp = take(HN); L.Wt = take(HN); L.Wc = take(HN); L.Wv = take(HN); L.Wg = take(HN);
    L.Dwv = take(HN); L.Dsim = take(HN);
    L.U = take(d.PP); L.DU = take(d.PP); L.DG = take(4 * d.hid);
    L.dZ = take(s.RM + s.L * d.hid); L.dC = take(s.L * d.hid);
    L.Gt = take(4 * d.hid); L.Ct = take(d.hid); L.Cp = take(d.hid);
    L.Khat = take(d.H * d.Md); L.Ks = take(d.H * d.Md); L.Kinv = take(d.H); L.Kss = take(d.H);
    L.Cinv = take(ntm_norm_floats(d)); L.Css = take(d.Md); L.C2 = take(ntm_norm_floats(d)); L.Dkhat = take(d.H * d.Md);
    L.Sw = take(d.H * d.SS);
    L.Red = take(d.H * (DNQT + (d.similarity == NTM_SIM_SMOOTH_COSINE ? 1 : 0)) * (d.N / 64));
    L.Dmh = take(d.N * (d.Md | 1));
    L.total = o;
}

template <int MAXT, int SIM = NTM_SIM_AS_CODED>             // SIM: as ntm_seq_bwd.hip
__global__ __launch_bounds__(MAXT) void ntm_seq_bwd_deep_kernel(NtmDeepBwdArgs a, NtmDeepBwdLds L) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr bool SMOOTH = SIM == NTM_SIM_SMOOTH_COSINE;
    constexpr int NQS = DNQT + (SMOOTH ? 1 : 0);         // reduction slots per head
    const int b = blockIdx.x, tid0 = threadIdx.x, T = blockDim.x;
    const int N = a.d.N, Md = a.d.Md, MP = Md | 1, R = a.d.R, Wh = a.d.Wh;
    const int H = R + Wh, hid = a.d.hid, SS = a.d.SS, NL = a.s.L;
    const int S = a.d.S, RM = R * Md, NW = N >> 6, NMd = N * Md, HN = H * N;
    const size_t BS = (size_t)a.d.B * S;
    struct {
        int O, oK, oB, oG, oS, oY, oE, oA, P, PP;
    } d;
    d.O = a.d.O;
    d.oK = 0; d.oB = H * Md; d.oG = d.oB + H; d.oS = d.oG + H; d.oY = d.oS + H * SS; d.oE = d.oY + H;
    d.oA = d.oE + Wh * Md; d.P = d.oA + Wh * Md;
    d.PP = (d.P + d.O + 3) & ~3;
    const int PP = d.PP;
    const bool wf = a.d.write_first != 0;
    const int ldhT = a.ldhT, cs_ld = 2 * hid * NL;
    int tid = tid0, lane = tid0 & 63;

    float* sPart = smem + L.part;
    float* sdM = smem + L.dM;  float* sG = smem + L.G;  float* sMp = smem + L.Mp;  float* sMt = smem + L.Mt;
    float* sdW = smem + L.dW;  float* sWp = smem + L.Wp; float* sWt = smem + L.Wt; float* sWc = smem + L.Wc;
    float* sWv = smem + L.Wv;  float* sWg = smem + L.Wg; float* sDwv = smem + L.Dwv; float* sDsim = smem + L.Dsim;
    float* sU = smem + L.U;    float* sDU = smem + L.DU; float* sDG = smem + L.DG;
    float* sdZ = smem + L.dZ;  // carried [dread | dh_0 | .. | dh_{L-1}]
    float* sdC = smem + L.dC;  // carried [dc_0 | .. | dc_{L-1}]
    float* sGt = smem + L.Gt;  float* sCt = smem + L.Ct; float* sCp = smem + L.Cp;
    float* sKhat = smem + L.Khat; float* sKs = smem + L.Ks; float* sKinv = smem + L.Kinv; float* sKss = smem + L.Kss;
    float* sCinv = smem + L.Cinv; float* sCss = smem + L.Css; float* sC2 = smem + L.C2; float* sDkhat = smem + L.Dkhat;
    float* sSw = smem + L.Sw;  float* sRed = smem + L.Red;  float* sDmh = smem + L.Dmh;
    float* sRn = sCinv; float* sRc = sC2;  // smooth cosine: [N] row norms |M_prev[n]| and the row-norm coefficients where the [Md] column terms are
    f32x4* sPart4 = reinterpret_cast<f32x4*>(sPart);
    const f32x4* Wb4 = reinterpret_cast<const f32x4*>(a.Wb);

    // thread roles
    int hh = tid / N, nn = tid - hh * N;                // (head, slot) owner; active iff hh < H
    bool hn = hh < H;
    int wi = nn >> 6;
    const int nout = H * Md + 2 * Wh * Md;
    const int nslP = min(max(1, T / nout), N);
    const int nperP = (N + nslP - 1) / nslP;
    const int hg4 = ldhT >> 2;
    const int nslH = max(1, T / hg4), nperH = (PP + nslH - 1) / nslH;
    const int nslC = max(1, T / Md), nperC = (N + nslC - 1) / nslC;

    // ---- prefetch registers for one step's records (the top layer's and the heads')
    float pM[DMAXM], pMt[DMAXM], pWp = 0.f, pWt = 0.f, pWc = 0.f, pWv = 0.f, pU = 0.f, pCt = 0.f, pCp = 0.f, pDl = 0.f;
    f32x4 pG = {0.f, 0.f, 0.f, 0.f};
    auto prefetch = [&](int t) {
        const size_t bt = (size_t)b * S + t;
        const float* Mp = (t > 0) ? a.st_M + (bt - 1) * NMd : a.M0 + (size_t)b * NMd;
#pragma unroll
        for (int q = 0; q < DMAXM; ++q) {
            const int idx = tid + q * T;
            pM[q] = (idx < NMd) ? Mp[idx] : 0.f;
            pMt[q] = (wf && idx < NMd) ? a.st_M[bt * NMd + idx] : 0.f;
        }
        if (hn) {
            pWp = (t > 0) ? a.st_w[(bt - 1) * HN + tid] : a.w0[(size_t)b * HN + tid];
            pWt = a.st_w[bt * HN + tid];
            pWc = a.st_wc[bt * HN + tid];
            pWv = a.st_wv[bt * HN + tid];
        }
        if (tid < PP) {
            pU = a.st_u[bt * PP + tid];
            pDl = (tid >= d.P && tid < d.P + d.O) ? a.dlogits[bt * d.O + (tid - d.P)] : 0.f;
        }
        if (tid < hid) {
            pG = reinterpret_cast<const f32x4*>(a.st_gates)[bt * hid + tid];
            pCt = a.st_c[bt * hid + tid];
            pCp = (t > 0) ? a.st_c[(bt - 1) * hid + tid] : a.cs0[(size_t)b * cs_ld + 2 * hid * (NL - 1) + tid];
        }
    };
    auto commit = [&]() {
#pragma unroll
        for (int q = 0; q < DMAXM; ++q) {
            const int idx = tid + q * T;
            if (idx < NMd) {
                const int n = idx / Md, m = idx - n * Md;
                sMp[n * MP + m] = pM[q];
                if (wf) sMt[n * MP + m] = pMt[q];
            }
        }
        if (hn) { sWp[tid] = pWp; sWt[tid] = pWt; sWc[tid] = pWc; sWv[tid] = pWv; }
        if (tid < PP) { sU[tid] = pU; sDU[tid] = pDl; }
        if (tid < hid) { reinterpret_cast<f32x4*>(sGt)[tid] = pG; sCt[tid] = pCt; sCp[tid] = pCp; }
    };

    // ---- carried gradients start from the (optional) gradient of the final state
    for (int i = tid; i < NMd; i += T)
        sdM[(i / Md) * MP + (i % Md)] = a.dM_fin ? a.dM_fin[(size_t)b * NMd + i] : 0.f;
    for (int i = tid; i < HN; i += T) sdW[i] = a.dw_fin ? a.dw_fin[(size_t)b * HN + i] : 0.f;
    for (int i = tid; i < RM + NL * hid; i += T) {
        float v = 0.f;
        if (i < RM) {
            v = a.dread_fin ? a.dread_fin[(size_t)b * RM + i] : 0.f;
        } else if (a.dcs_fin) {
            const int l = (i - RM) / hid, j = (i - RM) - l * hid;
            v = a.dcs_fin[(size_t)b * cs_ld + 2 * hid * l + hid + j];
        }
        sdZ[i] = v;
    }
    for (int i = tid; i < NL * hid; i += T) {
        const int l = i / hid, j = i - l * hid;
        sdC[i] = a.dcs_fin ? a.dcs_fin[(size_t)b * cs_ld + 2 * hid * l + j] : 0.f;
    }
    prefetch(S - 1);
    commit();
    __syncthreads();

    // per-head block reduction of nq values held by the (h, n) owner threads
    auto red_write = [&](const float (&v)[DNQ], int nq, int base) {
#pragma unroll
        for (int q = 0; q < DNQ; ++q) {
            if (q < nq) {
                const float s = wave_sum(hn ? v[q] : 0.f);
                if (hn && lane == 0) sRed[(hh * NQS + base + q) * NW + wi] = s;
            }
        }
    };
    auto red_read = [&](int h, int q) -> float {
        float s = 0.f;
        for (int w = 0; w < NW; ++w) s += sRed[(h * NQS + q) * NW + w];
        return s;
    };

    for (int t = S - 1; t >= 0; --t) {
        {   // opaque thread id (see ntm_seq_bwd.hip)
            int tid_op = tid0;
            asm volatile("" : "+v"(tid_op));
            tid = tid_op; lane = tid & 63;
            hh = tid / N; nn = tid - hh * N; hn = hh < H; wi = nn >> 6;
        }
        const size_t bt = (size_t)b * S + t;
        if (t > 0) prefetch(t - 1);

        // ------------------------------------------------ X1: memory-shaped elementwise + column norms + small vectors
        for (int idx = tid; idx < NMd; idx += T) {
            const int n = idx / Md, m = idx - n * Md, ai = n * MP + m;
            float dMt = sdM[ai];
            float dMr = 0.f;
            for (int i = 0; i < R; ++i) dMr += sWt[i * N + n] * sdZ[i * Md + m];
            if (wf) dMt += dMr;
            float E = 1.f;
            for (int j = 0; j < Wh; ++j) E *= (1.0f - sWt[(R + j) * N + n] * sU[d.oE + j * Md + m]);
            sG[ai] = dMt;
            sdM[ai] = dMt * E + (wf ? 0.f : dMr);
        }
        if constexpr (SMOOTH) {
            if (tid < N) {         // row norms of M_prev, no clamp
                float s = 0.f;
                for (int m = 0; m < Md; ++m) { const float v = sMp[tid * MP + m]; s += v * v; }
                sRn[tid] = sqrtf(s);
            }
        } else
        if (tid < nslC * Md) {     // column sum of squares of M_prev (quirk Q1 normaliser)
            const int m = tid % Md, sl = tid / Md;
            const int n0 = sl * nperC, n1 = min(N, n0 + nperC);
            float s = 0.f;
            for (int n = n0; n < n1; ++n) { const float v = sMp[n * MP + m]; s += v * v; }
            sPart[sl * Md + m] = s;
        }
        if (tid < H) {             // key norms and shift softmax
            const int h = tid;
            float ss = 0.f;
            for (int m = 0; m < Md; ++m) { const float kv = sU[d.oK + h * Md + m]; ss += kv * kv; }
            sKss[h] = ss;
            sKinv[h] = SMOOTH ? sqrtf(ss) : 1.0f / sqrtf(fmaxf(ss, 1e-12f));        // smooth cosine: |k| itself
            float mx = -INFINITY;
            for (int j = 0; j < SS; ++j) mx = fmaxf(mx, sU[d.oS + h * SS + j]);
            float sum = 0.f;
            for (int j = 0; j < SS; ++j) sum += expf(sU[d.oS + h * SS + j] - mx);
            for (int j = 0; j < SS; ++j) sSw[h * SS + j] = expf(sU[d.oS + h * SS + j] - mx) / sum;
        }
        __syncthreads();

        // ------------------------------------------------ X2: d(w_t) for every head; R1 sums
        float dwt = 0.f, pw = 0.f, wv = 0.f, wt = 0.f, wc = 0.f, wp = 0.f, gam = 1.f, gate = 0.f;
        float rv[DNQ];
        if (!SMOOTH && tid < Md) {
            float s = 0.f;
            for (int sl = 0; sl < nslC; ++sl) s += sPart[sl * Md + tid];
            sCss[tid] = s;
            sCinv[tid] = 1.0f / sqrtf(fmaxf(s, 1e-12f));
        }
        if (hn) {
            const int h = hh, n = nn;
            float acc = sdW[tid];
            if (h < R) {
                const float* Mr = wf ? sMt : sMp;
                for (int m = 0; m < Md; ++m) acc += sdZ[h * Md + m] * Mr[n * MP + m];
            } else {
                const int j = h - R;
                for (int m = 0; m < Md; ++m) {
                    float oth = 1.f;
                    for (int j2 = 0; j2 < Wh; ++j2)
                        if (j2 != j) oth *= (1.0f - sWt[(R + j2) * N + n] * sU[d.oE + j2 * Md + m]);
                    const float g = sG[n * MP + m];
                    const float Tj = g * sMp[n * MP + m] * oth;
                    acc += -sU[d.oE + j * Md + m] * Tj + sU[d.oA + j * Md + m] * g;
                }
            }
            dwt = acc;
            wv = sWv[tid]; wt = sWt[tid]; wc = sWc[tid]; wp = sWp[tid];
            gam = sU[d.oY + h]; gate = sU[d.oG + h];
            pw = powf(wv, gam);
            sWg[tid] = gate * wc + (1.0f - gate) * wp;
            rv[0] = pw; rv[1] = dwt * wt;
        }
        red_write(rv, 2, DQR1);
        __syncthreads();

        // ------------------------------------------------ R2: sharpen backward, shift-weight sums
        float dpw = 0.f, dwv = 0.f;
        if (tid < H * Md) {        // normalised keys (needed from R4 on); smooth cosine: the keys as they are
            const int h = tid / Md, m = tid - h * Md;
            const float kh = SMOOTH ? sU[d.oK + tid] : sU[d.oK + tid] * sKinv[h];
            sKhat[tid] = kh;
            sKs[tid] = SMOOTH ? kh : kh * sCinv[m];
        }
        if (hn) {
            const float den = red_read(hh, DQR1) + 1e-3f;
            const float s2 = red_read(hh, DQR1 + 1);
            dpw = (dwt - s2) / den;
            dwv = (wv > 0.f) ? dpw * gam * pw / wv : 0.f;
            sDwv[tid] = dwv;
            rv[0] = (wv > 0.f) ? dpw * pw * logf(wv) : 0.f;        // d gamma
            const int start = -((SS + 1) >> 1);
#pragma unroll
            for (int j = 0; j < DNQ - 1; ++j) {
                if (j < SS) {
                    int src = nn + start + j; src = (src % N + N) % N;
                    rv[1 + j] = dwv * sWg[hh * N + src];            // d shift_j
                }
            }
        }
        red_write(rv, 1 + SS, DQR2);
        __syncthreads();

        // ------------------------------------------------ R3: shift + gate backward
        float dwg = 0.f, dwc = 0.f;
        float Sgam = 0.f, Ssw[DNQ - 1];
        if (hn) {
            Sgam = red_read(hh, DQR2);
#pragma unroll
            for (int j = 0; j < DNQ - 1; ++j) Ssw[j] = (j < SS) ? red_read(hh, DQR2 + 1 + j) : 0.f;
            const int start = -((SS + 1) >> 1);
            for (int j = 0; j < SS; ++j) {
                int src = nn - (start + j); src = (src % N + N) % N;
                dwg += sSw[hh * SS + j] * sDwv[hh * N + src];
            }
            sdW[tid] = (1.0f - gate) * dwg;                         // carried d(w_{t-1})
            dwc = gate * dwg;
            rv[0] = dwg * (wc - wp);                                // d g
            rv[1] = wc * dwc;                                       // softmax backward inner product
        }
        red_write(rv, 2, DQR3);
        __syncthreads();

        // ------------------------------------------------ R4: content softmax backward
        float Sg = 0.f, dv = 0.f;
        if (hn) {
            Sg = red_read(hh, DQR3);
            const float Bs = red_read(hh, DQR3 + 1);
            dv = wc * (dwc - Bs);
            float sim = 0.f;
            for (int m = 0; m < Md; ++m) sim += sKs[hh * Md + m] * sMp[nn * MP + m];
            if constexpr (SMOOTH) {
                // sim = dot / den, den = |M[n]||k| + 1e-3:  d dot = a = dsim / den,  d den = b = -dsim sim / den.  sDsim keeps a
                // (B7 and the key sums below read it where they read dsim as coded); b |k| goes to the row-norm term of d M_prev
                // (sDwv is free: its readers passed R3's barrier) and b |M[n]|, summed over the slots, to the norm term of d k
                const float rn = sRn[nn], kn = sKinv[hh], den = rn * kn + 1e-3f;
                sim = sim / den;
                const float da = dv * sU[d.oB + hh] / den, db = -da * sim;
                rv[0] = dv * sim;                                   // d beta
                sDsim[tid] = da;
                sDwv[tid] = db * kn;
                rv[1] = db * rn;
            } else {
                rv[0] = dv * sim;                                   // d beta
                sDsim[tid] = dv * sU[d.oB + hh];
            }
        }
        red_write(rv, SMOOTH ? 2 : 1, DQR4);
        __syncthreads();
        if constexpr (SMOOTH) {
            if (tid < N) {         // row-norm term: d M_prev[n][:] += M_prev[n][:] * (sum_h b[h][n] |k_h|) / |M[n]|, 0 at a zero row
                float s = 0.f;
                for (int h = 0; h < H; ++h) s += sDwv[h * N + tid];
                const float rn = sRn[tid];
                sRc[tid] = (rn > 0.f) ? s / rn : 0.f;
            }
        }
        if (hn && nn == 0) {       // per-head scalar controls -> raw gradients
            const int h = hh;
            const float beta = sU[d.oB + h];
            sDU[d.oB + h] = red_read(h, DQR4) * (1.0f - expf(-beta));                 // softplus' = 1 - exp(-softplus)
            sDU[d.oG + h] = Sg * gate * (1.0f - gate);
            sDU[d.oY + h] = Sgam * (1.0f - expf(-(gam - 1.0f)));
            float dot = 0.f;
#pragma unroll
            for (int j = 0; j < DNQ - 1; ++j) if (j < SS) dot += sSw[h * SS + j] * Ssw[j];
#pragma unroll
            for (int j = 0; j < DNQ - 1; ++j) if (j < SS) sDU[d.oS + h * SS + j] = sSw[h * SS + j] * (Ssw[j] - dot);
        }

        // ------------------------------------------------ B7: dMhat = sum_h dsim khat; reductions over slots (keys, erase, add)
        for (int idx = tid; idx < NMd; idx += T) {
            const int n = idx / Md, m = idx - n * Md;
            float dmh = 0.f;
            for (int h = 0; h < H; ++h) dmh += sDsim[h * N + n] * sKhat[h * Md + m];
            sDmh[n * MP + m] = dmh;
        }
        if (tid < nslP * nout) {
            const int o = tid % nout, sl = tid / nout;
            const int n0 = sl * nperP, n1 = min(N, n0 + nperP);
            float s = 0.f;
            if (o < H * Md) {                                  // sum_n dsim[h][n] * M_prev[n][m]
                const int h = o / Md, m = o - h * Md;
                float s1 = 0.f, s2 = 0.f, s3 = 0.f;
                int n = n0;
                for (; n + 3 < n1; n += 4) {
                    s += sDsim[h * N + n] * sMp[n * MP + m];
                    s1 += sDsim[h * N + n + 1] * sMp[(n + 1) * MP + m];
                    s2 += sDsim[h * N + n + 2] * sMp[(n + 2) * MP + m];
                    s3 += sDsim[h * N + n + 3] * sMp[(n + 3) * MP + m];
                }
                for (; n < n1; ++n) s += sDsim[h * N + n] * sMp[n * MP + m];
                s = (s + s1) + (s2 + s3);
            } else {
                const int o2 = o - H * Md;
                const int which = o2 / (Wh * Md);              // 0: erase, 1: add
                const int jm = o2 - which * Wh * Md;
                const int j = jm / Md, m = jm - j * Md;
                float sa = 0.f, sb = 0.f;
                for (int n = n0; n < n1; ++n) {
                    const float ww = sWt[(R + j) * N + n];
                    const float g = sG[n * MP + m];
                    float term;
                    if (which == 0) {
                        float oth = 1.f;
                        for (int j2 = 0; j2 < Wh; ++j2)
                            if (j2 != j) oth *= (1.0f - sWt[(R + j2) * N + n] * sU[d.oE + j2 * Md + m]);
                        term = -ww * g * sMp[n * MP + m] * oth;
                    } else {
                        term = ww * g;
                    }
                    if ((n - n0) & 1) sb += term; else sa += term;
                }
                s = sa + sb;
            }
            sPart[sl * nout + o] = s;
        }
        __syncthreads();
        // column-norm term: s_m = sum_n dMhat[n][m] * M_prev[n][m], one wave_sum per column (waves stride over m)
        if constexpr (!SMOOTH)
        for (int m = (tid >> 6); m < Md; m += (T >> 6)) {
            float s = 0.f;
            for (int n = lane; n < N; n += 64) s += sDmh[n * MP + m] * sMp[n * MP + m];
            s = wave_sum(s);
            if (lane == 0) {
                const float ci = sCinv[m];
                sC2[m] = (sCss[m] > 1e-12f) ? -ci * ci * ci * s : 0.f;
            }
        }
        if (tid < nout) {
            float s = 0.f;
            for (int sl = 0; sl < nslP; ++sl) s += sPart[sl * nout + tid];
            if (tid < H * Md) {
                sDkhat[tid] = SMOOTH ? s : s * sCinv[tid % Md];
            } else {
                const int o2 = tid - H * Md;
                const int which = o2 / (Wh * Md);
                const int jm = o2 - which * Wh * Md;
                if (which == 0) { const float e = sU[d.oE + jm]; sDU[d.oE + jm] = s * e * (1.0f - e); }
                else { const float av = sU[d.oA + jm]; sDU[d.oA + jm] = s * (1.0f - av * av); }
            }
        }
        __syncthreads();
        if (tid < H * Md) {
            const int h = tid / Md;
            if constexpr (SMOOTH) {                                 // d k = sum_n a M_prev[n] + k / |k| * sum_n b |M[n]|, 0 through |k| = 0
                const float kn = sKinv[h], kv = sU[d.oK + tid];
                const float dk = sDkhat[tid] + ((kn > 0.f) ? kv / kn * red_read(h, DQR4 + 1) : 0.f);
                sDU[d.oK + tid] = dk * (1.0f - kv * kv);
            } else {
                float dot = 0.f;
                for (int m = 0; m < Md; ++m) dot += sDkhat[h * Md + m] * sU[d.oK + h * Md + m];
                const float ki = sKinv[h];
                const float ck = (sKss[h] > 1e-12f) ? -ki * ki * ki * dot : 0.f;
                const float kv = sU[d.oK + tid];
                const float dk = ki * sDkhat[tid] + kv * ck;
                sDU[d.oK + tid] = dk * (1.0f - kv * kv);
            }
        }
        for (int idx = tid; idx < NMd; idx += T) {
            const int n = idx / Md, m = idx - n * Md, ai = n * MP + m;
            if constexpr (SMOOTH) sdM[ai] += sDmh[ai] + sMp[ai] * sRc[n];
            else sdM[ai] += sCinv[m] * sDmh[ai] + sMp[ai] * sC2[m];
        }
        __syncthreads();
        if (tid < PP) a.du[bt * PP + tid] = sDU[tid];

        // ------------------------------------------------ B9: dU . Wa^T (partials; the top layer's B10 adds its carried dh)
        if (tid < nslH * hg4) {
            const int cg = tid % hg4, sl = tid / hg4;
            const int c0 = sl * nperH, c1 = min(PP, c0 + nperH);
            sPart4[sl * hg4 + cg] = ntk_stream_matvec<(MAXT > 768 ? 2 : 4)>(reinterpret_cast<const f32x4*>(a.WaT) + cg, hg4, sDU, c0, c1, PP - 1);
        }
        __syncthreads();

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
            if (l == NL - 1 && t > 0) commit();  // next (earlier) step's records: every reader of the old ones has passed a barrier
            __syncthreads();
        }
    }

    // ---- gradient of the initial state
    for (int i = tid; i < NMd; i += T) a.dM0[(size_t)b * NMd + i] = sdM[(i / Md) * MP + (i % Md)];
    for (int i = tid; i < HN; i += T) a.dw0[(size_t)b * HN + i] = sdW[i];
    for (int i = tid; i < RM; i += T) a.dread0[(size_t)b * RM + i] = sdZ[i];
    for (int i = tid; i < NL * hid; i += T) {
        const int l = i / hid, j = i - l * hid;
        a.dcs0[(size_t)b * cs_ld + 2 * hid * l + j] = sdC[i];
        a.dcs0[(size_t)b * cs_ld + 2 * hid * l + hid + j] = sdZ[RM + i];
    }
}

// ------------------------------------------------------------------------------------------------ host side
int ntm_validate_dims(const NtmDims& d, const char* who);          // ntm_seq_fwd.hip

// workgroup sizes: the single-layer kernels' rules (ntm_pick_threads / ntk_ntm_seq_bwd); the BPTT also covers the 2*hid
// columns of a layer's input gradient
static int ntm_deep_fwd_threads(const NtmDims& d) {
    int want = ntm_imax(d.H * d.N, 3 * d.hid);
    want = ntm_imax(want, d.hid + ntm_imax(d.Md, 4));
    want = ntm_imax(want, d.PP + d.Md);
    want = ntm_imax(want, d.H * d.Md + d.H + 1);
    want = ntm_imax(want, ((d.hid + 63) / 64 + 1) * 64);
    want = ntm_imax(want, (d.H + 1) * 64);
    want = ((want + 63) / 64) * 64;
    return want > 1024 ? 1024 : want;
}

static int ntm_deep_bwd_threads(const NtmDims& d) {
    int T = ntm_imax(d.H * d.N, 3 * d.hid);
    T = ntm_imax(T, d.PP);
    T = ntm_imax(T, d.K);
    T = ntm_imax(T, 2 * d.hid);
    T = ntm_imax(T, d.H * d.Md + d.Md + 2 * d.Wh * d.Md);
    return ((T + 63) / 64) * 64;
}

struct NtmDeepPlan {
    int Tf, Tb;
    NtmLds Lf;
    NtmDeepBwdLds Lb;
    size_t lds_f, lds_b;
};

// the instantiation a workgroup size takes (both deep kernels): the launchers and ntk_ntm_seq_deep_plan read it here
static inline int ntm_deep_kernel_id(int T) { return T <= 768 ? NTK_NTM_DEEP_768 : NTK_NTM_DEEP_1024; }

// every limit of the two deep kernels, host arithmetic only
static int ntm_deep_plan(const NtmDims& d, const NtmDeepShape& s, NtmDeepPlan& p, const char* who) {
    NTK_REQUIRE(s.L >= 2, NTK_ERR_BAD_SHAPE, "%s: L=%d layers (the deep kernels take L >= 2; one layer is ntk_ntm_seq_fwd/bwd)", who, s.L);
    int rc = ntm_validate_dims(d, who);
    if (rc != NTK_OK) return rc;
    NTK_REQUIRE((d.hid % 4) == 0, NTK_ERR_UNSUPPORTED, "%s: hidden=%d must be a multiple of 4", who, d.hid);
    NTK_REQUIRE(d.SS + 1 <= DNQ, NTK_ERR_UNSUPPORTED, "%s: shift space %d too wide", who, d.SS);
    p.Tf = ntm_deep_fwd_threads(d);
    NTK_REQUIRE(p.Tf >= d.N, NTK_ERR_UNSUPPORTED, "%s: mem_size %d exceeds the workgroup", who, d.N);
    p.Tb = ntm_deep_bwd_threads(d);
    NTK_REQUIRE(p.Tb <= 1024 && d.H * d.N <= 1024 && d.N * d.Md <= DMAXM * p.Tb, NTK_ERR_UNSUPPORTED,
                "%s: heads*mem_size=%d (max 1024) / mem_size*mem_dim=%d exceed one workgroup", who, d.H * d.N, d.N * d.Md);
    ntm_deep_fwd_lds(d, s.L, p.Tf, p.Lf);
    ntm_deep_bwd_lds(d, s, p.Tb, ntm_align4(d.hid), p.Lb);
    p.lds_f = (size_t)p.Lf.total * sizeof(float);
    p.lds_b = (size_t)p.Lb.total * sizeof(float);
    NTK_REQUIRE(p.lds_f <= 160 * 1024 && p.lds_b <= 160 * 1024, NTK_ERR_UNSUPPORTED,
                "%s: %d layers of hidden=%d need %zu / %zu B of LDS (forward / BPTT; > 160 KiB)", who, s.L, d.hid, p.lds_f, p.lds_b);
    return NTK_OK;
}

extern "C" int ntk_ntm_seq_deep_supported(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L) {
    NtmDims d;
    ntm_fill_dims(d, B, 1, N, Md, R, Wh, hid, shift_range, O, 0);
    NtmDeepShape s;
    ntm_deep_shape(s, 1, R * Md, hid, L);
    NtmDeepPlan p;
    return ntm_deep_plan(d, s, p, "ntk_ntm_seq_deep_supported") == NTK_OK ? 1 : 0;
}

extern "C" int ntk_ntm_seq_deep_plan_sim(int B, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int L, int write_first,
                                         int similarity, int* fwd_kernel, int* fwd_threads, int* bwd_kernel, int* bwd_threads) {
    NTM_REQUIRE_SIMILARITY(similarity, "ntk_ntm_seq_deep_plan");
    NtmDims d;
    ntm_fill_dims(d, B, 1, N, Md, R, Wh, hid, shift_range, O, write_first, similarity);
    NtmDeepShape s;
    ntm_deep_shape(s, 1, R * Md, hid, L);
    NtmDeepPlan p;
    const bool ok = ntm_deep_plan(d, s, p, "ntk_ntm_seq_deep_plan") == NTK_OK;
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
    NtmDeepShape s;
    ntm_deep_shape(s, D, R * Md, hid, L);
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
    NtmDeepShape s;
    ntm_deep_shape(s, D, R * Md, hid, L);
    const size_t n = ntm_deep_nwx0(s) + ntm_deep_nwf(s) + ntm_deep_nwb(s);
    const int blocks = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    ntm_deep_pack_kernel<<<blocks, 256, 0, (hipStream_t)stream>>>(s, lowerT, top_WxT, top_Wr, Wx0, Wf, Wb);
    NTK_CHECK_LAUNCH("ntk_ntm_seq_deep_pack");
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
    const char* who = "ntk_ntm_seq_fwd_deep";
    NTM_REQUIRE_SIMILARITY(similarity, who);
    NtmFwdArgs a = {};
    ntm_fill_dims(a.d, B, S, N, Md, R, Wh, hid, shift_range, O, write_first, similarity);
    NTK_REQUIRE(D >= 1, NTK_ERR_BAD_SHAPE, "%s: D=%d", who, D);
    NtmDeepFwdArgs dp = {};
    ntm_deep_shape(dp.s, D, R * Md, hid, L);
    NtmDeepPlan p;
    int rc = ntm_deep_plan(a.d, dp.s, p, who);
    if (rc != NTK_OK) return rc;
    NTK_REQUIRE(xproj && Wf && Wa && M0 && w0 && read0 && cs0 && logits && M_out && w_out && read_out && cs_out,
                NTK_ERR_BAD_PTR, "%s: null pointer", who);
    NTK_REQUIRE(ntk_aligned16(xproj) && ntk_aligned16(Wf) && ntk_aligned16(Wa) && (!st_gates || ntk_aligned16(st_gates)) &&
                    (!st_lgates || ntk_aligned16(st_lgates)),
                NTK_ERR_BAD_PTR, "%s: xproj/Wf/Wa/st_gates/st_lgates must be 16-byte aligned", who);
    NTK_REQUIRE(!st_gates == !st_c, NTK_ERR_BAD_PTR, "%s: st_gates and st_c go together", who);
    NTK_REQUIRE(!st_buf0 || X, NTK_ERR_BAD_PTR, "%s: the st_buf0 record needs X", who);
    a.xproj = xproj; a.Wr = nullptr; a.Wa = Wa; a.M0 = M0; a.w0 = w0; a.read0 = read0; a.cs0 = nullptr;
    a.logits = logits; a.outputs = outputs; a.M_out = M_out; a.w_out = w_out; a.read_out = read_out; a.cs_out = nullptr;
    a.st_z = st_z; a.st_gates = st_gates; a.st_c = st_c; a.st_h = st_h; a.st_u = st_u;
    a.st_wc = st_wc; a.st_wv = st_wv; a.st_w = st_w; a.st_M = st_M; a.st_read = st_read;
    dp.X = X; dp.Wf = Wf; dp.cs0 = cs0; dp.cs_out = cs_out;
    dp.st_xtop = st_xtop; dp.st_buf0 = st_buf0; dp.st_bufk = (L > 2) ? st_bufk : nullptr; dp.st_lgates = st_lgates; dp.st_lc = st_lc;
    {
        static NtkLdsAttrCache lds_cache;
        const void* const ks[] = {(const void*)ntm_seq_fwd_deep_kernel<768>, (const void*)ntm_seq_fwd_deep_kernel<1024>,
                                  (const void*)ntm_seq_fwd_deep_kernel<768, NTM_SIM_SMOOTH_COSINE>,
                                  (const void*)ntm_seq_fwd_deep_kernel<1024, NTM_SIM_SMOOTH_COSINE>};
        const int rc_lds = ntk_raise_lds_limit(lds_cache, ks, 4, who);
        if (rc_lds != NTK_OK) return rc_lds;
    }
    if (similarity == NTM_SIM_SMOOTH_COSINE) {
        if (ntm_deep_kernel_id(p.Tf) == NTK_NTM_DEEP_768) ntm_seq_fwd_deep_kernel<768, NTM_SIM_SMOOTH_COSINE><<<B, p.Tf, p.lds_f, (hipStream_t)stream>>>(a, dp, p.Lf);
        else ntm_seq_fwd_deep_kernel<1024, NTM_SIM_SMOOTH_COSINE><<<B, p.Tf, p.lds_f, (hipStream_t)stream>>>(a, dp, p.Lf);
    } else
    if (ntm_deep_kernel_id(p.Tf) == NTK_NTM_DEEP_768) ntm_seq_fwd_deep_kernel<768><<<B, p.Tf, p.lds_f, (hipStream_t)stream>>>(a, dp, p.Lf);
    else ntm_seq_fwd_deep_kernel<1024><<<B, p.Tf, p.lds_f, (hipStream_t)stream>>>(a, dp, p.Lf);
    NTK_CHECK_LAUNCH(who);
    return NTK_OK;
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
    const char* who = "ntk_ntm_seq_bwd_deep";
    NTM_REQUIRE_SIMILARITY(similarity, who);
    NtmDeepBwdArgs a = {};
    ntm_fill_dims(a.d, B, S, N, Md, R, Wh, hid, shift_range, O, write_first, similarity);
    ntm_deep_shape(a.s, 1, R * Md, hid, L);
    NtmDeepPlan p;
    int rc = ntm_deep_plan(a.d, a.s, p, who);
    if (rc != NTK_OK) return rc;
    NTK_REQUIRE(ldhT >= hid && (ldhT % 4) == 0, NTK_ERR_BAD_SHAPE, "%s: ldhT=%d (hid=%d)", who, ldhT, hid);
    NTK_REQUIRE(Wb && WaT && M0 && w0 && cs0 && st_gates && st_c && st_u && st_wc && st_wv && st_w && st_M && st_lgates && st_lc &&
                    dlogits && dgates && dpre && du && dM0 && dw0 && dread0 && dcs0,
                NTK_ERR_BAD_PTR, "%s: null pointer", who);
    NTK_REQUIRE(ntk_aligned16(Wb) && ntk_aligned16(WaT) && ntk_aligned16(st_gates) && ntk_aligned16(st_lgates) && ntk_aligned16(dgates),
                NTK_ERR_BAD_PTR, "%s: Wb/WaT/st_gates/st_lgates/dgates must be 16-byte aligned", who);
    if (ldhT != ntm_align4(hid)) ntm_deep_bwd_lds(a.d, a.s, p.Tb, ldhT, p.Lb);
    const size_t lds_bytes = (size_t)p.Lb.total * sizeof(float);
    NTK_REQUIRE(lds_bytes <= 160 * 1024, NTK_ERR_UNSUPPORTED, "%s: needs %zu B of LDS (> 160 KiB)", who, lds_bytes);
    a.Wb = Wb; a.WaT = WaT; a.ldhT = ldhT; a.M0 = M0; a.w0 = w0; a.cs0 = cs0;
    a.st_gates = st_gates; a.st_c = st_c; a.st_u = st_u; a.st_wc = st_wc; a.st_wv = st_wv; a.st_w = st_w; a.st_M = st_M;
    a.st_lgates = st_lgates; a.st_lc = st_lc; a.dlogits = dlogits;
    a.dM_fin = dM_fin; a.dw_fin = dw_fin; a.dread_fin = dread_fin; a.dcs_fin = dcs_fin;
    a.dgates = dgates; a.dpre = dpre; a.du = du; a.dM0 = dM0; a.dw0 = dw0; a.dread0 = dread0; a.dcs0 = dcs0;
    {
        static NtkLdsAttrCache lds_cache;
        const void* const ks[] = {(const void*)ntm_seq_bwd_deep_kernel<768>, (const void*)ntm_seq_bwd_deep_kernel<1024>,
                                  (const void*)ntm_seq_bwd_deep_kernel<768, NTM_SIM_SMOOTH_COSINE>,
                                  (const void*)ntm_seq_bwd_deep_kernel<1024, NTM_SIM_SMOOTH_COSINE>};
        const int rc_lds = ntk_raise_lds_limit(lds_cache, ks, 4, who);
        if (rc_lds != NTK_OK) return rc_lds;
    }
    if (similarity == NTM_SIM_SMOOTH_COSINE) {
        if (ntm_deep_kernel_id(p.Tb) == NTK_NTM_DEEP_768) ntm_seq_bwd_deep_kernel<768, NTM_SIM_SMOOTH_COSINE><<<B, p.Tb, lds_bytes, (hipStream_t)stream>>>(a, p.Lb);
        else ntm_seq_bwd_deep_kernel<1024, NTM_SIM_SMOOTH_COSINE><<<B, p.Tb, lds_bytes, (hipStream_t)stream>>>(a, p.Lb);
    } else
    if (ntm_deep_kernel_id(p.Tb) == NTK_NTM_DEEP_768) ntm_seq_bwd_deep_kernel<768><<<B, p.Tb, lds_bytes, (hipStream_t)stream>>>(a, p.Lb);
    else ntm_seq_bwd_deep_kernel<1024><<<B, p.Tb, lds_bytes, (hipStream_t)stream>>>(a, p.Lb);
    NTK_CHECK_LAUNCH(who);
    return NTK_OK;
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
    return ntk_ntm_seq_fwd_deep_sim(B, S, N, Md, R, Wh, hid, shift_range, O, L, write_first, NTM_SIM_AS_CODED, D, X, xproj, Wf, Wa,
                                    M0, w0, read0, cs0, logits, outputs, M_out, w_out, read_out, cs_out, st_z, st_gates, st_c, st_h,
                                    st_u, st_wc, st_wv, st_w, st_M, st_read, st_xtop, st_buf0, st_bufk, st_lgates, st_lc, stream);
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
    return ntk_ntm_seq_bwd_deep_sim(B, S, N, Md, R, Wh, hid, shift_range, O, L, write_first, NTM_SIM_AS_CODED, Wb, WaT, ldhT, M0, w0, cs0,
                                    st_gates, st_c, st_u, st_wc, st_wv, st_w, st_M, st_lgates, st_lc, dlogits, dM_fin, dw_fin,
                                    dread_fin, dcs_fin, dgates, dpre, du, dM0, dw0, dread0, dcs0, stream);
}
