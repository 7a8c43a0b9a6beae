// The phases every NTM sequence kernel runs, once: control layout, content addressing, memory write and read of the forward
// step (P2's normaliser, P3 .. P8) and the head / memory / unpack part of the BPTT step (X1 .. B9) with its record prefetch and
// per-head reductions.  Device code only, included by ntm_seq_fwd.hip, ntm_seq_fwd_ws.hip, ntm_seq_bwd.hip and
// ntm_seq_deep.hip; the phase comments and the reference's line numbers are those of ntm_seq_fwd.hip / ntm_seq_bwd.hip.
//
// Everything is a __forceinline__ function (template) over plain values: a kernel builds one by-value state struct (LDS
// pointers, dimensions, work decomposition) before its step loop and hands it to every phase; at the fixed-dims instantiations
// the dimensions are compile-time constants and fold after inlining, as they did in place.  SMOOTH, FIX, the shift-tap bound
// and the stream batch depth stay template parameters.  The forward phases contain no workgroup barrier: the kernels keep
// theirs between the calls.  The BPTT step takes its nine barriers as a callable, so a kernel states what a barrier is
// (a stamped one in ntm_seq_bwd.hip, a plain one in ntm_seq_deep.hip) and the sequence X1 | X2 | R2 | R3 | R4 | B7 | B8a | B8b | B9
// reads top to bottom in ntm_bwd_heads_step.
#pragma once
#include "ntm_seq_args.h"

// ------------------------------------------------------------------------------------------------ control layout
// offsets of k, beta, g, shift, gamma, erase, add inside the unpacked control vector (ntm_cell.py:128-130), the padded widths
struct NtmCtl {
    int O, oK, oB, oG, oS, oY, oE, oA, P, PP, ldz, ldh, write_first;
};

__device__ __forceinline__ NtmCtl ntm_ctl(int Md, int R, int Wh, int hid, int SS, int O, int write_first) {
    const int H = R + Wh, K = R * Md + hid;
    NtmCtl d;
    d.O = O;
    d.oK = 0; d.oB = H * Md; d.oG = d.oB + H; d.oS = d.oG + H; d.oY = d.oS + H * SS; d.oE = d.oY + H;
    d.oA = d.oE + Wh * Md; d.P = d.oA + Wh * Md;
    d.PP = (d.P + d.O + 3) & ~3; d.ldz = (K + 1 + 3) & ~3; d.ldh = (hid + 1 + 3) & ~3;
    d.write_first = write_first;
    return d;
}

// ------------------------------------------------------------------------------------------------ forward
// T = the threads that run the phases (the compute threads of the wave-specialised kernel); sH = the h that drives the unpack
struct NtmFwdSt {
    int T, N, Md, MP, R, Wh, H, hid, SS, RM;
    int nslB, kperB;       // hidden-unit slices of the unpack product
    int nslR, nperR;       // N-slices of the read product
    float *sPart, *sM, *sW, *sWg, *sZ, *sU, *sKs, *sPw;
    float* sCn;            // [Md] inverse column norms of M (as coded) / [N] row norms of M (smooth cosine)
    const float* sH;
};

__device__ __forceinline__ NtmFwdSt ntm_fwd_state(float* smem, const NtmLds& L, int T, int N, int Md, int R, int Wh, int hid,
                                                  int SS, int PP, int h_at) {
    NtmFwdSt c;
    c.T = T; c.N = N; c.Md = Md; c.MP = Md | 1; c.R = R; c.Wh = Wh; c.H = R + Wh; c.hid = hid; c.SS = SS; c.RM = R * Md;
    c.nslB = min(max(1, T / (PP >> 2)), hid);
    c.kperB = (hid + c.nslB - 1) / c.nslB;
    c.nslR = min(max(1, T / c.RM), N);
    c.nperR = (N + c.nslR - 1) / c.nslR;
    c.sPart = smem + L.part; c.sM = smem + L.M; c.sW = smem + L.W; c.sWg = smem + L.Wg; c.sZ = smem + L.Z; c.sU = smem + L.U;
    c.sKs = smem + L.Ks; c.sCn = smem + L.Cn; c.sPw = smem + L.Pw;
    c.sH = c.sZ + h_at;
    return c;
}

// P2, beside the LSTM cell: the waves not running it take the normaliser of the content addressing.  As coded they l2-normalise
// the feature columns of M over the slot axis (tf.nn.l2_normalize, ops.py:150, quirk Q1)
template <bool SMOOTH>
__device__ __forceinline__ void ntm_fwd_mem_norms(const NtmFwdSt& c, int tid) {
    const int N = c.N, Md = c.Md, MP = c.MP, lane = tid & 63, wave = tid >> 6, nwaves = c.T >> 6;
    const int w0 = (c.hid + 63) >> 6;
    if constexpr (SMOOTH) {
        // smooth cosine: the row norms |M[n]|, a lane per slot (rows are MP = Md | 1 floats apart: no bank conflict), no clamp
        if (wave >= w0) {
            for (int n = (wave - w0) * 64 + lane; n < N; n += (nwaves - w0) * 64) {
                float s = 0.f;
                for (int m = 0; m < Md; ++m) { const float v = c.sM[n * MP + m]; s += v * v; }
                c.sCn[n] = sqrtf(s);
            }
        }
    } else
    if (wave >= w0) {
        for (int m = wave - w0; m < Md; m += nwaves - w0) {
            float s = 0.f;
            for (int n = lane; n < N; n += 64) { const float v = c.sM[n * MP + m]; s += v * v; }
            s = wave_sum(s);
            if (lane == 0) c.sCn[m] = 1.0f / sqrtf(fmaxf(s, 1e-12f));
        }
    }
}

// P3: unpack / output partials, h' x Wa[hid][PP]; NB = row batches in flight
// (explicit two-batch stream: the compiler otherwise keeps ONE load in flight, see common.h)
template <int NB>
__device__ __forceinline__ void ntm_fwd_unpack_partials(const NtmFwdSt& c, const NtmCtl& d, const f32x4* Wa4, int tid) {
    const int ncg = d.PP >> 2;                        // float4 column groups of the unpack product
    if (tid < c.nslB * ncg) {
        const int cg = tid % ncg, ks = tid / ncg;
        const int k0 = ks * c.kperB, k1 = min(c.hid, k0 + c.kperB);
        reinterpret_cast<f32x4*>(c.sPart)[ks * ncg + cg] = ntk_stream_matvec<NB>(Wa4 + cg, ncg, c.sH, k0, k1, c.hid);
    }
}

// P4: control activations
__device__ __forceinline__ void ntm_fwd_controls(const NtmFwdSt& c, const NtmCtl& d, const NtmFwdArgs& a, int tid, size_t bt) {
    const int hid = c.hid, nslB = c.nslB, PP = d.PP;
    if (tid < PP) {
        float v = a.Wa[(size_t)hid * PP + tid];
        for (int ks = 0; ks < nslB; ++ks) v += c.sPart[ks * PP + tid];
        float r = v;
        if (tid < d.oB) r = ntm_tanh(v);                       // k      :133
        else if (tid < d.oG) r = ntm_softplus(v);              // beta   :140
        else if (tid < d.oS) r = ntm_sigmoid(v);               // g      :151
        else if (tid < d.oY) r = v;                            // shift logits (softmax per head below)
        else if (tid < d.oE) r = ntm_softplus(v) + 1.0f;       // gamma  :169-170
        else if (tid < d.oA) r = ntm_sigmoid(v);               // erase  :193
        else if (tid < d.P) r = ntm_tanh(v);                   // add    :195
        c.sU[tid] = r;
        if (a.st_u) a.st_u[bt * PP + tid] = r;
        if (tid >= d.P && tid < d.P + d.O) a.logits[bt * d.O + (tid - d.P)] = v;
    }
}

// P5-P7, the wave of head h: key scaling, similarity (Q1), beta, softmax over N, gate, circular shift (Q2), sharpen (Q4).
// No workgroup barrier inside.  MAXSS = the shift taps held in registers (3 at fixed dims, NTM_MAX_SHIFT_TAPS otherwise)
template <bool SMOOTH, int MAXSS>
__device__ __forceinline__ void ntm_fwd_head_wave(const NtmFwdSt& c, const NtmCtl& d, const NtmFwdArgs& a, int h, int lane, size_t bt) {
    const int N = c.N, Md = c.Md, MP = c.MP, H = c.H, SS = c.SS;
    float kss = 0.f;
    for (int m = 0; m < Md; ++m) { const float kv = c.sU[d.oK + h * Md + m]; kss += kv * kv; }
    const float kn = sqrtf(kss);                           // |k|, smooth cosine only
    if constexpr (SMOOTH) {
        for (int m = lane; m < Md; m += 64) c.sKs[h * Md + m] = c.sU[d.oK + h * Md + m];
    } else {
        const float kinv = 1.0f / sqrtf(fmaxf(kss, 1e-12f));
        if (lane < Md) c.sKs[h * Md + lane] = c.sU[d.oK + h * Md + lane] * kinv * c.sCn[lane];
        for (int m = lane + 64; m < Md; m += 64) c.sKs[h * Md + m] = c.sU[d.oK + h * Md + m] * kinv * c.sCn[m];
    }
    const float beta = c.sU[d.oB + h], g = c.sU[d.oG + h], gamma = c.sU[d.oY + h];
    float swv[MAXSS];                                      // softmax of the shift logits (ntm_cell.py:161)
    {
        float mx = -INFINITY;
#pragma unroll
        for (int j = 0; j < MAXSS; ++j) if (j < SS) mx = fmaxf(mx, c.sU[d.oS + h * SS + j]);
        float sum = 0.f;
#pragma unroll
        for (int j = 0; j < MAXSS; ++j) { swv[j] = (j < SS) ? ntm_exp(c.sU[d.oS + h * SS + j] - mx) : 0.f; sum += swv[j]; }
#pragma unroll
        for (int j = 0; j < MAXSS; ++j) swv[j] = swv[j] / sum;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    float mxv = -INFINITY;
    for (int n = lane; n < N; n += 64) {
        float sim = 0.f;
        for (int m = 0; m < Md; ++m) sim += c.sKs[h * Md + m] * c.sM[n * MP + m];
        if constexpr (SMOOTH) sim = sim / (c.sCn[n] * kn + 1e-3f);
        const float v = sim * beta;
        c.sWg[h * N + n] = v;
        mxv = fmaxf(mxv, v);
    }
    mxv = wave_max(mxv);
    float sum = 0.f;
    for (int n = lane; n < N; n += 64) { const float e = ntm_exp(c.sWg[h * N + n] - mxv); c.sWg[h * N + n] = e; sum += e; }
    sum = wave_sum(sum);
    for (int n = lane; n < N; n += 64) {
        const float wc = c.sWg[h * N + n] / sum;
        if (a.st_wc) a.st_wc[(bt * H + h) * N + n] = wc;
        c.sWg[h * N + n] = wc * g + c.sW[h * N + n] * (1.0f - g);
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQ_REL, "wavefront");
    __builtin_amdgcn_wave_barrier();
    const int start = -((SS + 1) >> 1);                    // Py2 floor of -SS/2 (Q2): 3 -> -2
    float psum = 0.f;
    for (int n = lane; n < N; n += 64) {
        float wv = 0.f;
#pragma unroll
        for (int j = 0; j < MAXSS; ++j) {
            if (j < SS) {
                int src = n + start + j;
                src = (src % N + N) % N;
                wv += swv[j] * c.sWg[h * N + src];
            }
        }
        if (a.st_wv) a.st_wv[(bt * H + h) * N + n] = wv;
        const float pw = ntm_pow(wv, gamma);
        c.sPw[h * N + n] = pw;
        psum += pw;
    }
    psum = wave_sum(psum);
    for (int n = lane; n < N; n += 64) {
        const float w = c.sPw[h * N + n] / (psum + 1e-3f);
        c.sW[h * N + n] = w;
        if (a.st_w) a.st_w[(bt * H + h) * N + n] = w;
    }
}

// softmax of the output logits (one lane)
__device__ __forceinline__ void ntm_fwd_output_softmax(const NtmFwdSt& c, const NtmCtl& d, const NtmFwdArgs& a, size_t bt) {
    float mx = -INFINITY;
    for (int j = 0; j < d.O; ++j) mx = fmaxf(mx, c.sU[d.P + j]);
    float sum = 0.f;
    for (int j = 0; j < d.O; ++j) sum += expf(c.sU[d.P + j] - mx);
    for (int j = 0; j < d.O; ++j) a.outputs[bt * d.O + j] = expf(c.sU[d.P + j] - mx) / sum;
}

// P8: erase / add write
__device__ __forceinline__ void ntm_fwd_update_M(const NtmFwdSt& c, const NtmCtl& d, const NtmFwdArgs& a, int tid, size_t bt) {
    const int T = c.T, N = c.N, Md = c.Md, MP = c.MP, R = c.R, Wh = c.Wh;
    for (int idx = tid; idx < N * Md; idx += T) {
        const int n = idx / Md, m = idx - n * Md;
        float E = 1.f, A = 0.f;
        for (int j = 0; j < Wh; ++j) {
            const float ww = c.sW[(R + j) * N + n];
            E *= (1.0f - ww * c.sU[d.oE + j * Md + m]);
            A += ww * c.sU[d.oA + j * Md + m];
        }
        const float nm = c.sM[n * MP + m] * E + A;
        c.sM[n * MP + m] = nm;
        if (a.st_M) a.st_M[bt * N * Md + idx] = nm;
    }
}

// P8: read partials over N-slices, then their sums (a barrier between the two)
__device__ __forceinline__ void ntm_fwd_read_partials(const NtmFwdSt& c, int tid) {
    const int N = c.N, Md = c.Md, MP = c.MP, RM = c.RM, nslR = c.nslR, nperR = c.nperR;
    if (tid < nslR * RM) {
        const int o = tid % RM, sl = tid / RM;
        const int i = o / Md, m = o - i * Md;
        const int n0 = sl * nperR, n1 = min(N, n0 + nperR);
        float s0 = 0.f, s1 = 0.f;                 // two chains: the loop is bound by the add latency, not by LDS
        int n = n0;
        for (; n + 1 < n1; n += 2) {
            s0 += c.sW[i * N + n] * c.sM[n * MP + m];
            s1 += c.sW[i * N + n + 1] * c.sM[(n + 1) * MP + m];
        }
        if (n < n1) s0 += c.sW[i * N + n] * c.sM[n * MP + m];
        c.sPart[sl * RM + o] = s0 + s1;
    }
}

__device__ __forceinline__ void ntm_fwd_read_finish(const NtmFwdSt& c, const NtmFwdArgs& a, int tid, size_t bt) {
    const int RM = c.RM, nslR = c.nslR;
    if (tid < RM) {
        float s = 0.f;
        for (int sl = 0; sl < nslR; ++sl) s += c.sPart[sl * RM + tid];
        c.sZ[tid] = s;
        if (a.st_read) a.st_read[bt * RM + tid] = s;
    }
}

// ------------------------------------------------------------------------------------------------ BPTT
// T = the threads the step's work is laid out over (640 beside the stream waves of the wave-specialised form)
struct NtmBwdSt {
    int b, S, T, N, Md, MP, R, Wh, H, hid, SS, NW, NMd, HN, ldhT;
    int nout, nslP, nperP;         // B7: outputs (keys, erase, add) x N-slices
    int hg4, nslH, nperH;          // B9: float4 column groups of Wa^T x slices of its PP rows
    int nslC, nperC;               // X1: N-slices of the column sums
    float *sPart, *sdM, *sG, *sMp, *sMt, *sdW, *sWp, *sWt, *sWc, *sWv, *sWg, *sDwv, *sDsim, *sU, *sDU, *sDG, *sdZ, *sdC, *sGt, *sCt,
        *sCp, *sKhat, *sKs, *sKinv, *sKss, *sCinv, *sCss, *sC2, *sDkhat, *sSw, *sRed, *sDmh;
    const f32x4* sWaRes4;          // fixed dims: the resident rows of Wa^T, behind the state (+ the diagnostic words)
};

__device__ __forceinline__ NtmBwdSt ntm_bwd_state(float* smem, const NtmBwdLds& L, int b, int S, int T, int N, int Md, int R, int Wh,
                                                  int hid, int SS, int PP, int ldhT) {
    NtmBwdSt c;
    c.b = b; c.S = S; c.T = T; c.N = N; c.Md = Md; c.MP = Md | 1; c.R = R; c.Wh = Wh; c.H = R + Wh; c.hid = hid; c.SS = SS;
    c.NW = N >> 6; c.NMd = N * Md; c.HN = c.H * N; c.ldhT = ldhT;
    c.nout = c.H * Md + 2 * Wh * Md;
    c.nslP = min(max(1, T / c.nout), N);
    c.nperP = (N + c.nslP - 1) / c.nslP;
    c.hg4 = ldhT >> 2;
    c.nslH = max(1, T / c.hg4); c.nperH = (PP + c.nslH - 1) / c.nslH;
    c.nslC = max(1, T / Md); c.nperC = (N + c.nslC - 1) / c.nslC;
    c.sPart = smem + L.part;
    c.sdM = smem + L.dM;  c.sG = smem + L.G;  c.sMp = smem + L.Mp;  c.sMt = smem + L.Mt;
    c.sdW = smem + L.dW;  c.sWp = smem + L.Wp; c.sWt = smem + L.Wt; c.sWc = smem + L.Wc;
    c.sWv = smem + L.Wv;  c.sWg = smem + L.Wg; c.sDwv = smem + L.Dwv; c.sDsim = smem + L.Dsim;
    c.sU = smem + L.U;    c.sDU = smem + L.DU; c.sDG = smem + L.DG; c.sdZ = smem + L.dZ;
    c.sdC = smem + L.dC;  c.sGt = smem + L.Gt; c.sCt = smem + L.Ct; c.sCp = smem + L.Cp;
    c.sKhat = smem + L.Khat; c.sKs = smem + L.Ks; c.sKinv = smem + L.Kinv; c.sKss = smem + L.Kss;
    c.sCinv = smem + L.Cinv; c.sCss = smem + L.Css; c.sC2 = smem + L.C2; c.sDkhat = smem + L.Dkhat;
    c.sSw = smem + L.Sw;  c.sRed = smem + L.Red;  c.sDmh = smem + L.Dmh;
    c.sWaRes4 = reinterpret_cast<const f32x4*>(smem + L.total + 32);
    return c;
}

// thread roles: (head, slot) owner, active iff hh < H.  Derived from the opaque thread id inside every step
struct NtmBwdWho {
    int tid, lane, hh, nn, wi;
    bool hn;
};

__device__ __forceinline__ NtmBwdWho ntm_bwd_who(int tid, int N, int H) {
    NtmBwdWho w;
    w.tid = tid; w.lane = tid & 63;
    w.hh = tid / N; w.nn = tid - w.hh * N; w.hn = w.hh < H; w.wi = w.nn >> 6;
    return w;
}

// prefetch registers for one step's records (the top layer's and the heads')
struct NtmBwdRecs {
    float M[MAXM], Mt[MAXM], Wp, Wt, Wc, Wv, U, Ct, Cp, Dl;
    f32x4 G;
};

// c_init: the initial c of the (top) LSTM layer of this sequence, step 0's c_prev
template <class Args>
__device__ __forceinline__ void ntm_bwd_prefetch(const NtmBwdSt& c, const NtmCtl& d, const Args& a, const NtmBwdWho& w, NtmBwdRecs& p,
                                                 int t, const float* c_init) {
    const int b = c.b, S = c.S, T = c.T, NMd = c.NMd, HN = c.HN, hid = c.hid, PP = d.PP, tid = w.tid;
    const bool hn = w.hn, wf = d.write_first != 0;
    const size_t bt = (size_t)b * S + t;
    const float* Mp = (t > 0) ? a.st_M + (bt - 1) * NMd : a.M0 + (size_t)b * NMd;
#pragma unroll
    for (int q = 0; q < MAXM; ++q) {
        const int idx = tid + q * T;
        p.M[q] = (idx < NMd) ? Mp[idx] : 0.f;
        p.Mt[q] = (wf && idx < NMd) ? a.st_M[bt * NMd + idx] : 0.f;
    }
    if (hn) {
        p.Wp = (t > 0) ? a.st_w[(bt - 1) * HN + tid] : a.w0[(size_t)b * HN + tid];
        p.Wt = a.st_w[bt * HN + tid];
        p.Wc = a.st_wc[bt * HN + tid];
        p.Wv = a.st_wv[bt * HN + tid];
    }
    if (tid < PP) {
        p.U = a.st_u[bt * PP + tid];
        p.Dl = (tid >= d.P && tid < d.P + d.O) ? a.dlogits[bt * d.O + (tid - d.P)] : 0.f;
    }
    if (tid < hid) {
        p.G = reinterpret_cast<const f32x4*>(a.st_gates)[bt * hid + tid];
        p.Ct = a.st_c[bt * hid + tid];
        p.Cp = (t > 0) ? a.st_c[(bt - 1) * hid + tid] : c_init[tid];
    }
}

__device__ __forceinline__ void ntm_bwd_commit(const NtmBwdSt& c, const NtmCtl& d, const NtmBwdWho& w, const NtmBwdRecs& p) {
    const int T = c.T, NMd = c.NMd, Md = c.Md, MP = c.MP, hid = c.hid, PP = d.PP, tid = w.tid;
    const bool hn = w.hn, wf = d.write_first != 0;
#pragma unroll
    for (int q = 0; q < MAXM; ++q) {
        const int idx = tid + q * T;
        if (idx < NMd) {
            const int n = idx / Md, m = idx - n * Md;
            c.sMp[n * MP + m] = p.M[q];
            if (wf) c.sMt[n * MP + m] = p.Mt[q];
        }
    }
    if (hn) { c.sWp[tid] = p.Wp; c.sWt[tid] = p.Wt; c.sWc[tid] = p.Wc; c.sWv[tid] = p.Wv; }
    if (tid < PP) { c.sU[tid] = p.U; c.sDU[tid] = p.Dl; }
    if (tid < hid) { reinterpret_cast<f32x4*>(c.sGt)[tid] = p.G; c.sCt[tid] = p.Ct; c.sCp[tid] = p.Cp; }
}

// the carried gradients of M, w and read start from the (optional) gradient of the final state
template <class Args>
__device__ __forceinline__ void ntm_bwd_init_carried(const NtmBwdSt& c, const Args& a, int tid) {
    const int b = c.b, T = c.T, NMd = c.NMd, HN = c.HN, Md = c.Md, MP = c.MP, RM = c.R * c.Md;
    for (int i = tid; i < NMd; i += T)
        c.sdM[(i / Md) * MP + (i % Md)] = a.dM_fin ? a.dM_fin[(size_t)b * NMd + i] : 0.f;
    for (int i = tid; i < HN; i += T) c.sdW[i] = a.dw_fin ? a.dw_fin[(size_t)b * HN + i] : 0.f;
    for (int i = tid; i < RM; i += T) c.sdZ[i] = a.dread_fin ? a.dread_fin[(size_t)b * RM + i] : 0.f;
}

// per-head block reduction of nq values held by the (h, n) owner threads; NQS = reduction slots per head
template <int NQS>
__device__ __forceinline__ void ntm_red_write(const NtmBwdSt& c, const NtmBwdWho& w, const float (&v)[NQ], int nq, int base) {
#pragma unroll
    for (int q = 0; q < NQ; ++q) {
        if (q < nq) {
            const float s = wave_sum(w.hn ? v[q] : 0.f);
            if (w.hn && w.lane == 0) c.sRed[(w.hh * NQS + base + q) * c.NW + w.wi] = s;
        }
    }
}

template <int NQS>
__device__ __forceinline__ float ntm_red_read(const NtmBwdSt& c, int h, int q) {
    float s = 0.f;
    for (int w = 0; w < c.NW; ++w) s += c.sRed[(h * NQS + q) * c.NW + w];
    return s;
}

// X1 .. B9 of a BPTT step: from the carried gradients and the committed records of step t to the raw control gradients du_t,
// the carried dM / dw of step t - 1 and the partials of dU . Wa^T in sPart.  barrier(i) is the workgroup barrier that ends a
// phase (nine of them, i = 0 .. 8, each reached by every thread that calls this); stamp(i) marks a point inside a phase for the
// diagnostic build.  FIX (benchmark shape, write_first off) keeps its four-column X1, its DPP form of B7 and its resident rows of
// Wa^T in B9; MAXT picks the stream depth of the generic B9.
template <int MAXT, bool FIX, bool SMOOTH, class Args, class Barrier, class Stamp>
__device__ __forceinline__ void ntm_bwd_heads_step(const NtmBwdSt& c, const NtmCtl& d, const Args& a, const NtmBwdWho& w, size_t bt,
                                                   Barrier&& barrier, Stamp&& stamp) {
    constexpr int NQS = NQT + (SMOOTH ? 1 : 0);         // reduction slots per head
    const int T = c.T, N = c.N, Md = c.Md, MP = c.MP, R = c.R, Wh = c.Wh, H = c.H, SS = c.SS, NMd = c.NMd, PP = d.PP;
    const int nout = c.nout, nslP = c.nslP, nperP = c.nperP, hg4 = c.hg4, nslH = c.nslH, nperH = c.nperH, nslC = c.nslC, nperC = c.nperC;
    const int tid = w.tid, lane = w.lane, hh = w.hh, nn = w.nn;
    const bool hn = w.hn, wf = d.write_first != 0;
    float* const sPart = c.sPart; float* const sdM = c.sdM; float* const sG = c.sG; float* const sMp = c.sMp; float* const sMt = c.sMt;
    float* const sdW = c.sdW; float* const sWp = c.sWp; float* const sWt = c.sWt; float* const sWc = c.sWc; float* const sWv = c.sWv;
    float* const sWg = c.sWg; float* const sDwv = c.sDwv; float* const sDsim = c.sDsim; float* const sU = c.sU; float* const sDU = c.sDU;
    float* const sdZ = c.sdZ; float* const sKhat = c.sKhat; float* const sKs = c.sKs; float* const sKinv = c.sKinv; float* const sKss = c.sKss;
    float* const sCinv = c.sCinv; float* const sCss = c.sCss; float* const sC2 = c.sC2; float* const sDkhat = c.sDkhat;
    float* const sSw = c.sSw; float* const sDmh = c.sDmh;
    const f32x4* const sWaRes4 = c.sWaRes4;
    float* const sRn = sCinv; float* const sRc = sC2;  // smooth cosine: [N] row norms |M_prev[n]| and the row-norm coefficients where the [Md] column terms are
    f32x4* const sPart4 = reinterpret_cast<f32x4*>(sPart);

    // ------------------------------------------------ X1: memory-shaped elementwise + column norms + small vectors
    if constexpr (FIX) {
        // benchmark shape (write_first off): a thread = (slot n, four adjacent columns): the five head weights of the slot
        // are read once for four elements and d(read) comes in 16-byte reads: 29 LDS operations per thread instead of 52
        const int n = tid / 5, m0 = (tid - n * 5) * 4;
        float wt[5];
#pragma unroll
        for (int i = 0; i < 5; ++i) wt[i] = sWt[i * N + n];
        f32x4 dmr = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < 4; ++i) dmr += wt[i] * *reinterpret_cast<const f32x4*>(sdZ + i * Md + m0);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int ai = n * MP + m0 + e;
            const float dMt = sdM[ai];
            const float E = 1.0f - wt[4] * sU[d.oE + m0 + e];
            sG[ai] = dMt;
            sdM[ai] = dMt * E + dmr[e];
        }
    } else
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
    barrier(0);

    // ------------------------------------------------ X2: d(w_t) for every head; R1 sums
    float dwt = 0.f, pw = 0.f, wv = 0.f, wt = 0.f, wc = 0.f, wp = 0.f, gam = 1.f, gate = 0.f;
    float rv[NQ];
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
    ntm_red_write<NQS>(c, w, rv, 2, QR1);
    barrier(1);

    // ------------------------------------------------ R2: sharpen backward, shift-weight sums
    float dpw = 0.f, dwv = 0.f;
    if (tid < H * Md) {        // normalised keys (needed from R4 on); smooth cosine: the keys as they are
        const int h = tid / Md, m = tid - h * Md;
        const float kh = SMOOTH ? sU[d.oK + tid] : sU[d.oK + tid] * sKinv[h];
        sKhat[tid] = kh;
        sKs[tid] = SMOOTH ? kh : kh * sCinv[m];
    }
    if (hn) {
        const float den = ntm_red_read<NQS>(c, hh, QR1) + 1e-3f;
        const float s2 = ntm_red_read<NQS>(c, hh, QR1 + 1);
        dpw = (dwt - s2) / den;
        dwv = (wv > 0.f) ? dpw * gam * pw / wv : 0.f;
        sDwv[tid] = dwv;
        rv[0] = (wv > 0.f) ? dpw * pw * logf(wv) : 0.f;        // d gamma
        const int start = -((SS + 1) >> 1);
#pragma unroll
        for (int j = 0; j < NQ - 1; ++j) {
            if (j < SS) {
                int src = nn + start + j; src = (src % N + N) % N;
                rv[1 + j] = dwv * sWg[hh * N + src];            // d shift_j
            }
        }
    }
    ntm_red_write<NQS>(c, w, rv, 1 + SS, QR2);
    barrier(2);

    // ------------------------------------------------ R3: shift + gate backward
    float dwg = 0.f, dwc = 0.f;
    float Sgam = 0.f, Ssw[NQ - 1];
    if (hn) {
        Sgam = ntm_red_read<NQS>(c, hh, QR2);
#pragma unroll
        for (int j = 0; j < NQ - 1; ++j) Ssw[j] = (j < SS) ? ntm_red_read<NQS>(c, hh, QR2 + 1 + j) : 0.f;
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
    ntm_red_write<NQS>(c, w, rv, 2, QR3);
    barrier(3);

    // ------------------------------------------------ R4: content softmax backward
    float Sg = 0.f, dv = 0.f;
    if (hn) {
        Sg = ntm_red_read<NQS>(c, hh, QR3);
        const float Bs = ntm_red_read<NQS>(c, hh, QR3 + 1);
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
    ntm_red_write<NQS>(c, w, rv, SMOOTH ? 2 : 1, QR4);
    barrier(4);
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
        sDU[d.oB + h] = ntm_red_read<NQS>(c, h, QR4) * (1.0f - expf(-beta));                 // softplus' = 1 - exp(-softplus)
        sDU[d.oG + h] = Sg * gate * (1.0f - gate);
        sDU[d.oY + h] = Sgam * (1.0f - expf(-(gam - 1.0f)));
        float dot = 0.f;
#pragma unroll
        for (int j = 0; j < NQ - 1; ++j) if (j < SS) dot += sSw[h * SS + j] * Ssw[j];
#pragma unroll
        for (int j = 0; j < NQ - 1; ++j) if (j < SS) sDU[d.oS + h * SS + j] = sSw[h * SS + j] * (Ssw[j] - dot);
    }

    stamp(12);
    // ------------------------------------------------ B7: dMhat[n][m] = sum_h dsim[h][n] khat[h][m], computed ONCE
    //                                                  (the column-norm sum and the d(M_prev) update both use it);
    //                                                  reductions over slots (keys, erase, add)
    for (int idx = tid; idx < NMd; idx += T) {
        const int n = idx / Md, m = idx - n * Md;
        float dmh = 0.f;
        for (int h = 0; h < H; ++h) dmh += sDsim[h * N + n] * sKhat[h * Md + m];
        sDmh[n * MP + m] = dmh;
    }
    stamp(13);
    if constexpr (FIX) {
        // benchmark shape (5 heads, 1 write head): a thread = (memory column m = tid >> 4, row class sl = tid & 15) reads
        // M_prev[n][m], G[n][m], ww[n] and dsim[0..4][n] ONCE per row n = sl, sl + 16, ... and feeds seven sums; the sixteen
        // row classes of a column are sixteen adjacent lanes, reduced on the DPP path: 20 K LDS reads per step instead of 41 K,
        // no slot partials (the one-output-per-thread form below was 14 % of a BPTT step)
        if (tid < 16 * Md) {
            const int m = tid >> 4, sl = tid & 15;
            float a0 = 0.f, a1 = 0.f, a2 = 0.f, a3 = 0.f, a4 = 0.f, ae = 0.f, aa = 0.f;
#pragma unroll 4
            for (int n = sl; n < N; n += 16) {
                const float mp = sMp[n * MP + m], g = sG[n * MP + m], ww = sWt[R * N + n];
                a0 += sDsim[0 * N + n] * mp; a1 += sDsim[1 * N + n] * mp; a2 += sDsim[2 * N + n] * mp;
                a3 += sDsim[3 * N + n] * mp; a4 += sDsim[4 * N + n] * mp;
                const float wg = ww * g;
                ae -= wg * mp;
                aa += wg;
            }
            auto r16 = [](float v) { v += ntk_dpp<0xB1>(v); v += ntk_dpp<0x4E>(v); v += ntk_dpp<0x141>(v); v += ntk_dpp<0x140>(v); return v; };
            a0 = r16(a0); a1 = r16(a1); a2 = r16(a2); a3 = r16(a3); a4 = r16(a4); ae = r16(ae); aa = r16(aa);
            if (sl == 0) {
                sPart[0 * Md + m] = a0; sPart[1 * Md + m] = a1; sPart[2 * Md + m] = a2; sPart[3 * Md + m] = a3; sPart[4 * Md + m] = a4;
                sPart[H * Md + m] = ae; sPart[H * Md + Wh * Md + m] = aa;
            }
        }
    } else if (tid < nslP * nout) {
        const int o = tid % nout, sl = tid / nout;
        const int n0 = sl * nperP, n1 = min(N, n0 + nperP);
        float s = 0.f;
        if (o < H * Md) {                                  // sum_n dsim[h][n] * M_prev[n][m]
            const int h = o / Md, m = o - h * Md;
            // four independent chains, four rows per trip: the rolled single-chain loop paid an LDS round trip + the add
            // latency per row (this phase was 18 % of a BPTT step)
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
            float sa = 0.f, sb = 0.f;                       // two chains (even / odd rows)
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
    barrier(5);
    // column-norm term: s_m = sum_n dMhat[n][m] * M_prev[n][m], one wave_sum per column (waves stride over m)
    if constexpr (!SMOOTH)
    for (int m = (tid >> 6); m < Md; m += (T >> 6)) {
        float s = 0.f;
        for (int n = lane; n < N; n += 64) s += sDmh[n * MP + m] * sMp[n * MP + m];
        s = wave_sum(s);
        if (lane == 0) {
            const float ci = sCinv[m];
            sC2[m] = (sCss[m] > 1e-12f) ? -ci * ci * ci * s : 0.f;   // dM += M * C2 (2 * d css)
        }
    }
    if (tid < nout) {
        float s = 0.f;
        for (int sl = 0; sl < (FIX ? 1 : nslP); ++sl) s += sPart[sl * nout + tid];
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
    barrier(6);
    if (tid < H * Md) {
        const int h = tid / Md;
        if constexpr (SMOOTH) {                                 // d k = sum_n a M_prev[n] + k / |k| * sum_n b |M[n]|, 0 through |k| = 0
            const float kn = sKinv[h], kv = sU[d.oK + tid];
            const float dk = sDkhat[tid] + ((kn > 0.f) ? kv / kn * ntm_red_read<NQS>(c, h, QR4 + 1) : 0.f);
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
    barrier(7);
    if (tid < PP) a.du[bt * PP + tid] = sDU[tid];

    // ------------------------------------------------ B9: dh' = carried dh + dU . Wa^T
    if (tid < nslH * hg4) {
        const int cg = tid % hg4, sl = tid / hg4;
        const int c0 = sl * nperH, c1 = min(PP, c0 + nperH);
        if constexpr (FIX) {
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const int cs = min(c1, c0 + NTMB_RES_WA);
            const f32x4 str = ntk_stream_matvec_exact<4>(reinterpret_cast<const f32x4*>(a.WaT) + cg, hg4, sDU, cs, c1);
#pragma unroll
            for (int q = 0; q < NTMB_RES_WA; ++q) acc += ((c0 + q < c1) ? sDU[c0 + q] : 0.f) * sWaRes4[q * (nslH * hg4) + tid];
            sPart4[sl * hg4 + cg] = acc + str;
        } else {
            sPart4[sl * hg4 + cg] = ntk_stream_matvec<(MAXT > 768 ? 2 : 4)>(reinterpret_cast<const f32x4*>(a.WaT) + cg, hg4, sDU, c0, c1, PP - 1);
        }
    }
    barrier(8);
}
