// The phases both k-workgroups-per-sequence DNC forms run, once: the LDS-resident form (dnc_cluster_fwd.hip / dnc_cluster_bwd.hip)
// and the memory-partitioned form (dnc_mp_fwd.hip / dnc_mp_bwd.hip) differ in what they do with the N x W memory, the N x N link
// and the hand-offs those need; everything per hidden unit and per slot is here.  Device code only; phase names (P1 .. P8 of the
// forward step, B1 .. B16 of the BPTT step) and the reference's line numbers are those of the kernel files.
//
// Everything is a __forceinline__ function template over the form's shape block (DncClusterCfg / DncMpCfg: same field names), its
// kernel arguments (same field names; a by-value block or the kernarg-segment reference of a step) and one by-value struct of LDS
// pointers and per-step values.  A kernel builds that struct INSIDE its step, from the shape block, the opaque thread id and the
// opaque kernarg pointer of that step (nothing is hoisted above the time loop); at the FIX instantiations the shape block is a
// compile-time constant and folds after inlining, as it did in place.  A phase contains a workgroup barrier where the text it
// replaces did (the publishes, P5c | P5d, B6, B8 | B9): every thread of the workgroup calls it.  Several blocks carry exactness
// contracts (fp contract off, "exactly the forward kernel's expression", the tie-break of the allocation sort): the tested claim
// that both forms equal the one-workgroup kernel rests on this one copy.
#pragma once
#include "dnc_cluster.h"

constexpr float CL_EPS = 1e-6f;

// ------------------------------------------------------------------------------------------------ launch prologue
// workgroup -> (sequence b, member g): with xcd_local the k members of a sequence share blockIdx % 8 (speed only, never correctness)
__device__ __forceinline__ void dncc_block_to_bg(int xcd_local, int k, int& b, int& g) {
    if (xcd_local) {
        const int x = blockIdx.x & 7, s = blockIdx.x >> 3;
        b = x + 8 * (s / k);
        g = s % k;
    } else {
        b = blockIdx.x / k;
        g = blockIdx.x % k;
    }
}

// same-XCD fast form of the hand-offs (dnc_cluster.h): decided per cluster by a handshake, never assumed.  s_word: two ints in
// LDS (s_word[-1] is the abort word of cl_wait).  False when the launch was aborted (sticky: as cl_wait).
__device__ __forceinline__ bool dncc_same_xcd_prologue(int xcd_local, unsigned* xcc, int b, int g, int k, unsigned* err, unsigned* sticky,
                                                       int* s_word, unsigned long long t_start, int tid, bool& plain) {
    plain = false;
    if (xcd_local) {
        const int same = cl_same_xcd(xcc + (size_t)b * k, g, k, err, s_word - 1, s_word, t_start, tid);
        if (same < 0) { if (sticky && tid == 0) __hip_atomic_store(sticky, 1u, NTK_RLX, NTK_AGENT); return false; }
        plain = __builtin_amdgcn_readfirstlane(same) != 0;
    }
    return true;
}

// number of keys[0 .. cnt) above `mine` (cnt a multiple of 8, keys 16-byte aligned): the rank of a slot in the usage order is this
// count over all N keys (the LDS form: nslA slices per slot, the partitioned form: the own N / k keys, summed over the workgroups)
template <int UNROLL = 0>
__device__ __forceinline__ int dncc_rank_count(const unsigned long long* keys, int cnt, unsigned long long mine) {
    const u64x2* kp = reinterpret_cast<const u64x2*>(keys);
    int c = 0;
    auto eight = [&](int m) {
        const u64x2 k0 = kp[(m >> 1)], k1 = kp[(m >> 1) + 1], k2 = kp[(m >> 1) + 2], k3 = kp[(m >> 1) + 3];
        c += (k0[0] > mine) + (k0[1] > mine) + (k1[0] > mine) + (k1[1] > mine) + (k2[0] > mine) + (k2[1] > mine) +
             (k3[0] > mine) + (k3[1] > mine);
    };
    if constexpr (UNROLL > 0) {
#pragma unroll UNROLL
        for (int m = 0; m < cnt; m += 8) eight(m);
    } else {
        for (int m = 0; m < cnt; m += 8) eight(m);
    }
    return c;
}

// exclusive cumulative product over v[0 .. N) in place, by ONE wave (N a multiple of 64, N <= 512): tf.cumprod(exclusive=True),
// addressing.py:399, in rank order
__device__ __forceinline__ void dncc_excl_cumprod(float* v, int N, int lane) {
    const int PER = N >> 6, bs = lane * PER;
    float ex[8], run = 1.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < PER) { ex[j] = run; run *= v[bs + j]; }
    float inc = run;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) { const float o = __shfl_up(inc, dd, 64); if (lane >= dd) inc *= o; }
    float excl = __shfl_up(inc, 1, 64);
    if (lane == 0) excl = 1.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < PER) v[bs + j] = excl * ex[j];
}

// exclusive SUFFIX sum over v[0 .. N) in place, by one wave: v[r] = sum_{r' > r} v[r']
__device__ __forceinline__ void dncc_excl_suffix_sum(float* v, int N, int lane) {
    const int PER = N >> 6, bs = lane * PER;
    float ex[8], run = 0.f;
#pragma unroll
    for (int j = 7; j >= 0; --j) if (j < PER) { ex[j] = run; run += v[bs + j]; }
    float inc = run;
#pragma unroll
    for (int dd = 1; dd < 64; dd <<= 1) { const float o = __shfl_down(inc, dd, 64); if (lane + dd < 64) inc += o; }
    float excl = __shfl_down(inc, 1, 64);
    if (lane == 63) excl = 0.f;
#pragma unroll
    for (int j = 0; j < 8; ++j) if (j < PER) v[bs + j] = excl + ex[j];
}

// ------------------------------------------------------------------------------------------------ forward
struct DncClFwdSt {
    float *sPart, *sZ, *sC, *sHP, *sI, *sK, *sU, *sNU, *sRW, *sWW, *sP, *sCW, *sSC;
    unsigned long long* sKEY;
    int* sRank;
    int tid, g, row0, u0, u1;      // thread; member of the cluster, its first slot / link row, its hidden units [u0, u1)
    size_t bt;                     // b * S + t
    bool rec, plain;               // BPTT records wanted; plain hand-off stores (same-XCD form)
    float clipv;
};

template <class Lds, class Cfg>
__device__ __forceinline__ DncClFwdSt dncc_fwd_state(float* smem, const Lds& L, const Cfg& C, int g, int tid) {
    DncClFwdSt s;
    s.sPart = smem + L.part; s.sZ = smem + L.Z; s.sC = smem + L.C; s.sHP = smem + L.HP; s.sI = smem + L.I; s.sK = smem + L.K;
    s.sU = smem + L.U; s.sNU = smem + L.NU; s.sRW = smem + L.RW; s.sWW = smem + L.WW; s.sP = smem + L.P; s.sCW = smem + L.CW;
    s.sSC = smem + L.SC;
    s.sKEY = reinterpret_cast<unsigned long long*>(smem + L.KEY);
    s.sRank = reinterpret_cast<int*>(smem + L.RANK);
    s.tid = tid; s.g = g; s.row0 = g * C.NR; s.u0 = min(C.hid, g * C.upk); s.u1 = min(C.hid, s.u0 + C.upk);
    s.bt = 0; s.rec = false; s.plain = false; s.clipv = 0.f;
    return s;
}

// state in: the per-slot vectors and the controller state (replicated), the cell of the own units; keys zeroed
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_fwd_load_state(const Cfg& C, const Args& a, const DncClFwdSt& s, int b) {
    const int N = C.N, R = C.R, RWd = R * C.W, hid = C.hid, nU = s.u1 - s.u0, tid0 = s.tid;
    for (int i = tid0; i < N; i += CT) {
        s.sU[i] = a.usage[(size_t)b * N + i];
        s.sWW[i] = a.ww[(size_t)b * N + i];
        s.sP[i] = a.prec[(size_t)b * N + i];
    }
    for (int i = tid0; i < R * N; i += CT) s.sRW[i] = a.rw[(size_t)b * R * N + i];
    for (int i = tid0; i < RWd; i += CT) s.sZ[i] = a.reads[(size_t)b * RWd + i];
    for (int i = tid0; i < hid; i += CT) s.sZ[RWd + i] = a.hc[(size_t)b * 2 * hid + i];
    for (int i = tid0; i < nU; i += CT) s.sC[i] = a.hc[(size_t)b * 2 * hid + hid + s.u0 + i];
    for (int i = tid0; i < (1 + R) * C.W; i += CT) s.sK[i] = 0.f;
}

// state out: the cell of the own units; the replicated vectors by workgroup 0
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_fwd_store_state(const Cfg& C, const Args& a, const DncClFwdSt& s, int b) {
    const int N = C.N, R = C.R, RWd = R * C.W, hid = C.hid, nU = s.u1 - s.u0, tid0 = s.tid;
    for (int i = tid0; i < nU; i += CT) a.hc[(size_t)b * 2 * hid + hid + s.u0 + i] = s.sC[i];
    if (s.g == 0) {
        for (int i = tid0; i < N; i += CT) {
            a.usage[(size_t)b * N + i] = s.sU[i];
            a.ww[(size_t)b * N + i] = s.sWW[i];
            a.prec[(size_t)b * N + i] = s.sP[i];
        }
        for (int i = tid0; i < R * N; i += CT) a.rw[(size_t)b * R * N + i] = s.sRW[i];
        for (int i = tid0; i < RWd; i += CT) a.reads[(size_t)b * RWd + i] = s.sZ[i];
        for (int i = tid0; i < hid; i += CT) a.hc[(size_t)b * 2 * hid + i] = s.sZ[RWd + i];
    }
}

// P1: the input of the own units' gates (input projection row + bias row of Wr) and the record of the controller input
template <class Cfg, class Args>
__device__ __forceinline__ f32x4 dncc_fwd_gate_input(const Cfg& C, const Args& a, const DncClFwdSt& s) {
    f32x4 xg = {0.f, 0.f, 0.f, 0.f};
    if (s.tid < s.u1 - s.u0)
        xg = reinterpret_cast<const f32x4*>(a.xproj)[s.bt * C.hid + s.u0 + s.tid] + reinterpret_cast<const f32x4*>(a.Wr)[(size_t)C.K * C.hid + s.u0 + s.tid];
    return xg;
}
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_fwd_rec_z(const Cfg& C, const Args& a, const DncClFwdSt& s) {
    const int K = C.K;
    if (s.rec && s.g == 0) for (int i = s.tid; i < C.ldz; i += CT) a.rec_z[s.bt * C.ldz + i] = (i < K) ? s.sZ[i] : (i == K ? 1.f : 0.f);
}

// P1: gate product of the own units, streamed: a thread = one own unit x one K-slice -> sPart4[slice][unit]
template <class Cfg>
__device__ __forceinline__ void dncc_fwd_gate_partials(const Cfg& C, const DncClFwdSt& s, const f32x4* Wr4) {
    const int tid = s.tid, upk = C.upk, K = C.K, kperG = C.kperG;
    if (tid < C.ksl * upk) {
        const int ks = cl_div(tid, C.mg_upk), j = tid - ks * upk;
        const int k0 = ks * kperG, k1 = min(K, k0 + kperG);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (j < s.u1 - s.u0 && k0 < k1) acc = ntk_stream_matvec<4>(Wr4 + s.u0 + j, C.hid, s.sZ, k0, k1, K - 1);
        reinterpret_cast<f32x4*>(s.sPart)[ks * upk + j] = acc;
    }
}

// P1: sum of the gate partials, snt.LSTM pointwise step of the own units, their records
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_fwd_lstm(const Cfg& C, const Args& a, const DncClFwdSt& s, f32x4 xg) {
    const int tid = s.tid, upk = C.upk, hid = C.hid, RWd = C.R * C.W, u0 = s.u0, ksl = C.ksl;
    const f32x4* sPart4 = reinterpret_cast<const f32x4*>(s.sPart);
    if (tid < s.u1 - u0) {
        f32x4 gsum = xg;
        for (int ks = 0; ks < ksl; ++ks) gsum += sPart4[ks * upk + tid];
        const float gi = cl_sigmoid(gsum[0]), gj = cl_tanh(gsum[1]);
        const float gf = cl_sigmoid(gsum[2] + 1.0f);             // snt.LSTM forget_bias = 1.0
        const float go = cl_sigmoid(gsum[3]);
        // written out: left to the compiler, WHICH of the two products is fused into the add differs between instantiations
        const float c2 = fmaf(gi, gj, gf * s.sC[tid]);
        const float h2 = cl_tanh(c2) * go;
        s.sC[tid] = dnc_clip(c2, s.clipv);                       // dnc.py:112-113
        s.sHP[tid] = s.sZ[RWd + u0 + tid];                       // h_{t-1}: still needed by the deferred output of step t-1
        s.sZ[RWd + u0 + tid] = dnc_clip(h2, s.clipv);
        if (s.rec) {
            f32x4 ga = {gi, gj, gf, go};
            reinterpret_cast<f32x4*>(a.rec_gates)[s.bt * hid + u0 + tid] = ga;
            a.rec_c[s.bt * hid + u0 + tid] = c2;
        }
    }
}

// P2: interface partial sums over the own units: a thread = one float4 column group x one unit slice -> sPart4[slice][group]
template <class Cfg>
__device__ __forceinline__ void dncc_fwd_ifc_partials(const Cfg& C, const DncClFwdSt& s, const f32x4* Wi4) {
    const int tid = s.tid, icg = C.icg, uperI = C.uperI, RWd = C.R * C.W;
    if (tid < C.nslI * icg) {
        const int us = cl_div(tid, C.mg_icg), cg = tid - us * icg;
        const int ua = s.u0 + us * uperI, ub = min(s.u1, ua + uperI);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        const f32x4* wp = Wi4 + (size_t)ua * icg + cg;
#pragma unroll 8
        for (int u = ua; u < ub; ++u, wp += icg) acc += s.sZ[RWd + u] * (*wp);
        reinterpret_cast<f32x4*>(s.sPart)[us * icg + cg] = acc;
    }
}

// publish hand-off 0: [h of the own units | interface partial] into the own slot; every thread calls (cl_publish)
template <class Cfg>
__device__ __forceinline__ void dncc_fwd_publish0(const Cfg& C, const DncClFwdSt& s, float* slot, unsigned* my_flag, unsigned epoch) {
    const int tid = s.tid, IP = C.IP, nslI = C.nslI, RWd = C.R * C.W;
    if (tid < s.u1 - s.u0) cl_store(slot + tid, s.sZ[RWd + s.u0 + tid], s.plain);
    for (int c = tid; c < IP; c += CT) {
        float v = 0.f;
        for (int us = 0; us < nslI; ++us) v += s.sPart[us * IP + c];
        cl_store(slot + C.upkp + c, v, s.plain);
    }
    cl_publish(my_flag, epoch, tid, s.plain);
}

// y = clip([h ; reads] Wy + by) (dnc.py:118-122) of output o at step index bt, by one wave.  It does not feed the recurrence: a
// step computes y_{t-1} in the shadow of hand-off 0 (DEFERRED: h_{t-1} of the own units is in sHP, already overwritten in sZ; the
// other units' is still in sZ, overwritten after the wait), the epilogue the last step's.
template <bool DEFERRED, class Cfg, class Args>
__device__ __forceinline__ void dncc_fwd_output(const Cfg& C, const Args& a, const DncClFwdSt& s, size_t bt, int o, int lane) {
    const int hid = C.hid, RWd = C.R * C.W;
    float sum = 0.f;
    for (int kk = lane; kk < C.Ky; kk += 64) {
        float zv;
        if constexpr (DEFERRED) zv = (kk < hid) ? ((kk >= s.u0 && kk < s.u1) ? s.sHP[kk - s.u0] : s.sZ[RWd + kk]) : s.sZ[kk - hid];
        else zv = (kk < hid) ? s.sZ[RWd + kk] : s.sZ[kk - hid];
        sum += zv * a.Wy[(size_t)kk * C.OP + o];
    }
    sum = wave_sum(sum);
    if (lane == 0) {
        const float pre = sum + a.Wy[(size_t)C.Ky * C.OP + o];
        a.out[bt * C.O + o] = dnc_clip(pre, s.clipv);
        if (s.rec) a.rec_ypre[bt * C.O + o] = pre;
    }
}

// consume hand-off 0: h of every unit (base: the k slots of this step's parity, slot0 floats each)
template <class Cfg>
__device__ __forceinline__ void dncc_fwd_gather_h(const Cfg& C, const DncClFwdSt& s, const float* base, int slot0) {
    const int hid = C.hid, upk = C.upk, RWd = C.R * C.W;
    for (int u = s.tid; u < hid; u += CT) {
        const int gg = cl_div(u, C.mg_upk);
        s.sZ[RWd + u] = cl_load(base + (size_t)gg * slot0 + (u - gg * upk));
    }
}

// consume hand-off 0: interface column c from its pre-activation v (+ aligned copies of the keys: write key, then the read keys)
template <class Cfg>
__device__ __forceinline__ void dncc_fwd_ifc_column(const Cfg& C, const DncClFwdSt& s, int c, float v) {
    float r = v;
    if (c >= C.oE && c < C.oRm) r = dnc_sigmoid(v);                      // erase, free, alloc, write gates
    else if ((c >= C.oBw && c < C.oKr) || (c >= C.oBr && c < C.I)) r = dnc_softplus(v);   // strengths
    s.sI[c] = r;
    if (c >= C.oKw && c < C.oBw) s.sK[c - C.oKw] = r;
    else if (c >= C.oKr && c < C.oBr) s.sK[C.W + (c - C.oKr)] = r;
}

// records of the controller output and of the activated interface (workgroup 0)
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_fwd_rec_hc_ifc(const Cfg& C, const Args& a, const DncClFwdSt& s) {
    const int tid = s.tid, hid = C.hid, IP = C.IP, RWd = C.R * C.W;
    const size_t bt = s.bt;
    if (s.rec && s.g == 0) {
        for (int i = tid; i < C.ldh; i += CT) {
            const float v = (i < hid) ? s.sZ[RWd + i] : (i == hid ? 1.f : 0.f);
            a.rec_hc[bt * C.ldh + i] = v;
            if (i < hid) a.rec_yin[bt * C.ldy + i] = v;
        }
        for (int c = tid; c < IP; c += CT) {
            float v = s.sI[c];
            if (c >= C.oRm && c < C.oKw) {             // the read modes are recorded after their softmax (computed below)
                const float* rm = s.sI + C.oRm + ((c - C.oRm) / 3) * 3;
                const float mx = fmaxf(rm[0], fmaxf(rm[1], rm[2]));
                const float e0 = expf(rm[0] - mx), e1 = expf(rm[1] - mx), e2 = expf(rm[2] - mx);
                v = expf(v - mx) / (e0 + e1 + e2);
            }
            a.rec_ifc[bt * IP + c] = v;
        }
    }
}

// key norms: wave i < 1 + R  ->  sSC[8 + i] = sqrt(|key_i|^2 + eps)
template <class Cfg>
__device__ __forceinline__ void dncc_fwd_key_norms(const Cfg& C, const DncClFwdSt& s) {
    const int W = C.W, lane = s.tid & 63, wave = s.tid >> 6;
    if (wave < 1 + C.R) {
        float ss = 0.f;
        for (int w = lane; w < W; w += 64) { const float kv = s.sK[wave * W + w]; ss += kv * kv; }
        ss = wave_sum(ss);
        if (lane == 0) s.sSC[8 + wave] = sqrtf(ss + CL_EPS);
    }
}

// P3: usage (addressing.py:342-374), op by op, with the sort key of the allocation
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_fwd_usage(const Cfg& C, const Args& a, const DncClFwdSt& s) {
    const int N = C.N, R = C.R, NR = C.NR, row0 = s.row0;
    const float EPS = CL_EPS;
    {
#pragma clang fp contract(off)
        float fg[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) fg[i] = (i < R) ? s.sI[C.oF + i] : 0.f;
        for (int n = s.tid; n < N; n += CT) {
            float pw = 1.f;
            pw *= (1.0f - s.sWW[n]);
            float u = s.sU[n];
            u = u + (1.0f - u) * (1.0f - pw);
            float phi = 1.f;
#pragma unroll
            for (int i = 0; i < 4; ++i) if (i < R) phi *= (1.0f - fg[i] * s.sRW[i * N + n]);
            u *= phi;
            s.sU[n] = u;
            const float nu = 1.0f - (EPS + (1.0f - EPS) * u);
            s.sNU[n] = nu;
            // sort key of the allocation: larger nonusage first, ties to the lower slot (tf.nn.top_k); nonusage >= +0,
            // so its bit pattern orders like its value
            s.sKEY[n] = ((unsigned long long)__float_as_uint(nu) << 32) | (unsigned)(0xFFFF - n);
            if (s.rec && n >= row0 && n < row0 + NR) a.rec_u[s.bt * N + n] = u;
        }
    }
}

// read_mode softmax (access.py:186-187), in place in the interface
template <class Cfg>
__device__ __forceinline__ void dncc_fwd_read_modes(const Cfg& C, const DncClFwdSt& s) {
    if (s.tid < C.R) {
        float* rm = s.sI + C.oRm + s.tid * 3;
        const float mx = fmaxf(rm[0], fmaxf(rm[1], rm[2]));
        const float e0 = expf(rm[0] - mx), e1 = expf(rm[1] - mx), e2 = expf(rm[2] - mx);
        const float sum = e0 + e1 + e2;
        rm[0] = e0 / sum; rm[1] = e1 / sum; rm[2] = e2 / sum;
    }
}

// P5c | P5d: sT holds the usages in rank order, sCW the write-content weights.  Exclusive cumulative product by wave 0, barrier,
// allocation and write weights (access.py:220-257), op by op; every thread calls
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_fwd_alloc_write_weights(const Cfg& C, const Args& a, const DncClFwdSt& s, float* sT) {
    const int N = C.N, NR = C.NR, row0 = s.row0;
    if ((s.tid >> 6) == 0) dncc_excl_cumprod(sT, N, s.tid & 63);
    __syncthreads();
    {
#pragma clang fp contract(off)
        const float ag = s.sI[C.oAg], wg = s.sI[C.oWg];
        for (int n = s.tid; n < N; n += CT) {
            const float al = s.sNU[n] * sT[s.sRank[n]];
            const float cw = s.sCW[n];
            s.sWW[n] = wg * (ag * al + (1.0f - ag) * cw);
            if (s.rec && n >= row0 && n < row0 + NR) { a.rec_al[s.bt * N + n] = al; a.rec_cw[s.bt * N + n] = cw; }
        }
    }
}

// sum of the write weights (precedence update) by one wave -> sSC[0]
__device__ __forceinline__ void dncc_fwd_ww_sum(const DncClFwdSt& s, int N, int lane) {
    float sum = 0.f;
    for (int n = lane; n < N; n += 64) sum += s.sWW[n];
    sum = wave_sum(sum);
    if (lane == 0) s.sSC[0] = sum;
}

// precedence update (addressing.py:238-240) with its records
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_fwd_precedence(const Cfg& C, const Args& a, const DncClFwdSt& s) {
    const int N = C.N, NR = C.NR, row0 = s.row0;
    const float sww = s.sSC[0];
    for (int n = s.tid; n < N; n += CT) {
        const float pn = (1.0f - sww) * s.sP[n] + s.sWW[n];                         // addressing.py:238-240
        s.sP[n] = pn;
        if (s.rec && n >= row0 && n < row0 + NR) { a.rec_p[s.bt * N + n] = pn; a.rec_ww[s.bt * N + n] = s.sWW[n]; }
    }
}

// ------------------------------------------------------------------------------------------------ BPTT
struct DncClBwdSt {
    float *sPart, *sI, *sDX, *sWW, *sWWp, *sU, *sUp, *sPp, *sCW, *sAL, *sSIMw, *sDWW, *sDCW, *sDA, *sgP, *sDPp, *sgU, *sgUn, *sNU;
    unsigned long long* sKEY;
    int* sRank;
    float *sRWp, *sRWt, *sgRW, *sG, *sDRWp, *sDSIM, *sSIMr, *sGZ, *sDR, *sDHC, *sDG, *sgC, *sSC;
    int tid, g, u0, u1;
    size_t bt;
    bool plain;
    float clipv;
};

template <class Lds, class Cfg>
__device__ __forceinline__ DncClBwdSt dncc_bwd_state(float* smem, const Lds& L, const Cfg& C, int g, int tid) {
    DncClBwdSt s;
    s.sPart = smem + L.part; s.sI = smem + L.I; s.sDX = smem + L.DX;
    s.sWW = smem + L.WW; s.sWWp = smem + L.WWp; s.sU = smem + L.U; s.sUp = smem + L.Up; s.sPp = smem + L.Pp; s.sCW = smem + L.CW;
    s.sAL = smem + L.AL; s.sSIMw = smem + L.SIMw; s.sDWW = smem + L.DWW; s.sDCW = smem + L.DCW; s.sDA = smem + L.DA;
    s.sgP = smem + L.gP; s.sDPp = smem + L.DPp; s.sgU = smem + L.gU; s.sgUn = smem + L.gUn; s.sNU = smem + L.NU;
    s.sKEY = reinterpret_cast<unsigned long long*>(smem + L.KEY);
    s.sRank = reinterpret_cast<int*>(smem + L.RANK);
    s.sRWp = smem + L.RWp; s.sRWt = smem + L.RWt; s.sgRW = smem + L.gRW; s.sG = smem + L.G; s.sDRWp = smem + L.DRWp;
    s.sDSIM = smem + L.DSIM; s.sSIMr = smem + L.SIMr; s.sGZ = smem + L.GZ; s.sDR = smem + L.DR; s.sDHC = smem + L.DHC;
    s.sDG = smem + L.DG; s.sgC = smem + L.gC; s.sSC = smem + L.SC;
    s.tid = tid; s.g = g; s.u0 = min(C.hid, g * C.upk); s.u1 = min(C.hid, s.u0 + C.upk);
    s.bt = 0; s.plain = false; s.clipv = 0.f;
    return s;
}

// carried gradients in: zero (the loss depends on the outputs only) or what the following segment left behind
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_bwd_carry_in(const Cfg& C, const Args& a, const DncClBwdSt& s, int b, int ldkT) {
    const int N = C.N, RN = C.R * N, K = C.K, hid = C.hid, nU = s.u1 - s.u0, tid0 = s.tid;
    float* cy = a.gcarry ? a.gcarry + (size_t)b * (2 * N + RN + ldkT + hid) : nullptr;
    const bool cin = cy && a.carry_in;
    for (int i = tid0; i < N; i += CT) { s.sgP[i] = cin ? cy[i] : 0.f; s.sgU[i] = cin ? cy[N + i] : 0.f; }
    for (int i = tid0; i < RN; i += CT) s.sgRW[i] = cin ? cy[2 * N + i] : 0.f;
    for (int i = tid0; i < ldkT; i += CT) s.sGZ[i] = (cin && i < K) ? cy[2 * N + RN + i] : 0.f;
    for (int i = tid0; i < nU; i += CT) s.sgC[i] = cin ? cy[2 * N + RN + ldkT + s.u0 + i] : 0.f;
}

// carried gradients out (segmented BPTT)
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_bwd_carry_out(const Cfg& C, const Args& a, const DncClBwdSt& s, int b, int ldkT) {
    const int N = C.N, RN = C.R * N, hid = C.hid, nU = s.u1 - s.u0, tid0 = s.tid;
    float* cy = a.gcarry ? a.gcarry + (size_t)b * (2 * N + RN + ldkT + hid) : nullptr;
    if (cy) {
        if (s.g == 0) {
            for (int i = tid0; i < N; i += CT) { cy[i] = s.sgP[i]; cy[N + i] = s.sgU[i]; }
            for (int i = tid0; i < RN; i += CT) cy[2 * N + i] = s.sgRW[i];
            for (int i = tid0; i < ldkT; i += CT) cy[2 * N + RN + i] = s.sGZ[i];
        }
        for (int i = tid0; i < nU; i += CT) cy[2 * N + RN + ldkT + s.u0 + i] = s.sgC[i];
    }
}

// the per-slot records of slot n -> LDS, with the nonusage and the sort key of the forward pass
__device__ __forceinline__ void dncc_bwd_slot_records(const DncClBwdSt& s, int n, float ww, float u_, float cw, float al, float wwp, float up,
                                                      float pp) {
    const float EPS = CL_EPS;
    {
#pragma clang fp contract(off)
        const float u = u_;
        s.sWW[n] = ww;
        s.sU[n] = u;
        s.sCW[n] = cw;
        s.sAL[n] = al;
        s.sWWp[n] = wwp;
        s.sUp[n] = up;
        s.sPp[n] = pp;
        const float nu = 1.0f - (EPS + (1.0f - EPS) * u);             // exactly the forward kernel's expression
        s.sNU[n] = nu;
        s.sKEY[n] = ((unsigned long long)__float_as_uint(nu) << 32) | (unsigned)(0xFFFF - n);
    }
}

// B1: output clip + linear (ypre, dout: this thread's record and loss gradient, threads tid < O)
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_bwd_output_clip(const Cfg& C, const Args& a, const DncClBwdSt& s, float ypre, float dout) {
    const int tid = s.tid;
    if (tid < 64) s.sSC[tid] = 0.f;
    if (tid < C.OP) {
        float gy = 0.f;
        if (tid < C.O) gy = (s.clipv <= 0.f || fabsf(ypre) < s.clipv) ? dout : 0.f;
        s.sSC[32 + tid] = gy;
        if (s.g == 0) a.dypre[s.bt * C.OP + tid] = gy;
    }
}

// d[h ; reads] of this step: the carried gradient + the output path (Wy^T); key norms: sSC[0..R-1] = |kr_i|, sSC[R] = |kw|
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_bwd_output_path_key_norms(const Cfg& C, const Args& a, const DncClBwdSt& s) {
    const int tid = s.tid, lane = tid & 63, wave = tid >> 6, hid = C.hid, R = C.R, W = C.W, RWd = R * W;
    for (int kk = tid; kk < C.Ky; kk += CT) {
        float sum = 0.f;
        for (int o = 0; o < C.O; ++o) sum += a.Wy[(size_t)kk * C.OP + o] * s.sSC[32 + o];
        if (kk < hid) s.sDHC[kk] = s.sGZ[RWd + kk] + sum;       // carried d(clipped h) + this step's output path
        else s.sDR[kk - hid] = s.sGZ[kk - hid] + sum;           // carried d(reads) + output path
    }
    if (wave <= R) {
        const float* kp = (wave < R) ? s.sI + C.oKr + wave * W : s.sI + C.oKw;
        float ss = 0.f;
        for (int w = lane; w < W; w += 64) ss += kp[w] * kp[w];
        ss = wave_sum(ss);
        if (lane == 0) s.sSC[wave] = sqrtf(ss + CL_EPS);
    }
}

// B3: read-weight mix, read-content softmax (wave i = head i).  cr / fv / bv: the head's recorded content weights, forward and
// backward directional reads of slots lane + 64 j
template <int NJ, class Cfg>
__device__ __forceinline__ void dncc_bwd_read_mix(const Cfg& C, const DncClBwdSt& s, const float (&pf_cr)[NJ], const float (&pf_fv)[NJ],
                                                  const float (&pf_bv)[NJ]) {
    const int N = C.N, lane = s.tid & 63, wave = s.tid >> 6;
    if (wave < C.R) {
        const int i = wave;
        const float* rm = s.sI + C.oRm + i * 3;              // [backward, forward, content] (access.py:283-289)
        float p0 = 0.f, p1 = 0.f, p2 = 0.f, s1 = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int n = lane + 64 * j;
            if (n < N) {
                const float gg = s.sG[i * N + n], cr = pf_cr[j];
                p0 += gg * pf_bv[j]; p1 += gg * pf_fv[j]; p2 += gg * cr;
                s1 += cr * (rm[2] * gg);
            }
        }
        p0 = wave_sum(p0); p1 = wave_sum(p1); p2 = wave_sum(p2); s1 = wave_sum(s1);
        const float br = s.sI[C.oBr + i];
        float dbeta = 0.f;
#pragma unroll
        for (int j = 0; j < NJ; ++j) {
            const int n = lane + 64 * j;
            if (n < N) {
                const float gg = s.sG[i * N + n];
                const float dscore = pf_cr[j] * (rm[2] * gg - s1);
                dbeta += dscore * s.sSIMr[i * N + n];
                s.sDSIM[i * N + n] = dscore * br;
            }
        }
        dbeta = wave_sum(dbeta);
        if (lane == 0) {
            const float dotp = rm[0] * p0 + rm[1] * p1 + rm[2] * p2;
            s.sDX[C.oRm + i * 3 + 0] = rm[0] * (p0 - dotp);
            s.sDX[C.oRm + i * 3 + 1] = rm[1] * (p1 - dotp);
            s.sDX[C.oRm + i * 3 + 2] = rm[2] * (p2 - dotp);
            s.sDX[C.oBr + i] = dbeta * (1.0f - expf(-br));   // strengths pass through softplus
        }
    }
}

// B6: precedence (wave 0 computes the two scalars); two barriers, every thread calls
template <class Cfg>
__device__ __forceinline__ void dncc_bwd_precedence(const Cfg& C, const DncClBwdSt& s) {
    const int N = C.N, lane = s.tid & 63, wave = s.tid >> 6;
    if (wave == 0) {
        float sw = 0.f, t1 = 0.f;
        for (int n = lane; n < N; n += 64) { sw += s.sWW[n]; t1 += s.sgP[n] * s.sPp[n]; }
        sw = wave_sum(sw); t1 = wave_sum(t1);
        if (lane == 0) { s.sSC[16] = sw; s.sSC[17] = t1; }
    }
    __syncthreads();
    for (int n = s.tid; n < N; n += CT) {
        s.sDPp[n] += (1.0f - s.sSC[16]) * s.sgP[n];
        s.sDWW[n] += s.sgP[n] - s.sSC[17];
    }
    __syncthreads();
}

// B8 | B9 and d(write strength): write-weight mix (access.py:252-257), allocation backward in rank order, d(score) of the
// write-content softmax.  sT: 2 N floats of scratch (rank-ordered usages, rank-ordered dA * a).  Three barriers, every thread calls.
template <class Cfg>
__device__ __forceinline__ void dncc_bwd_write_mix_alloc(const Cfg& C, const DncClBwdSt& s, float* sT) {
    const int N = C.N, tid = s.tid, lane = tid & 63, wave = tid >> 6;
    const float EPS = CL_EPS;
    {
        const float ga = s.sI[C.oAg], gw = s.sI[C.oWg];
        float* sS = sT + N;                                    // rank-ordered dA * a
        for (int n = tid; n < N; n += CT) {
            const float dww = s.sDWW[n];
            const float dA = gw * ga * dww;
            s.sDA[n] = dA;
            s.sDCW[n] = gw * (1.0f - ga) * dww;
            const int rk = s.sRank[n];
            sT[rk] = 1.0f - s.sNU[n];
            sS[rk] = dA * s.sAL[n];
        }
        if (wave == CW - 1) {
            float dgw = 0.f, dga = 0.f, s18 = 0.f;
            for (int n = lane; n < N; n += 64) {
                const float dww = s.sDWW[n];
                dgw += dww * (ga * s.sAL[n] + (1.0f - ga) * s.sCW[n]);
                dga += gw * dww * (s.sAL[n] - s.sCW[n]);
                s18 += s.sCW[n] * (gw * (1.0f - ga) * dww);
            }
            dgw = wave_sum(dgw); dga = wave_sum(dga); s18 = wave_sum(s18);
            if (lane == 0) { s.sDX[C.oWg] = dgw * gw * (1.0f - gw); s.sDX[C.oAg] = dga * ga * (1.0f - ga); s.sSC[18] = s18; }
        }
        __syncthreads();
        // B9: allocation backward in rank order
        //   a[n] = nonusage[n] * prod_{before n} usage  ->  d usage[n] = -dA[n] * prod[n] + (sum_{after n} dA a) / usage[n]
        if (wave == 0) dncc_excl_cumprod(sT, N, lane);         // exclusive prefix product (as the forward pass)
        else if (wave == 1) dncc_excl_suffix_sum(sS, N, lane); // S[r] = sum_{r' > r} dA a
        __syncthreads();
        for (int n = tid; n < N; n += CT) {
            const int rk = s.sRank[n];
            const float ut = 1.0f - s.sNU[n];                  // sorted_usage = 1 - sorted_nonusage
            const float dut = -s.sDA[n] * sT[rk] + sS[rk] / ut;
            s.sgUn[n] = s.sgU[n] + (1.0f - EPS) * dut;         // total d(usage_t)
            s.sDCW[n] = s.sCW[n] * (s.sDCW[n] - s.sSC[18]);    // d(score) of the write-content softmax
        }
    }
    __syncthreads();
    if (wave == 0) {
        float dbeta = 0.f;
        for (int n = lane; n < N; n += 64) dbeta += s.sDCW[n] * s.sSIMw[n];
        dbeta = wave_sum(dbeta);
        const float bw = s.sI[C.oBw];
        if (lane == 0) s.sDX[C.oBw] = dbeta * (1.0f - expf(-bw));
    }
}

// B11: usage backward (addressing.py:342-374)
template <class Cfg>
__device__ __forceinline__ void dncc_bwd_usage(const Cfg& C, const DncClBwdSt& s) {
    const int N = C.N, R = C.R;
    float fgv[4];
#pragma unroll
    for (int i = 0; i < 4; ++i) fgv[i] = (i < R) ? s.sI[C.oF + i] : 0.f;
    for (int n = s.tid; n < N; n += CT) {
        const float gq = s.sgUn[n];
        const float wwp = s.sWWp[n];
        const float u1v = s.sUp[n] + (1.0f - s.sUp[n]) * wwp;                // write weights: stop_gradient
        float rwp[4], phi = 1.f;
#pragma unroll
        for (int i = 0; i < 4; ++i) { rwp[i] = (i < R) ? s.sRWp[i * N + n] : 0.f; phi *= (1.0f - fgv[i] * rwp[i]); }
        const float dphi = gq * u1v;
        s.sgU[n] = gq * phi * (1.0f - wwp);                                  // carried d(usage_{t-1})
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            if (i < R) {
                float oth = 1.f;
#pragma unroll
                for (int i2 = 0; i2 < 4; ++i2) if (i2 != i) oth *= (1.0f - fgv[i2] * rwp[i2]);
                s.sDRWp[i * N + n] += dphi * (-fgv[i]) * oth;
                s.sDSIM[i * N + n] = dphi * (-rwp[i]) * oth;                 // reuse: per-slot term of d(free_gate_i)
            }
        }
    }
}

// d(free gates) from B11's per-slot terms (wave i = head i)
template <class Cfg>
__device__ __forceinline__ void dncc_bwd_free_gates(const Cfg& C, const DncClBwdSt& s) {
    const int N = C.N, lane = s.tid & 63, wave = s.tid >> 6;
    if (wave < C.R) {
        const int i = wave;
        float sum = 0.f;
        for (int n = lane; n < N; n += 64) sum += s.sDSIM[i * N + n];
        sum = wave_sum(sum);
        const float fg = s.sI[C.oF + i];
        if (lane == 0) s.sDX[C.oF + i] = sum * fg * (1.0f - fg);
    }
}

// the vectors carried to step t-1
template <class Cfg>
__device__ __forceinline__ void dncc_bwd_carry_vectors(const Cfg& C, const DncClBwdSt& s) {
    const int N = C.N, RN = C.R * N;
    for (int i = s.tid; i < RN; i += CT) s.sgRW[i] = s.sDRWp[i];                // carried d(read weights_{t-1})
    for (int n = s.tid; n < N; n += CT) s.sgP[n] = s.sDPp[n];                   // carried d(precedence_{t-1})
}

// B15: clip + snt.LSTM backward of the own units (dh: d(clipped h) of unit u0 + tid; gates, c, cprev: its records; first: step 0 of
// the launch, cprev_rec is the caller's hc0)
template <class Cfg, class Args>
__device__ __forceinline__ void dncc_bwd_lstm(const Cfg& C, const Args& a, const DncClBwdSt& s, float dh, f32x4 gg, float c2, float cprev_rec,
                                              bool first) {
    const int tid = s.tid;
    const float clipv = s.clipv;
    if (tid < s.u1 - s.u0) {
        const int u = s.u0 + tid;
        const float gi = gg[0], gj = gg[1], gf = gg[2], go = gg[3];
        // the recorded cell is pre-clip, the carried state was clipped; hc0 is what the forward started from, as given (an initial cell
        // beyond the clip entered the forward's c' = f c + i j unclipped: dnc_seq_bwd.hip B15 does the same)
        const float cprev = first ? cprev_rec : dnc_clip(cprev_rec, clipv);
        const float tc = cl_tanh(c2);
        const float h2 = tc * go;
        const float dh2 = (clipv <= 0.f || fabsf(h2) < clipv) ? dh : 0.f;
        const float dcc = (clipv <= 0.f || fabsf(c2) < clipv) ? s.sgC[tid] : 0.f;
        const float dc2 = dcc + dh2 * go * (1.0f - tc * tc);
        f32x4 dg;
        dg[0] = dc2 * gj * gi * (1.0f - gi);
        dg[1] = dc2 * gi * (1.0f - gj * gj);
        dg[2] = dc2 * cprev * gf * (1.0f - gf);
        dg[3] = dh2 * tc * go * (1.0f - go);
        s.sgC[tid] = dc2 * gf;
        reinterpret_cast<f32x4*>(s.sDG)[tid] = dg;
        reinterpret_cast<f32x4*>(a.dgates)[s.bt * C.hid + u] = dg;
    }
}

// B16: partial d[reads_prev ; h_prev] over the own gate columns (rows of Wr^T), published into the own slot of the last hand-off;
// Q: the form's BPTT geometry (kg4, nslZ, nperZ, ldkT, mg_kg4); PF: rows per batch of the stream.  Every thread calls.
template <int PF, class Geo, class Args>
__device__ __forceinline__ void dncc_bwd_zprev_publish(const Geo& Q, const Args& a, const DncClBwdSt& s, float* slot, unsigned* my_flag, unsigned epoch) {
    const int tid = s.tid, kg4 = Q.kg4, nrow = 4 * (s.u1 - s.u0);
    if (tid < Q.nslZ * kg4) {
        const int sl = cl_div(tid, Q.mg_kg4), cg = tid - sl * kg4;
        const int r0 = sl * Q.nperZ, r1 = min(nrow, r0 + Q.nperZ);
        f32x4 acc = {0.f, 0.f, 0.f, 0.f};
        if (r0 < r1) acc = ntk_stream_matvec<PF>(reinterpret_cast<const f32x4*>(a.WrT) + (size_t)(4 * s.u0) * kg4 + cg, kg4, s.sDG, r0, r1, nrow - 1);
        *reinterpret_cast<f32x4*>(s.sPart + sl * Q.ldkT + cg * 4) = acc;
    }
    __syncthreads();
    for (int kk = tid; kk < Q.ldkT; kk += CT) {
        float sum = 0.f;
        for (int sl = 0; sl < Q.nslZ; ++sl) sum += s.sPart[sl * Q.ldkT + kk];
        cl_store(slot + kk, sum, s.plain);
    }
    cl_publish(my_flag, epoch, tid, s.plain);
}

// consume the last hand-off: d[reads ; h]_{t-1} = the sum of the k partials in workgroup order (base: the k slots of this parity)
__device__ __forceinline__ void dncc_bwd_zprev_consume(const DncClBwdSt& s, const float* base, int slot, int k, int K) {
    for (int kk = s.tid; kk < K; kk += CT) {
        float pv[8];
#pragma unroll
        for (int gg = 0; gg < 8; ++gg) pv[gg] = (gg < k) ? cl_load(base + (size_t)gg * slot + kk) : 0.f;
        float sum = 0.f;
#pragma unroll
        for (int gg = 0; gg < 8; ++gg) if (gg < k) sum += pv[gg];
        s.sGZ[kk] = sum;
    }
}
