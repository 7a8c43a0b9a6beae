// NTM sequence forward: one persistent workgroup per sequence walks all S
// steps of NTMCell.__call__ (ntm_cell.py:53-253) with the whole recurrent state
// (memory N x Md, head weights H x N, reads, LSTM c/h) resident in LDS; only
// the weights are streamed (from L2) and the per-step tensors the BPTT pass
// needs are written once, coalesced, to HBM.  Replaces the tf.while_loop of
// LoopNTMTracker (ntm_tracker_new.py:13-64), S sequential TF graph iterations.
//
// Per step (all phases separated by workgroup barriers):
//   P1 gate partials      z=[read_prev;h_prev] (K) x Wr[K][4*hid]   (K-sliced over thread groups)
//   P2 LSTM cell          BasicLSTMCell, gate order i,j,f,o, forget_bias 0 (ntm_cell.py:45-50)
//                         || the other waves l2-normalise the feature columns of M over the slots (quirk Q1)
//                         (SIM = smooth cosine: they take the N row norms |M[n]| instead)
//   P3 unpack partials    h' x Wa[hid][PP]                           (ntm_cell.py:124-126, :220)
//   P4 control activations tanh/softplus/sigmoid/1+softplus           (:133,140,151,169,193,195)
//   P5-P7 ONE WAVE PER HEAD, no workgroup barrier: key scaling, shift softmax (ops.py:150-152, ntm_cell.py:161),
//      similarity (Q1: feature columns normalised over slots; SIM = smooth cosine: k.M[n] / (|k||M[n]| + 1e-3), the
//      content addressing of the reference's ops_test.py), beta, softmax over N, gate (:136-156),
//      circular shift with taps -(r+1)..r-1 (Q2), sharpen with +1e-3 (Q4)   (ops.py:204-213, ntm_cell.py:173-176)
//   P8 erase/add write and read (reads see the pre-write memory unless write_first, Q6) (:202-215)
//
// P2's normaliser and P3 .. P8 are the phase functions of ntm_phases.h, shared with ntm_seq_fwd_ws.hip and ntm_seq_deep.hip; the
// barriers between them stay here.  This file's own: the gate product P1 with its resident rows and rolling prefetch, the LSTM
// cell of P2, the initial / final state, the plan (ntm_fwd_plan, ntm_pick_threads, ntm_validate_dims) and the launcher.  The argument
// struct, the pointer check and the LDS carve-up are in ntm_seq_args.h.
#include "ntm_common.h"

// Diagnostic build only (-DNTK_CL_PROF): s_memtime shares per phase, accumulated in LDS by thread 0 of workgroup 0
#ifdef NTK_CL_PROF
__device__ unsigned long long g_ntm_fwd_prof[16];
#define NTM_STAMP(i)                                                        \
    do {                                                                    \
        if (blockIdx.x == 0 && tid == 0) {                                  \
            const unsigned long long now_ = __builtin_amdgcn_s_memtime();   \
            s_prof[i] += now_ - s_prof[15];                                 \
            s_prof[15] = now_;                                              \
        }                                                                   \
    } while (0)
extern "C" int ntk_ntm_fwd_prof(unsigned long long* out16) {
    return hipMemcpyFromSymbol(out16, HIP_SYMBOL(g_ntm_fwd_prof), 16 * sizeof(unsigned long long)) == hipSuccess ? NTK_OK : NTK_ERR_HIP;
}
#else
#define NTM_STAMP(i) do { } while (0)
#endif

#include "ntm_phases.h"
#include <stdlib.h>

// FIX = true specialises every dimension to the reference defaults the benchmark configs run
// (direct_offset_output.py:21-27: mem 128x20, hidden 200, 4 read + 1 write heads, shift_range 1,
// output_dim 2, 640 threads): index arithmetic constant-folds and the small loops unroll.
// FIXT = 512 with NTM_RES_REG / NTM_RES_LDS > 0 is the same specialisation with RESIDENT gate weights: 512 threads leave a
// thread 256 registers, and 44 of the 140 rows of Wr a thread multiplies per step (one float4 gate column of its unit x half
// of K) stay on the CU for the whole sequence -- 24 rows in registers, 20 in the 128 KB of LDS the state leaves free --
// instead of streaming from L2 every step.  The stream of the remaining rows is requested first and lands while the
// resident rows are multiplied; the products are summed in the same order as before.  Measured (scripts/dev_ntm_prof.py,
// dev_ntm_timing.py): the gate stream is 51 % of a forward step and runs at the ~100 GB/s one CU draws from L2 however
// deep the prefetch (16 or 24 rows per thread in flight: the same) and however lean the loop (a guard-free form with
// scalar row bases: the same) -- only fewer bytes help: 912 -> 614 KB per step, forward 21.6 -> 20.3 ms at B32 x S1300.
// LDS rows alone at 640 threads gave nothing (the other phases lose at 512 threads what 14 % fewer bytes win).
// SIM (NTM_SIM_*) is the similarity of the content addressing, a compile-time mode: the as-coded instantiations are the
// kernels they were, the smooth-cosine ones differ in P2's normaliser (N row norms where the Md column norms were) and in the
// head waves' key and similarity.
template <int MAXT, int FIXT, int NTM_RES_REG = 0, int NTM_RES_LDS = 0, int SIM = NTM_SIM_AS_CODED>
__global__ __launch_bounds__(MAXT) void ntm_seq_fwd_kernel(NtmFwdArgs a, NtmLds L) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    constexpr bool FIX = FIXT != 0, RES = NTM_RES_REG + NTM_RES_LDS > 0, SMOOTH = SIM == NTM_SIM_SMOOTH_COSINE;
    const int b = blockIdx.x, tid = threadIdx.x, T = FIX ? FIXT : blockDim.x;
    const int N = FIX ? 128 : a.d.N, Md = FIX ? 20 : a.d.Md, MP = Md | 1, R = FIX ? 4 : a.d.R, Wh = FIX ? 1 : a.d.Wh;
    const int H = R + Wh, hid = FIX ? 200 : a.d.hid, SS = FIX ? 3 : a.d.SS;
    const int S = a.d.S, RM = R * Md, K = RM + hid;
    const NtmCtl d = ntm_ctl(Md, R, Wh, hid, SS, FIX ? 2 : a.d.O, a.d.write_first);
    const int PP = d.PP;
    const NtmFwdSt c = ntm_fwd_state(smem, L, T, N, Md, R, Wh, hid, SS, PP, RM);      // LDS pointers + decomposition of P3 .. P8
    float* const sPart = c.sPart; float* const sM = c.sM; float* const sW = c.sW; float* const sZ = c.sZ;
    float* const sC = smem + L.C;

    // K-slices of the gate product (uniform per kernel)
    const int nsl = max(1, T / hid);
    const int kper = (K + nsl - 1) / nsl;

    // ---- load the initial state
    for (int i = tid; i < N * Md; i += T) sM[(i / Md) * MP + (i % Md)] = a.M0[(size_t)b * N * Md + i];
    for (int i = tid; i < H * N; i += T) sW[i] = a.w0[(size_t)b * H * N + i];
    for (int i = tid; i < RM; i += T) sZ[i] = a.read0[(size_t)b * RM + i];
    for (int i = tid; i < hid; i += T) {
        sC[i] = a.cs0[(size_t)b * 2 * hid + i];
        sZ[RM + i] = a.cs0[(size_t)b * 2 * hid + hid + i];
    }
    __syncthreads();

    const f32x4* Wr4 = reinterpret_cast<const f32x4*>(a.Wr);
    const f32x4* Wa4 = reinterpret_cast<const f32x4*>(a.Wa);
    f32x4* sPart4 = reinterpret_cast<f32x4*>(sPart);

    const int tid0 = tid;
    f32x4 wres[NTM_RES_REG > 0 ? NTM_RES_REG : 1];
    const f32x4* sWres4 = reinterpret_cast<const f32x4*>(smem + L.total + 32);     // [NTM_RES_LDS][nsl * hid] behind the state (+ the diagnostic words)
    if constexpr (RES) {
        if (tid < nsl * hid) {
            const int j = tid % hid, ks = tid / hid, k0 = ks * kper;
#pragma unroll
            for (int q = 0; q < NTM_RES_REG; ++q) wres[q] = Wr4[(size_t)min(k0 + q, a.d.ldz - 1) * hid + j];
            f32x4* wl = reinterpret_cast<f32x4*>(smem + L.total + 32);
            for (int q = 0; q < NTM_RES_LDS; ++q) wl[q * (nsl * hid) + tid] = Wr4[(size_t)min(k0 + NTM_RES_REG + q, a.d.ldz - 1) * hid + j];
        }
        __syncthreads();
    }
#ifdef NTK_CL_PROF
    unsigned long long* s_prof = reinterpret_cast<unsigned long long*>(smem + L.total);      // 128 B behind the state (the launch adds them)
    if (tid == 0) { for (int i = 0; i < 15; ++i) s_prof[i] = 0; s_prof[15] = __builtin_amdgcn_s_memtime(); }
#endif
    for (int t = 0; t < S; ++t) {
        // re-derive every thread-index expression inside the step: an opaque copy of the thread id keeps
        // the compiler from hoisting dozens of loop-invariant addresses out of the t-loop and spilling them
        int tid_op = tid0;
        asm volatile("" : "+v"(tid_op));
        const int tid = tid_op;
        const int lane = tid & 63;
        const size_t bt = (size_t)b * S + t;
        // ------------------------------------------------------------ P1
        f32x4 xg = {0.f, 0.f, 0.f, 0.f};
        if (tid < hid) {   // prefetch this step's input projection + LSTM bias (row K of Wr)
            xg = reinterpret_cast<const f32x4*>(a.xproj)[bt * hid + tid];
            const f32x4 bb = Wr4[(size_t)K * hid + tid];
            xg += bb;
        }
        if (a.st_z) {
            for (int i = tid; i < d.ldz; i += T)
                a.st_z[bt * d.ldz + i] = (i < K) ? sZ[i] : (i == K ? 1.f : 0.f);
        }
        if (tid < nsl * hid) {
            const int j = tid % hid, ks = tid / hid;
            const int k0 = ks * kper, k1 = min(K, k0 + kper);
            f32x4 acc = {0.f, 0.f, 0.f, 0.f};
            const f32x4* wp = Wr4 + j;
            // rolling prefetch: two register batches of 8 rows keep >= 8 x 16 B per thread in flight from L2
            constexpr int PF = 8;
            f32x4 wa[PF], wb[PF];
            const int klast = a.d.ldz - 1;          // last row of the Wr allocation (a zero pad row)
            const int ks0 = RES ? min(k1, k0 + NTM_RES_REG + NTM_RES_LDS) : k0;      // first streamed row
#pragma unroll
            for (int q = 0; q < PF; ++q) wa[q] = wp[(size_t)min(ks0 + q, klast) * hid];
#pragma unroll
            for (int q = 0; q < PF; ++q) wb[q] = wp[(size_t)min(ks0 + PF + q, klast) * hid];
            if constexpr (RES) {                    // the resident rows, while the first streamed batches are in flight
#pragma unroll
                for (int q = 0; q < NTM_RES_REG; ++q) acc += ((k0 + q < k1) ? sZ[k0 + q] : 0.f) * wres[q];
#pragma unroll 4
                for (int q = 0; q < NTM_RES_LDS; ++q)
                    acc += ((k0 + NTM_RES_REG + q < k1) ? sZ[k0 + NTM_RES_REG + q] : 0.f) * sWres4[q * (nsl * hid) + tid];
            }
#pragma nounroll
            for (int k = ks0; k < k1; k += 2 * PF) {
#pragma unroll
                for (int q = 0; q < PF; ++q) {
                    const float zk = (k + q < k1) ? sZ[k + q] : 0.f;
                    acc += zk * wa[q];
                }
#pragma unroll
                for (int q = 0; q < PF; ++q) wa[q] = wp[(size_t)min(k + 2 * PF + q, klast) * hid];
#pragma unroll
                for (int q = 0; q < PF; ++q) {
                    const float zk = (k + PF + q < k1) ? sZ[k + PF + q] : 0.f;
                    acc += zk * wb[q];
                }
#pragma unroll
                for (int q = 0; q < PF; ++q) wb[q] = wp[(size_t)min(k + 3 * PF + q, klast) * hid];
            }
            sPart4[ks * hid + j] = acc;
        }
        __syncthreads();
        NTM_STAMP(0);
        // ------------------------------------------------------------ P2: LSTM cell  ||  column norms of M (Q1)
        const int wave = tid >> 6;
        if (tid < hid) {
            f32x4 g = xg;
            for (int ks = 0; ks < nsl; ++ks) g += sPart4[ks * hid + tid];
            const float gi = ntm_sigmoid(g[0]);
            const float gj = ntm_tanh(g[1]);
            const float gf = ntm_sigmoid(g[2]);      // forget_bias = 0.0 (ntm_cell.py:47)
            const float go = ntm_sigmoid(g[3]);
            const float c2 = sC[tid] * gf + gi * gj;
            const float h2 = ntm_tanh(c2) * go;
            sC[tid] = c2;
            sZ[RM + tid] = h2;
            if (a.st_gates) {
                f32x4 ga = {gi, gj, gf, go};
                reinterpret_cast<f32x4*>(a.st_gates)[bt * hid + tid] = ga;
                a.st_c[bt * hid + tid] = c2;
            }
            if (a.st_h) a.st_h[bt * d.ldh + tid] = h2;
        } else if (a.st_h && tid < d.ldh) {
            a.st_h[bt * d.ldh + tid] = (tid == hid) ? 1.f : 0.f;
        }
        ntm_fwd_mem_norms<SMOOTH>(c, tid);       // the waves not running the LSTM
        __syncthreads();
        NTM_STAMP(1);
        // ------------------------------------------------------------ P3: unpack / output partials
        ntm_fwd_unpack_partials<(MAXT > 768 ? 2 : 4)>(c, d, Wa4, tid);
        __syncthreads();
        NTM_STAMP(2);
        // ------------------------------------------------------------ P4: control activations
        ntm_fwd_controls(c, d, a, tid, bt);
        __syncthreads();
        NTM_STAMP(3);
        // ------------------------------------------------------------ P5-P7: one WAVE per head, no workgroup barrier inside;
        // the wave behind them takes the softmax of the output logits
        constexpr int MAXSS = FIX ? 3 : NTM_MAX_SHIFT_TAPS;         // (a compile-time 3 taps at the benchmark shape)
        if (wave < H) ntm_fwd_head_wave<SMOOTH, MAXSS>(c, d, a, wave, lane, bt);
        else if (wave == H && lane == 0 && a.outputs) ntm_fwd_output_softmax(c, d, a, bt);
        __syncthreads();
        NTM_STAMP(4);
        // ------------------------------------------------------------ P8: write + read
        if (d.write_first) { ntm_fwd_update_M(c, d, a, tid, bt); __syncthreads(); }
        ntm_fwd_read_partials(c, tid);
        __syncthreads();
        NTM_STAMP(5);
        if (!d.write_first) ntm_fwd_update_M(c, d, a, tid, bt);
        ntm_fwd_read_finish(c, a, tid, bt);
        __syncthreads();
        NTM_STAMP(6);
    }
#ifdef NTK_CL_PROF
    if (blockIdx.x == 0 && tid == 0) for (int i = 0; i < 16; ++i) g_ntm_fwd_prof[i] = s_prof[i];
#endif

    // ---- final state
    for (int i = tid; i < N * Md; i += T) a.M_out[(size_t)b * N * Md + i] = sM[(i / Md) * MP + (i % Md)];
    for (int i = tid; i < H * N; i += T) a.w_out[(size_t)b * H * N + i] = sW[i];
    for (int i = tid; i < RM; i += T) a.read_out[(size_t)b * RM + i] = sZ[i];
    for (int i = tid; i < hid; i += T) {
        a.cs_out[(size_t)b * 2 * hid + i] = sC[i];
        a.cs_out[(size_t)b * 2 * hid + hid + i] = sZ[RM + i];
    }
}

// pick the workgroup size: whole waves, enough threads for N slots x >=1 head, hid units + Md columns
// (the deep kernels' forward takes the same size, ntm_seq_deep.hip)
int ntm_pick_threads(const NtmDims& d) {
    int want = ntm_imax(d.H * d.N, 3 * d.hid);
    want = ntm_imax(want, d.hid + ntm_imax(d.Md, 4));
    want = ntm_imax(want, d.PP + d.Md);
    want = ntm_imax(want, d.H * d.Md + d.H + 1);
    want = ntm_imax(want, ((d.hid + 63) / 64 + 1) * 64);
    want = ntm_imax(want, (d.H + 1) * 64);
    want = ((want + 63) / 64) * 64;
    if (want > 1024) want = 1024;
    return want;
}

bool ntm_seq_fwd_ws_takes(const NtmDims& d);                        // ntm_seq_fwd_ws.hip
int ntm_seq_fwd_ws_plan(const NtmDims& d, NtmLds& L, size_t& lds_bytes);
int ntm_seq_fwd_ws_launch(const NtmFwdArgs& a, const NtmLds& L, size_t lds_bytes, void* stream);

int ntm_validate_dims(const NtmDims& d, const char* who) {
    NTK_REQUIRE(d.B > 0 && d.S > 0, NTK_ERR_BAD_SHAPE, "%s: B=%d S=%d", who, d.B, d.S);
    NTK_REQUIRE(d.N >= 64 && (d.N % 64) == 0 && d.N <= 1024, NTK_ERR_UNSUPPORTED,
                "%s: mem_size=%d must be a multiple of 64 in [64,1024]", who, d.N);
    NTK_REQUIRE(d.Md >= 1 && d.Md <= 256, NTK_ERR_UNSUPPORTED, "%s: mem_dim=%d out of range", who, d.Md);
    NTK_REQUIRE(d.R >= 1 && d.Wh >= 1, NTK_ERR_BAD_SHAPE, "%s: need >=1 read and write head (R=%d W=%d)", who, d.R, d.Wh);
    NTK_REQUIRE(d.hid >= 1 && d.hid + d.Md <= 1024 && d.PP + d.Md <= 1024 && d.H * d.Md + d.H + 1 <= 1024 &&
                    d.R * d.Md <= 1024,
                NTK_ERR_UNSUPPORTED, "%s: hidden=%d heads=%d mem_dim=%d exceed one workgroup", who, d.hid, d.H, d.Md);
    NTK_REQUIRE(d.SS >= 1 && d.SS < d.N && d.O >= 1, NTK_ERR_BAD_SHAPE, "%s: shift space %d / output_dim %d", who, d.SS, d.O);
    // limits of the kernels' fixed decomposition: shift taps live in a register array of NTM_MAX_SHIFT_TAPS (9: shift_range <= 4),
    // addressing runs one WAVE per head, and the column norms of M need one wave beyond those of the hidden units
    NTK_REQUIRE(d.SS <= NTM_MAX_SHIFT_TAPS, NTK_ERR_UNSUPPORTED, "%s: shift_range=%d (shift space %d > %d taps)", who, (d.SS - 1) / 2, d.SS,
                NTM_MAX_SHIFT_TAPS);
    NTK_REQUIRE((d.H + 1) * 64 <= 1024, NTK_ERR_UNSUPPORTED, "%s: %d heads (one wave per head: at most 15)", who, d.H);
    NTK_REQUIRE(((d.hid + 63) / 64 + 1) * 64 <= 1024, NTK_ERR_UNSUPPORTED, "%s: hidden=%d (at most 960)", who, d.hid);
    return NTK_OK;
}

// every limit of the forward kernels and the kernel a shape takes, host arithmetic only
int ntm_fwd_plan(const NtmDims& d, NtmFwdPlan& p, const char* who) {
    int rc = ntm_validate_dims(d, who);
    if (rc != NTK_OK) return rc;
    // benchmark shape: the kernel whose recurrent weight stream runs beside the step instead of in front of it (ntm_seq_fwd_ws.hip;
    // NTK_NTM_FWD_FORM=res selects round 2's resident-rows kernel below, for comparison)
    const char* form_env = getenv("NTK_NTM_FWD_FORM");               // read per call (development switch)
    const bool ws_off = form_env && form_env[0] == 'r';
    if (!ws_off && d.similarity == NTM_SIM_AS_CODED && ntm_seq_fwd_ws_takes(d)) {      // (no wave-specialised smooth-cosine form)
        p.kernel = NTK_NTM_FWD_WS;
        p.T = ntm_seq_fwd_ws_plan(d, p.L, p.lds_bytes);
    } else {
        p.T = ntm_pick_threads(d);
        NTK_REQUIRE(p.T >= d.N, NTK_ERR_UNSUPPORTED, "%s: mem_size %d exceeds the workgroup", who, d.N);
        const bool fixdims = (d.N == 128 && d.Md == 20 && d.R == 4 && d.Wh == 1 && d.hid == 200 && d.SS == 3 && d.O == 2);
#ifdef NTK_NTM_FWD_STREAM_ONLY                                              // dev build: the all-streaming 640-thread specialisation of round 1
        p.kernel = (fixdims && p.T == 640) ? NTK_NTM_FWD_FIX640_DEV : 0;
#else
        p.kernel = fixdims ? NTK_NTM_FWD_FIX512 : 0;
#endif
        if (p.kernel == NTK_NTM_FWD_FIX512) p.T = 512;
        if (p.kernel == 0) p.kernel = p.T <= 768 ? NTK_NTM_FWD_GENERIC768 : NTK_NTM_FWD_GENERIC1024;
        ntm_fwd_lds(d, p.T, p.L);
        p.lds_bytes = (size_t)p.L.total * sizeof(float) + 128;                   // + the diagnostic build's stamp words
        if (p.kernel == NTK_NTM_FWD_FIX512) p.lds_bytes += (size_t)20 * 2 * d.hid * sizeof(f32x4);
    }
    NTK_REQUIRE(p.lds_bytes <= 160 * 1024, NTK_ERR_UNSUPPORTED, "%s: state needs %zu B of LDS (> 160 KiB)", who, p.lds_bytes);
    return NTK_OK;
}

extern "C" int ntk_ntm_padded_dims(int N, int Md, int R, int Wh, int hid, int shift_range, int O,
                                   int* P, int* PP, int* K, int* ldz, int* ldh) {
    NtmDims d;
    ntm_fill_dims(d, 1, 1, N, Md, R, Wh, hid, shift_range, O, 0);
    if (P) *P = d.P;
    if (PP) *PP = d.PP;
    if (K) *K = d.K;
    if (ldz) *ldz = d.ldz;
    if (ldh) *ldh = d.ldh;
    return NTK_OK;
}

// ntk_ntm_seq_fwd behind its plain, *_sim and step entries: similarity, then shape and plan, then pointers, then the launch
int ntm_seq_fwd_run(const NtmFwdArgs& a, void* stream) {
    const char* who = "ntk_ntm_seq_fwd";
    NTM_REQUIRE_SIMILARITY(a.d.similarity, who);
    NtmFwdPlan p;
    int rc = ntm_fwd_plan(a.d, p, who);
    if (rc != NTK_OK) return rc;
    rc = ntm_fwd_check_ptrs(a, nullptr, who);
    if (rc != NTK_OK) return rc;
    if (p.kernel == NTK_NTM_FWD_WS) return ntm_seq_fwd_ws_launch(a, p.L, p.lds_bytes, stream);
    typedef void (*kern_t)(NtmFwdArgs, NtmLds);
    constexpr int AC = NTM_SIM_AS_CODED, SC = NTM_SIM_SMOOTH_COSINE;
    static const NtmKernelRow<kern_t> rows[] = {
        {NTK_NTM_FWD_FIX512, AC, ntm_seq_fwd_kernel<512, 512, 24, 20>},      {NTK_NTM_FWD_FIX512, SC, ntm_seq_fwd_kernel<512, 512, 24, 20, SC>},
        {NTK_NTM_FWD_GENERIC768, AC, ntm_seq_fwd_kernel<768, 0>},            {NTK_NTM_FWD_GENERIC768, SC, ntm_seq_fwd_kernel<768, 0, 0, 0, SC>},
        {NTK_NTM_FWD_GENERIC1024, AC, ntm_seq_fwd_kernel<1024, 0>},          {NTK_NTM_FWD_GENERIC1024, SC, ntm_seq_fwd_kernel<1024, 0, 0, 0, SC>},
        {NTK_NTM_FWD_FIX640_DEV, AC, ntm_seq_fwd_kernel<768, 640>}};         // (planned by the NTK_NTM_FWD_STREAM_ONLY build only)
    static NtkLdsAttrCache lds_cache;
    kern_t fn;
    rc = ntm_find_kernel(lds_cache, rows, p.kernel, a.d.similarity, who, fn);
    if (rc != NTK_OK) return rc;
    fn<<<a.d.B, p.T, p.lds_bytes, (hipStream_t)stream>>>(a, p.L);
    NTK_CHECK_LAUNCH(who);
    return NTK_OK;
}

extern "C" int ntk_ntm_seq_fwd_sim(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O,
                               int write_first, int similarity,
                               const float* xproj, const float* Wr, const float* Wa,
                               const float* M0, const float* w0, const float* read0, const float* cs0,
                               float* logits, float* outputs,
                               float* M_out, float* w_out, float* read_out, float* cs_out,
                               float* st_z, float* st_gates, float* st_c, float* st_h, float* st_u,
                               float* st_wc, float* st_wv, float* st_w, float* st_M, float* st_read,
                               void* stream) {
    return ntm_seq_fwd_run({ntm_dims(B, S, N, Md, R, Wh, hid, shift_range, O, write_first, similarity), xproj, Wr, Wa, M0, w0, read0, cs0,
                            logits, outputs, M_out, w_out, read_out, cs_out, st_z, st_gates, st_c, st_h, st_u, st_wc, st_wv, st_w, st_M,
                            st_read}, stream);
}

extern "C" int ntk_ntm_seq_fwd(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O,
                               int write_first,
                               const float* xproj, const float* Wr, const float* Wa,
                               const float* M0, const float* w0, const float* read0, const float* cs0,
                               float* logits, float* outputs,
                               float* M_out, float* w_out, float* read_out, float* cs_out,
                               float* st_z, float* st_gates, float* st_c, float* st_h, float* st_u,
                               float* st_wc, float* st_wv, float* st_w, float* st_M, float* st_read,
                               void* stream) {
    return ntm_seq_fwd_run({ntm_dims(B, S, N, Md, R, Wh, hid, shift_range, O, write_first, NTM_SIM_AS_CODED), xproj, Wr, Wa, M0, w0, read0,
                            cs0, logits, outputs, M_out, w_out, read_out, cs_out, st_z, st_gates, st_c, st_h, st_u, st_wc, st_wv, st_w,
                            st_M, st_read}, stream);
}
