// What the four NTM sequence launchers (ntm_seq_fwd.hip with ntm_seq_fwd_ws.hip, ntm_seq_bwd.hip, ntm_seq_deep.hip) take and share
// on the host: the argument structs of the kernels, the pointer checks, the two LDS carve-ups, the BPTT workgroup-size rule, the plan
// structs and the kernel table a launch looks its instantiation up in.  The kernels read the structs by value: member order and types
// are part of the generated code.
#pragma once
#include "ntm_common.h"
#include <type_traits>

static inline NtmDims ntm_dims(int B, int S, int N, int Md, int R, int Wh, int hid, int shift_range, int O, int write_first, int similarity) {
    NtmDims d;
    ntm_fill_dims(d, B, S, N, Md, R, Wh, hid, shift_range, O, write_first, similarity);
    return d;
}

// ------------------------------------------------------------------------------------------------ single-layer passes
struct NtmFwdArgs {
    NtmDims d;
    // inputs
    const float* xproj;    // [B,S,4*hid]  X * Wx (columns n' = unit*4+gate), no bias
    const float* Wr;       // [ldz][4*hid]
    const float* Wa;       // [ldh][PP]
    const float* M0;       // [B,N,Md]
    const float* w0;       // [B,H,N]
    const float* read0;    // [B,R,Md]
    const float* cs0;      // [B,2*hid]  (c then h)
    // outputs
    float* logits;         // [B,S,O]
    float* outputs;        // [B,S,O] softmax(logits) or null
    float* M_out;          // [B,N,Md]
    float* w_out;          // [B,H,N]
    float* read_out;       // [B,R,Md]
    float* cs_out;         // [B,2*hid]
    // per-step records (all nullable): what LoopNTMTracker writes to its TensorArrays plus the BPTT stash
    float* st_z;           // [B,S,ldz]   step input [read_prev;h_prev;1;0..]
    float* st_gates;       // [B,S,4*hid] activated gates (i,j,f,o per unit)
    float* st_c;           // [B,S,hid]
    float* st_h;           // [B,S,ldh]   [h';1;0..]
    float* st_u;           // [B,S,PP]    activated controls, raw shift logits, raw output logits
    float* st_wc;          // [B,S,H,N]   content-focused weights
    float* st_wv;          // [B,S,H,N]   shifted weights (before sharpening)
    float* st_w;           // [B,S,H,N]
    float* st_M;           // [B,S,N,Md]
    float* st_read;        // [B,S,R,Md]
};

struct NtmBwdArgs {
    NtmDims d;
    const float* WrT;      // [4*hid][ldkT]  transposed recurrent weights (rows n' = unit*4+gate)
    const float* WaT;      // [PP][ldhT]     transposed unpack/output weights
    int ldkT, ldhT;
    const float* M0; const float* w0; const float* cs0;
    const float* st_gates; const float* st_c; const float* st_u;
    const float* st_wc; const float* st_wv; const float* st_w; const float* st_M;
    const float* dlogits;  // [B,S,O]
    const float* dM_fin; const float* dw_fin; const float* dread_fin; const float* dcs_fin;  // nullable
    float* dgates;         // [B,S,4*hid]
    float* du;             // [B,S,PP]
    float* dM0; float* dw0; float* dread0; float* dcs0;
};

// ------------------------------------------------------------------------------------------------ deep controller
// Packed layouts of the deep kernels (hid % 4 == 0, see ntk_ntm_seq_deep_supported)
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

static inline NtmDeepShape ntm_deep_shape(int D, int RM, int hid, int L) {
    NtmDeepShape s;
    s.D = D; s.RM = RM; s.hid = hid; s.L = L;
    s.ldx = ntm_align4(D);
    s.ld0 = ntm_align4(D + RM + hid + 1);
    s.ld1 = ntm_align4(2 * hid + 1);
    s.ldxt = ntm_align4(hid);
    s.rf0 = ntm_align4(RM + hid + 1);
    s.rf1 = ntm_align4(2 * hid + 1);
    s.cb0 = ntm_align4(RM + hid);
    s.cb1 = 2 * hid;
    return s;
}

// the deep forward takes an NtmFwdArgs (Wr, cs0, cs_out null: their deep forms are here) and this
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

struct NtmDeepBwdArgs {
    NtmDims d;
    NtmDeepShape s;
    const float* Wb;       // transposed recurrent blocks (above)
    const float* WaT;      // [PP][ldhT]
    int ldhT;
    const float* M0; const float* w0;
    const float* cs0;      // [B,2*hid*L]
    const float* st_gates; const float* st_c; const float* st_u;       // the top layer and the heads, as NtmBwdArgs
    const float* st_wc; const float* st_wv; const float* st_w; const float* st_M;
    const float* st_lgates; const float* st_lc;                        // [L-1][B,S,hid,4], [L-1][B,S,hid]
    const float* dlogits;  // [B,S,O]
    const float* dM_fin; const float* dw_fin; const float* dread_fin; const float* dcs_fin;     // nullable; dcs [B,2*hid*L]
    float* dgates;         // [B,S,4*hid]       top layer, n' = unit*4 + gate
    float* dpre;           // [L-1][B,S,4*hid]  layers 0..L-2, TF gate-major (g*hid + unit)
    float* du;             // [B,S,PP]
    float* dM0; float* dw0; float* dread0; float* dcs0;                // dcs0 [B,2*hid*L]
};

// ------------------------------------------------------------------------------------------------ pointer checks
// NTK_OK, or NTK_ERR_BAD_PTR with a message that starts with the entry's name.  Nullable: outputs, every st_* record of the forward
// (st_gates with st_c; st_buf0 needs X) and the four d*_fin of the BPTT.

// dp: the deep forward's second struct (its Wf / cs0 / cs_out stand for Wr / cs0 / cs_out), null for the single-layer forward
static inline int ntm_fwd_check_ptrs(const NtmFwdArgs& a, const NtmDeepFwdArgs* dp, const char* who) {
    const float* const W = dp ? dp->Wf : a.Wr;
    const float* const lgates = dp ? dp->st_lgates : nullptr;
    NTK_REQUIRE(a.xproj && W && a.Wa && a.M0 && a.w0 && a.read0 && (dp ? dp->cs0 : a.cs0) && a.logits && a.M_out && a.w_out && a.read_out &&
                    (dp ? dp->cs_out : a.cs_out),
                NTK_ERR_BAD_PTR, "%s: null pointer", who);
    NTK_REQUIRE(ntk_aligned16(a.xproj) && ntk_aligned16(W) && ntk_aligned16(a.Wa) && ntk_aligned16(a.st_gates) && ntk_aligned16(lgates),
                NTK_ERR_BAD_PTR, "%s: %s must be 16-byte aligned", who, dp ? "xproj/Wf/Wa/st_gates/st_lgates" : "xproj/Wr/Wa/st_gates");
    NTK_REQUIRE(!a.st_gates == !a.st_c, NTK_ERR_BAD_PTR, "%s: st_gates and st_c go together", who);
    NTK_REQUIRE(!dp || !dp->st_buf0 || dp->X, NTK_ERR_BAD_PTR, "%s: the st_buf0 record needs X", who);
    return NTK_OK;
}

// A: NtmBwdArgs or NtmDeepBwdArgs (which adds st_lgates, st_lc and dpre, and whose recurrent weights are Wb)
template <class A>
static inline int ntm_bwd_check_ptrs(const A& a, const char* who) {
    constexpr bool deep = std::is_same<A, NtmDeepBwdArgs>::value;
    const float* W;
    const float* lgates = nullptr;
    bool lower = true;
    if constexpr (deep) { W = a.Wb; lgates = a.st_lgates; lower = a.st_lgates && a.st_lc && a.dpre; }
    else W = a.WrT;
    NTK_REQUIRE(W && a.WaT && a.M0 && a.w0 && a.cs0 && a.st_gates && a.st_c && a.st_u && a.st_wc && a.st_wv && a.st_w && a.st_M && lower &&
                    a.dlogits && a.dgates && a.du && a.dM0 && a.dw0 && a.dread0 && a.dcs0,
                NTK_ERR_BAD_PTR, "%s: null pointer", who);
    NTK_REQUIRE(ntk_aligned16(W) && ntk_aligned16(a.WaT) && ntk_aligned16(a.st_gates) && ntk_aligned16(lgates) && ntk_aligned16(a.dgates),
                NTK_ERR_BAD_PTR, "%s: %s must be 16-byte aligned", who, deep ? "Wb/WaT/st_gates/st_lgates/dgates" : "WrT/WaT/st_gates/dgates");
    return NTK_OK;
}

// ------------------------------------------------------------------------------------------------ LDS carve-ups
// forward: layers = 1 is the single-layer kernels' (d.K = R*Md + hid); the deep kernels keep every layer's h behind the reads in Z and
// every layer's c in C
static inline void ntm_fwd_lds(const NtmDims& d, int T, NtmLds& L, int layers = 1) {
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
    L.Z = o; o += ntm_align4(RM + layers * d.hid);
    L.C = o; o += ntm_align4(layers * d.hid);
    L.U = o; o += ntm_align4(d.PP);
    L.Ks = o; o += ntm_align4(d.H * d.Md);
    L.Cn = o; o += ntm_align4(ntm_norm_floats(d));
    L.Pw = o; o += ntm_align4(d.H * d.N);
    L.total = o;
}

// floats of the partials of a product whose ld columns (float4 groups) are sliced over T threads
static inline int ntm_bwd_part_floats(int T, int ld) { return ntm_imax(1, T / (ld / 4)) * ld; }

// BPTT: what differs between the single-layer and the deep kernels is stated by the caller -- part_more, the largest of its own
// users of `part` beside the ones below (the products over its recurrent weights), and the floats of the carried dZ and dC
static inline void ntm_bwd_lds(const NtmDims& d, int T, int ldhT, int part_more, int dZ, int dC, NtmBwdLds& L) {
    const int MP = d.Md | 1, NM = d.N * MP, HN = d.H * d.N;
    const int nout = d.H * d.Md + 2 * d.Wh * d.Md;
    const int nslP = ntm_imin(ntm_imax(1, T / nout), d.N);
    const int nslC = ntm_imax(1, T / d.Md);
    int part = ntm_imax(nslP * nout, ntm_bwd_part_floats(T, ldhT));
    part = ntm_imax(part, nslC * d.Md);
    part = ntm_imax(part, part_more);
    int o = 0;
    auto take = [&](int n) { int r = o; o += ntm_align4(n); return r; };
    L.part = take(part);
    L.dM = take(NM); L.G = take(NM); L.Mp = take(NM); L.Mt = take(d.write_first ? NM : 4);
    L.dW = take(HN); L.Wp = take(HN); L.Wt = take(HN); L.Wc = take(HN); L.Wv = take(HN); L.Wg = take(HN);
    L.Dwv = take(HN); L.Dsim = take(HN);
    L.U = take(d.PP); L.DU = take(d.PP); L.DG = take(4 * d.hid); L.dZ = take(dZ); L.dC = take(dC);
    L.Gt = take(4 * d.hid); L.Ct = take(d.hid); L.Cp = take(d.hid);
    L.Khat = take(d.H * d.Md); L.Ks = take(d.H * d.Md); L.Kinv = take(d.H); L.Kss = take(d.H);
    L.Cinv = take(ntm_norm_floats(d)); L.Css = take(d.Md); L.C2 = take(ntm_norm_floats(d)); L.Dkhat = take(d.H * d.Md);
    L.Sw = take(d.H * d.SS);
    L.Red = take(d.H * (NQT + (d.similarity == NTM_SIM_SMOOTH_COSINE ? 1 : 0)) * (d.N / 64));
    L.Dmh = take(d.N * (d.Md | 1));
    L.total = o;
}

// BPTT workgroup size: whole waves over the heads' slots, the gate columns, the controls, the step input, the key / erase / add
// columns, and `more`, what the caller's kernel adds
static inline int ntm_bwd_threads(const NtmDims& d, int more) {
    int T = ntm_imax(d.H * d.N, 3 * d.hid);
    T = ntm_imax(T, d.PP);
    T = ntm_imax(T, d.K);
    T = ntm_imax(T, d.H * d.Md + d.Md + 2 * d.Wh * d.Md);
    T = ntm_imax(T, more);
    return ((T + 63) / 64) * 64;
}

// ------------------------------------------------------------------------------------------------ plans
// What a launcher does with a shape: every limit of its kernels and the kernel a shape takes, host arithmetic only, for the launcher
// and for the queries (ntk_ntm_seq_plan, ntk_ntm_seq_deep_plan) alike.
struct NtmFwdPlan {
    int kernel;            // NTK_NTM_FWD_*
    int T;                 // threads of the workgroup
    NtmLds L;
    size_t lds_bytes;
};
struct NtmBwdPlan {
    int kernel;            // NTK_NTM_BWD_*
    int T;                 // threads the shape's work is laid out over (NtmBwdLds)
    int threads;           // threads of the workgroup: T, or 768 in the wave-specialised form (two stream waves beside T = 640)
    NtmBwdLds L;
    size_t lds_bytes;
};
struct NtmDeepPlan {       // (the kernel ids: ntm_deep_kernel_id of Tf / Tb)
    int Tf, Tb;
    NtmLds Lf;
    NtmBwdLds Lb;
    size_t lds_f, lds_b;
};
int ntm_validate_dims(const NtmDims& d, const char* who);          // ntm_seq_fwd.hip
int ntm_fwd_plan(const NtmDims& d, NtmFwdPlan& p, const char* who);
int ntm_pick_threads(const NtmDims& d);           // workgroup size of the generic forward kernels, single-layer and deep (ntm_seq_fwd.hip)

// the single-layer launchers behind their plain, *_sim and step entries (ntm_seq_fwd.hip, ntm_seq_bwd.hip; step_api.hip calls them
// with S = 1)
int ntm_seq_fwd_run(const NtmFwdArgs& a, void* stream);
int ntm_seq_bwd_run(const NtmBwdArgs& a, void* stream);

// ------------------------------------------------------------------------------------------------ kernel tables
// One row per instantiation a launcher can take.  The launch looks (id, similarity) up and the LDS limit is raised on every row of
// the same table, so an instantiation cannot launch with the default limit.  A pair without a row (the wave-specialised ids in
// smooth-cosine mode) is NTK_ERR_UNSUPPORTED.
template <class Fn>
struct NtmKernelRow {
    int id, similarity;
    Fn fn;
};

template <class Fn, int NK>
static inline int ntm_find_kernel(NtkLdsAttrCache& cache, const NtmKernelRow<Fn> (&rows)[NK], int id, int similarity, const char* who, Fn& fn) {
    const void* ks[NK];
    for (int i = 0; i < NK; ++i) ks[i] = (const void*)rows[i].fn;
    const int rc = ntk_raise_lds_limit(cache, ks, NK, who);
    if (rc != NTK_OK) return rc;
    fn = nullptr;
    for (const NtmKernelRow<Fn>& r : rows)
        if (r.id == id && r.similarity == similarity) fn = r.fn;
    NTK_REQUIRE(fn, NTK_ERR_UNSUPPORTED, "%s: kernel %d has no smooth-cosine form", who, id);
    return NTK_OK;
}
