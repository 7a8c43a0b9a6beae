// Shared definitions of the DNC sequence kernels (forward and BPTT).
// Packed parameter layouts: see include/ntmtrack.h (ntk_dnc_seq_fwd).
#pragma once
#include "common.h"
#include <initializer_list>

struct DncDims {
    int B, S, N, W, R, Wn, hid, O;
    int I, IP;       // interface width, padded
    int K, ldz;      // R*W + hid, padded K+1
    int ldh;         // padded hid+1
    int Ky, ldy, OP; // hid + R*W, padded Ky+1, padded O
    float clip;
    // interface offsets
    int oV, oE, oF, oAg, oWg, oRm, oKw, oBw, oKr, oBr;
};

static constexpr __host__ __device__ void dnc_fill_dims(DncDims& d, int B, int S, int N, int W, int R, int Wn, int hid, int O, float clip) {
    d.B = B; d.S = S; d.N = N; d.W = W; d.R = R; d.Wn = Wn; d.hid = hid; d.O = O; d.clip = clip;
    d.oV = 0;
    d.oE = d.oV + Wn * W;
    d.oF = d.oE + Wn * W;
    d.oAg = d.oF + R;
    d.oWg = d.oAg + Wn;
    d.oRm = d.oWg + Wn;
    d.oKw = d.oRm + R * (1 + 2 * Wn);
    d.oBw = d.oKw + Wn * W;
    d.oKr = d.oBw + Wn;
    d.oBr = d.oKr + R * W;
    d.I = d.oBr + R;
    d.IP = (d.I + 3) & ~3;
    d.K = R * W + hid;
    d.ldz = (d.K + 1 + 3) & ~3;
    d.ldh = (hid + 1 + 3) & ~3;
    d.Ky = hid + R * W;
    d.ldy = (d.Ky + 1 + 3) & ~3;
    d.OP = (O + 3) & ~3;
}

// First base of the one-workgroup kernels' argument structs: the dimensions stay ahead of the pointers in the kernarg segment
// (with the pointers first dnc_seq_fwd_kernel took one more VGPR).
struct DncDimsFirst {
    DncDims d;
};

// What a forward launch takes, in the order of the C entry points.  The six `extern "C"` launchers build their pack once,
// by aggregate initialisation from their parameters; the *Args structs of the kernels derive from it.
struct DncFwdPtrs {
    const float* xproj;   // [B,S,4*hid] (n' = unit*4+gate), no bias
    const float* Wr;      // [ldz][4*hid], row K = bias
    const float* Wi;      // [ldh][IP],   row hid = bias
    const float* Wy;      // [ldy][OP],   row Ky = bias
    // state, updated in place
    float* mem;           // [B,N,W]
    float* link;          // [B,Wn,N,N]
    float* usage;         // [B,N]
    float* rw;            // [B,R,N]
    float* ww;            // [B,Wn,N]
    float* prec;          // [B,Wn,N]
    float* reads;         // [B,R,W]    (access_output)
    float* hc;            // [B,2*hid]  (hidden then cell)
    float* out;           // [B,S,O]
    // per-step records for BPTT (all nullable, all-or-none)
    float* rec_z;         // [B,S,ldz]  [reads_prev ; h_prev ; 1 ; 0..]
    float* rec_gates;     // [B,S,4*hid] activated gates (i, j, sigmoid(f+1), o per unit)
    float* rec_c;         // [B,S,hid]  cell before clipping
    float* rec_hc;        // [B,S,ldh]  [clipped h ; 1 ; 0..]
    float* rec_yin;       // [B,S,ldy]  [clipped h ; reads_t ; 1 ; 0..]
    float* rec_ifc;       // [B,S,IP]   activated interface
    float* rec_u;         // [B,S,N]
    float* rec_ww;        // [B,S,Wn,N]
    float* rec_rw;        // [B,S,R,N]
    float* rec_cw;        // [B,S,Wn,N]
    float* rec_cr;        // [B,S,R,N]
    float* rec_al;        // [B,S,Wn,N] allocation weights
    float* rec_p;         // [B,S,Wn,N] precedence after the step
    float* rec_fwd;       // [B,S,R,Wn,N]
    float* rec_bwd;       // [B,S,R,Wn,N]
    float* rec_M;         // [B,S,N,W]
    float* rec_L;         // [B,S,Wn,N,N]
    float* rec_ypre;      // [B,S,O]    output before clipping
};

// What a BPTT launch takes, in the order of the C entry points; the integers between them (ldkT, ldhT, carry_in) stay with
// the *BwdArgs structs.  State and records as the forward pack lays them out.
struct DncBwdPtrs {
    const float* WrT;                // [4*hid][ldkT]
    const float* Wi;                 // cluster forms: [ldh][IP] as the forward takes it; one workgroup per sequence: its transpose WiT [IP][ldhT]
    const float* Wy;                 // [ldy][OP]
    const float* mem0; const float* link0; const float* usage0; const float* rw0; const float* ww0;
    const float* prec0; const float* hc0;
    const float* rec_gates; const float* rec_c; const float* rec_ifc; const float* rec_u; const float* rec_ww;
    const float* rec_rw; const float* rec_cw; const float* rec_cr; const float* rec_al; const float* rec_p;
    const float* rec_fwd; const float* rec_bwd; const float* rec_M; const float* rec_L; const float* rec_ypre;
    const float* dout;               // [B,S,O]
    float* gM; float* gL;            // [B,N,W], [B,Wn,N,N] zero-initialised scratch (carried gradients)
    float* dgates; float* dxi; float* dypre;
    float* gcarry;                   // nullable: [B, (Wn+1)*N + R*N + ldkT + hid] gradients carried into state t=-1 (segmented BPTT)
};

// Pointer checks of the six launchers: `required` non-null, `records` all given or none, `aligned16` 16-byte aligned (a null
// pointer passes: absent records, no workspace).  NTK_OK, or NTK_ERR_BAD_PTR with a message that starts with the entry's name.
static inline int dnc_check_ptr_sets(const char* who, std::initializer_list<const void*> required,
                                     std::initializer_list<const void*> records, std::initializer_list<const void*> aligned16) {
    for (const void* p : required) NTK_REQUIRE(p != nullptr, NTK_ERR_BAD_PTR, "%s: null pointer", who);
    int nn = 0;
    for (const void* p : records) nn += (p != nullptr);
    NTK_REQUIRE(nn == 0 || nn == (int)records.size(), NTK_ERR_BAD_PTR, "%s: record pointers are all-or-none (%d of %d given)", who, nn,
                (int)records.size());
    for (const void* p : aligned16) NTK_REQUIRE(ntk_aligned16(p), NTK_ERR_BAD_PTR, "%s: 16-byte alignment", who);
    return NTK_OK;
}
// The sets of a pack.  clustered: the entry takes a workspace (required, 16-byte aligned); the others pass none.
static inline int dnc_fwd_check_ptrs(const char* who, const DncFwdPtrs& p, bool clustered, const void* workspace) {
    NTK_REQUIRE(workspace || !clustered, NTK_ERR_BAD_PTR, "%s: null pointer", who);
    return dnc_check_ptr_sets(who, {p.xproj, p.Wr, p.Wi, p.Wy, p.mem, p.link, p.usage, p.rw, p.ww, p.prec, p.reads, p.hc, p.out},
                              {p.rec_z, p.rec_gates, p.rec_c, p.rec_hc, p.rec_yin, p.rec_ifc, p.rec_u, p.rec_ww, p.rec_rw, p.rec_cw,
                               p.rec_cr, p.rec_al, p.rec_p, p.rec_fwd, p.rec_bwd, p.rec_M, p.rec_L, p.rec_ypre},
                              {p.xproj, p.Wr, p.Wi, p.mem, p.link, p.rec_gates, p.rec_M, p.rec_L, workspace});
}
static inline int dnc_bwd_check_ptrs(const char* who, const DncBwdPtrs& p, bool clustered, const void* workspace) {      // gcarry: nullable
    NTK_REQUIRE(workspace || !clustered, NTK_ERR_BAD_PTR, "%s: null pointer", who);
    return dnc_check_ptr_sets(who, {p.WrT, p.Wi, p.Wy, p.mem0, p.link0, p.usage0, p.rw0, p.ww0, p.prec0, p.hc0, p.rec_gates, p.rec_c,
                                    p.rec_ifc, p.rec_u, p.rec_ww, p.rec_rw, p.rec_cw, p.rec_cr, p.rec_al, p.rec_p, p.rec_fwd, p.rec_bwd,
                                    p.rec_M, p.rec_L, p.rec_ypre, p.dout, p.gM, p.gL, p.dgates, p.dxi, p.dypre},
                              {}, {p.WrT, p.Wi, p.rec_gates, p.rec_M, p.rec_L, p.gM, p.gL, p.dgates, p.mem0, p.link0, workspace});
}

constexpr int DT = 1024;      // threads per workgroup
constexpr int DW = DT / 64;   // waves

__device__ __forceinline__ float dnc_sigmoid(float x) { return 1.0f / (1.0f + expf(-x)); }
__device__ __forceinline__ float dnc_softplus(float x) { return fmaxf(x, 0.f) + log1pf(expf(-fabsf(x))); }
__device__ __forceinline__ float dnc_clip(float x, float c) { return c > 0.f ? fminf(fmaxf(x, -c), c) : x; }

// in-place softmax of H rows of length N held in LDS; wave w owns rows w, w+DW, ... (no block barrier inside)
__device__ __forceinline__ void lds_softmax_rows(float* v, int H, int N, int wave, int lane) {
    for (int h = wave; h < H; h += DW) {
        float* r = v + h * N;
        float mx = -INFINITY;
        for (int n = lane; n < N; n += 64) mx = fmaxf(mx, r[n]);
        mx = wave_max(mx);
        float s = 0.f;
        for (int n = lane; n < N; n += 64) { const float e = expf(r[n] - mx); r[n] = e; s += e; }
        s = wave_sum(s);
        for (int n = lane; n < N; n += 64) r[n] = r[n] / s;
    }
}

