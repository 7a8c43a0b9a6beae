// The online trackers' per-frame bookkeeping on the device: the box state of B trackers after a frame's pass
// (test_tracker.py:306-309 and the decode around it) and on a restart (ntmtrack/geometry.py), and the masked row copies that keep
// the NTM and DNC state of the slots that sit a frame out.
//
// The two box kernels each write out "region -> normalised box -> crop box -> state" on their own, and the two copies must not be
// merged: the restart kernel is compiled without contraction (the NumPy path's bits), the update kernel with it (it fuses products
// of that sequence into the sums behind them), and the update kernel's state rows change when the sequence is not contracted.
#include "common.h"

// Per-frame box bookkeeping of the online tracker for B trackers, one thread each, the geometry in double precision throughout
// (state layout: include/ntmtrack.h, NTK_TRACK_STATE_*).  offsets = fp32 tanh(logits[b, S-1, :]) ordered (dy, dx); the centred box
// 0.5 -+ bbox_grid / (2 cropbox_grid) shifted by them; back through the inverse of the crop transformation (the crop box was mapped
// onto the unit square, so the inverse is X * (x2 - x1) + x1); scaled by (w, h) -- NOT (w - 1, h - 1): the decode and
// normalize_bbox are asymmetric in the reference and here; the region (x, y, width, height); then the next frame's box state:
// a region whose four numbers are all < 1 is taken as already normalised (test_tracker.py:306-309), else divided by
// (h - 1, w - 1); the crop box is that box scaled about its centre by cropbox_grid / bbox_grid.
__global__ void track_boxes_update_kernel(const float* __restrict__ logits, int B, int S, double cropbox_grid, double bbox_grid,
                                          const unsigned char* __restrict__ active, double* __restrict__ state,
                                          float* __restrict__ cropbox32, double* __restrict__ regions, float* __restrict__ offsets,
                                          int* __restrict__ frame) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (active && !active[b]) return;
    double* st = state + (size_t)b * NTK_TRACK_STATE_DOUBLES;
    const float* lg = logits + ((size_t)b * S + (S - 1)) * 2;
    const float fy = tanhf(lg[0]), fx = tanhf(lg[1]);       // fp32 tanh, as the single tracker takes it (torch.tanh of fp32 logits)
    const double w = st[NTK_TRACK_STATE_W], h = st[NTK_TRACK_STATE_H];
    const double* cb = st + NTK_TRACK_STATE_CROPBOX;
    const double width = bbox_grid / cropbox_grid;
    const double lo = .5 - width / 2, hi = .5 + width / 2;
    const double sy = cb[2] - cb[0], sx = cb[3] - cb[1];
    // the shifted box is an fp32 sum, as in the single tracker: there a Python float plus an fp32 offset is an fp32 number
    const double oy1 = (float)lo + fy, ox1 = (float)lo + fx, oy2 = (float)hi + fy, ox2 = (float)hi + fx;
    const double y1 = (oy1 * sy + cb[0]) * h, x1 = (ox1 * sx + cb[1]) * w;
    const double y2 = (oy2 * sy + cb[0]) * h, x2 = (ox2 * sx + cb[1]) * w;
    const double rw = x2 - x1, rh = y2 - y1;
    const bool normalized = x1 < 1 && y1 < 1 && rw < 1 && rh < 1;
    const double by = normalized ? 1.0 : h - 1, bx = normalized ? 1.0 : w - 1;
    const double n0 = y1 / by, n1 = x1 / bx, n2 = (y1 + rh) / by, n3 = (x1 + rw) / bx;
    const double scale = cropbox_grid / bbox_grid;
    const double cy = (n0 + n2) / 2, cx = (n1 + n3) / 2, hy = (n2 - n0) * scale / 2, hx = (n3 - n1) * scale / 2;
    const double c0 = cy - hy, c1 = cx - hx, c2 = cy + hy, c3 = cx + hx;
    double* nb = st + NTK_TRACK_STATE_BBOX;
    double* ncb = st + NTK_TRACK_STATE_CROPBOX;
    nb[0] = n0; nb[1] = n1; nb[2] = n2; nb[3] = n3;
    ncb[0] = c0; ncb[1] = c1; ncb[2] = c2; ncb[3] = c3;
    float* c32 = cropbox32 + 4 * (size_t)b;
    c32[0] = (float)c0; c32[1] = (float)c1; c32[2] = (float)c2; c32[3] = (float)c3;
    double* rg = regions + 4 * (size_t)b;
    rg[0] = x1; rg[1] = y1; rg[2] = rw; rg[3] = rh;
    offsets[2 * (size_t)b] = fy;
    offsets[2 * (size_t)b + 1] = fx;
    if (frame) frame[b] += 1;
}

// First-frame geometry of the online tracker for the slots that restart on this frame (BatchNTMTracker._first_frame_inputs on the
// device, masked): one thread per slot, float64 in the operation order of ntmtrack/geometry.py, no contraction, so the state
// row, the crop box and the region have the bits of the NumPy path.  The heat-map row is discrete_gauss on the g x g grid about
// the centre of the object box taken through the crop transformation; the exponentials are evaluated three times (maximum, sum,
// values) rather than kept in g * g registers.  A slot that does not restart has its gts0 row zeroed and nothing else written.
__global__ void track_restart_boxes_kernel(const double* __restrict__ regions_in, const unsigned char* __restrict__ restart,
                                           const unsigned char* __restrict__ active, int B, double cropbox_grid, double bbox_grid,
                                           double sigma, int g, double* __restrict__ state, float* __restrict__ cropbox32,
                                           double* __restrict__ regions, float* __restrict__ offsets, int* __restrict__ frame,
                                           float* __restrict__ gts0, unsigned char* __restrict__ run_mask,
                                           unsigned char* __restrict__ move_mask) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const bool rs = restart[b] != 0, act = !active || active[b];
    if (run_mask) run_mask[b] = (rs || act) ? 1 : 0;
    if (move_mask) move_mask[b] = (act && !rs) ? 1 : 0;
    float* hm = gts0 + (size_t)b * g * g;
    if (!rs) {
        for (int i = 0; i < g * g; ++i) hm[i] = 0.f;
        return;
    }
    double* st = state + (size_t)b * NTK_TRACK_STATE_DOUBLES;
    const double* rin = regions_in + 4 * (size_t)b;
    const double x1 = rin[0], y1 = rin[1], rw = rin[2], rh = rin[3];
    const double w = st[NTK_TRACK_STATE_W], h = st[NTK_TRACK_STATE_H];
    const bool normalized = x1 < 1 && y1 < 1 && rw < 1 && rh < 1;
    double n0 = y1, n1 = x1, n2 = y1 + rh, n3 = x1 + rw;
    if (!normalized) {
        const double by = h - 1, bx = w - 1;
        n0 = n0 / by; n1 = n1 / bx; n2 = n2 / by; n3 = n3 / bx;
    }
    const double scale = cropbox_grid / bbox_grid;
    const double cy = (n0 + n2) / 2, cx = (n1 + n3) / 2, hy = (n2 - n0) * scale / 2, hx = (n3 - n1) * scale / 2;
    const double c0 = cy - hy, c1 = cx - hx, c2 = cy + hy, c3 = cx + hx;
    double* nb = st + NTK_TRACK_STATE_BBOX;
    double* ncb = st + NTK_TRACK_STATE_CROPBOX;
    nb[0] = n0; nb[1] = n1; nb[2] = n2; nb[3] = n3;
    ncb[0] = c0; ncb[1] = c1; ncb[2] = c2; ncb[3] = c3;
    float* c32 = cropbox32 + 4 * (size_t)b;
    c32[0] = (float)c0; c32[1] = (float)c1; c32[2] = (float)c2; c32[3] = (float)c3;
    double* rg = regions + 4 * (size_t)b;
    rg[0] = x1; rg[1] = y1; rg[2] = rw; rg[3] = rh;
    offsets[2 * (size_t)b] = 0.f;
    offsets[2 * (size_t)b + 1] = 0.f;
    frame[b] = 0;
    // the object box through the map that sends the crop box to the unit square (rows (sx, 0, -x1 sx) and (0, sy, -y1 sy))
    const double sx = 1.0 / (c3 - c1), sy = 1.0 / (c2 - c0);
    const double tx = -c1 * sx, ty = -c0 * sy;
    const double ux1 = sx * n1 + tx, ux2 = sx * n3 + tx, uy1 = sy * n0 + ty, uy2 = sy * n2 + ty;
    const double mx = (ux1 + ux2) / 2., my = (uy1 + uy2) / 2.;
    const double x0 = 0.5 - mx * g, y0 = 0.5 - my * g, den = 2.0 * sigma * sigma;
    double top = 0.0;
    for (int iy = 0; iy < g; ++iy)
        for (int ix = 0; ix < g; ++ix) {
            const double ys = y0 + iy, xs = x0 + ix;
            top = fmax(top, exp(-(ys * ys + xs * xs) / den));
        }
    const double cut = 2.220446049250313e-16 * top;             // np.finfo(float64).eps * max
    double total = 0.0;
    for (int iy = 0; iy < g; ++iy)
        for (int ix = 0; ix < g; ++ix) {
            const double ys = y0 + iy, xs = x0 + ix;
            const double v = exp(-(ys * ys + xs * xs) / den);
            total += v < cut ? 0.0 : v;
        }
    for (int iy = 0; iy < g; ++iy)
        for (int ix = 0; ix < g; ++ix) {
            const double ys = y0 + iy, xs = x0 + ix;
            double v = exp(-(ys * ys + xs * xs) / den);
            v = v < cut ? 0.0 : v;
            hm[iy * g + ix] = (float)(total != 0 ? v / total : v);
        }
}

// out[b, :] = mask[b] ? a[b, :] : b_[b, :]   (out may be a or b_: every element is read and written by the same thread)
__global__ void select_rows_kernel(const unsigned char* __restrict__ mask, const float* a, const float* b_, float* out,
                                   size_t total, int n) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= total) return;
    out[idx] = mask[idx / (size_t)n] ? a[idx] : b_[idx];
}

// Masked row copy of several tensors in one launch: for every b with (mask[b] != 0) == keep_where, row b of src[i] is copied to
// row b of dst[i], i < ntensors (rows of rows.n[i] floats).  Grid (chunks, B): workgroup x copies chunk x of the list of all
// tensors' chunks of KEEP_CHUNK floats (rows.first[i] = index of tensor i's first chunk).  A workgroup whose row is not selected
// exits before it reads a table or touches a row.  16-byte loads and stores where the row size and both bases allow, else
// one float per lane.
constexpr int KEEP_CHUNK = 1024;             // floats per workgroup: one 16-byte access per lane; a 512 x 512 link row is 256 workgroups
struct KeepRows {
    long long n[NTK_STATE_KEEP_MAX_TENSORS];
    int first[NTK_STATE_KEEP_MAX_TENSORS + 1];
};

__global__ __launch_bounds__(256) void dnc_state_keep_kernel(const unsigned char* __restrict__ mask, int keep_where, int ntensors,
                                                            const float* const* __restrict__ src, float* const* __restrict__ dst,
                                                            KeepRows rows) {
    const int b = blockIdx.y;
    if ((mask[b] != 0) != (keep_where != 0)) return;
    int i = 0;
    while (i + 1 < ntensors && (int)blockIdx.x >= rows.first[i + 1]) ++i;
    const long long n = rows.n[i];
    const long long off = (long long)((int)blockIdx.x - rows.first[i]) * KEEP_CHUNK;
    const int len = (int)(n - off < KEEP_CHUNK ? n - off : KEEP_CHUNK);
    const float* s = src[i] + (size_t)b * (size_t)n + (size_t)off;
    float* d = dst[i] + (size_t)b * (size_t)n + (size_t)off;
    if ((n & 3) == 0 && ((((uintptr_t)s) | ((uintptr_t)d)) & 15u) == 0) {
        for (int j = 4 * (int)threadIdx.x; j < len; j += 4 * 256)
            *reinterpret_cast<float4*>(d + j) = *reinterpret_cast<const float4*>(s + j);
    } else {
        for (int j = (int)threadIdx.x; j < len; j += 256) d[j] = s[j];
    }
}

extern "C" int ntk_track_boxes_update(const float* logits, int B, int S, double cropbox_grid, double bbox_grid,
                                      const unsigned char* active, double* state, float* cropbox32, double* regions,
                                      float* offsets, int* frame, void* stream) {
    NTK_REQUIRE(logits && state && cropbox32 && regions && offsets, NTK_ERR_BAD_PTR, "ntk_track_boxes_update: null pointer");
    NTK_REQUIRE(B > 0 && S > 0 && cropbox_grid > 0 && bbox_grid > 0, NTK_ERR_BAD_SHAPE,
                "ntk_track_boxes_update: B=%d S=%d cropbox_grid=%g bbox_grid=%g", B, S, cropbox_grid, bbox_grid);
    track_boxes_update_kernel<<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(logits, B, S, cropbox_grid, bbox_grid, active, state,
                                                                            cropbox32, regions, offsets, frame);
    NTK_CHECK_LAUNCH("ntk_track_boxes_update");
    return NTK_OK;
}

extern "C" int ntk_track_restart_boxes(const double* regions_in, const unsigned char* restart, const unsigned char* active, int B,
                                       double cropbox_grid, double bbox_grid, double sigma, int gts_width, double* state,
                                       float* cropbox32, double* regions, float* offsets, int* frame, float* gts0,
                                       unsigned char* run_mask, unsigned char* move_mask, void* stream) {
    NTK_REQUIRE(regions_in && restart && state && cropbox32 && regions && offsets && frame && gts0, NTK_ERR_BAD_PTR,
                "ntk_track_restart_boxes: null pointer");
    NTK_REQUIRE(B > 0 && B <= 65535, NTK_ERR_BAD_SHAPE, "ntk_track_restart_boxes: B=%d (1..65535)", B);
    NTK_REQUIRE(cropbox_grid > 0 && bbox_grid > 0 && sigma > 0, NTK_ERR_BAD_SHAPE,
                "ntk_track_restart_boxes: cropbox_grid=%g bbox_grid=%g sigma=%g", cropbox_grid, bbox_grid, sigma);
    const int g = cropbox_grid <= 1024 ? (int)cropbox_grid : 0;
    NTK_REQUIRE(g >= 1 && (double)g == cropbox_grid && g * g == gts_width, NTK_ERR_BAD_SHAPE,
                "ntk_track_restart_boxes: gts_width=%d for cropbox_grid=%g (a whole number up to 1024, gts_width its square)",
                gts_width, cropbox_grid);
    track_restart_boxes_kernel<<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(regions_in, restart, active, B, cropbox_grid, bbox_grid,
                                                                             sigma, g, state, cropbox32, regions, offsets, frame,
                                                                             gts0, run_mask, move_mask);
    NTK_CHECK_LAUNCH("ntk_track_restart_boxes");
    return NTK_OK;
}

extern "C" int ntk_select_rows(const unsigned char* mask, const float* a, const float* b, float* out, int B, int n, void* stream) {
    NTK_REQUIRE(mask && a && b && out, NTK_ERR_BAD_PTR, "ntk_select_rows: null pointer");
    NTK_REQUIRE(B > 0 && n > 0, NTK_ERR_BAD_SHAPE, "ntk_select_rows: B=%d n=%d", B, n);
    const size_t total = (size_t)B * n;
    NTK_REQUIRE((total + 255) / 256 < 2147483647UL, NTK_ERR_BAD_SHAPE, "ntk_select_rows: B=%d n=%d: too many elements", B, n);
    select_rows_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(mask, a, b, out, total, n);
    NTK_CHECK_LAUNCH("ntk_select_rows");
    return NTK_OK;
}

extern "C" int ntk_dnc_state_keep(const unsigned char* mask, int keep_where, int B, int ntensors, const float* const* src,
                                  float* const* dst, const long long* row_floats, void* stream) {
    NTK_REQUIRE(mask && src && dst && row_floats, NTK_ERR_BAD_PTR, "ntk_dnc_state_keep: null pointer");
    NTK_REQUIRE(B >= 1 && B <= 65535, NTK_ERR_BAD_SHAPE, "ntk_dnc_state_keep: B=%d (1..65535)", B);
    NTK_REQUIRE(ntensors >= 1 && ntensors <= NTK_STATE_KEEP_MAX_TENSORS, NTK_ERR_BAD_SHAPE, "ntk_dnc_state_keep: ntensors=%d (1..%d)",
                ntensors, NTK_STATE_KEEP_MAX_TENSORS);
    KeepRows rows = {};
    long long chunks = 0;
    for (int i = 0; i < ntensors; ++i) {
        NTK_REQUIRE(row_floats[i] >= 0, NTK_ERR_BAD_SHAPE, "ntk_dnc_state_keep: row_floats[%d]=%lld", i, row_floats[i]);
        rows.n[i] = row_floats[i];
        rows.first[i] = (int)chunks;
        chunks += (row_floats[i] + KEEP_CHUNK - 1) / KEEP_CHUNK;
        NTK_REQUIRE(chunks < 2147483647LL, NTK_ERR_BAD_SHAPE, "ntk_dnc_state_keep: row_floats[%d]=%lld: too many elements per row", i,
                    row_floats[i]);
    }
    rows.first[ntensors] = (int)chunks;
    if (chunks == 0) return NTK_OK;
    dnc_state_keep_kernel<<<dim3((unsigned)chunks, (unsigned)B), 256, 0, (hipStream_t)stream>>>(mask, keep_where, ntensors, src, dst, rows);
    NTK_CHECK_LAUNCH("ntk_dnc_state_keep");
    return NTK_OK;
}
