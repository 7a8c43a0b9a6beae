// Segmentation-mask ground truth on the device (contract: include/ntmtrack.h, NTK_MASK_*): the bounds and area of a run-length
// coded mask and its overlap with the pixel set of a rectangle, straight from the counts -- the mask is never rasterised.  One
// 64-lane workgroup (one wave) per mask walks the counts 64 at a time: a wave inclusive scan plus a carry gives every run its
// start, a run of ones is then handled in closed form, in integers, and the results are reduced across the wave.  Plain vector
// stores, no atomics, no LDS.
#include "common.h"

namespace {

// A set of pixels of the mask's box as a range of columns [c0, c1) and of rows [r0, r1), both inside [0, w) x [0, h).
struct PixelRect {
    long long c0, c1, r0, r1;
};

__device__ __forceinline__ long long overlap_1d(long long a0, long long a1, long long b0, long long b1) {
    const long long lo = a0 > b0 ? a0 : b0, hi = a1 < b1 ? a1 : b1;
    return hi > lo ? hi - lo : 0;
}

// Pixel (c, r) belongs to the rectangle when its centre lies in [x, x2): the indices from ceil(x - 0.5) to ceil(x2 - 0.5) - 1.
// -> the two bounds as doubles (whole numbers, or the argument itself where it is too large to have a fraction).
__device__ __forceinline__ void centre_range(double x, double x2, double& first, double& end) {
    first = ceil(x - 0.5);
    end = ceil(x2 - 0.5);
    if (end < first) end = first;
}

// The range [first, end) of frame indices relative to a box that starts at `origin` and has `extent` pixels, clipped to the box.
__device__ __forceinline__ void clip_range(double first, double end, int origin, int extent, long long& lo, long long& hi) {
    const double a = fmin(fmax(first - (double)origin, 0.0), (double)extent);
    const double b = fmin(fmax(end - (double)origin, 0.0), (double)extent);
    lo = (long long)a;
    hi = (long long)b;
}

__device__ __forceinline__ long long wave_sum(long long v) {
    for (int d = 32; d > 0; d >>= 1) v += __shfl_xor(v, d, 64);
    return v;
}
__device__ __forceinline__ long long wave_min(long long v) {
    for (int d = 32; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, 64);
        v = o < v ? o : v;
    }
    return v;
}
__device__ __forceinline__ long long wave_max(long long v) {
    for (int d = 32; d > 0; d >>= 1) {
        const long long o = __shfl_xor(v, d, 64);
        v = o > v ? o : v;
    }
    return v;
}

// What the walk over one mask's counts leaves, the same in every lane.
struct MaskSums {
    long long area, inter;                      // |M|, |M n R|
    long long c_min, c_max, r_min, r_max;       // over the set pixels, relative to the box (valid when area > 0)
};

// The mask `cell` = (x0, y0, w, h, first, count) -> present.  Called by all 64 lanes of the wave (threadIdx.x = lane).  Nothing
// outside rle[0, n_rle) is read, whatever the cell holds.  INTER: R is the pixel set to intersect with.
template <bool INTER>
__device__ __forceinline__ bool walk_mask(const int* __restrict__ cell, const int* __restrict__ rle, int n_rle, const PixelRect& R,
                                          MaskSums& out) {
    const int lane = threadIdx.x;
    const long long w = cell[2], h = cell[3], first = cell[4], count = cell[5];
    if (!(w > 0 && h > 0 && w * h <= (long long)NTK_MASK_MAX_PIXELS && first >= 0 && count >= 0 && first + count <= (long long)n_rle))
        return false;
    const long long wh = w * h;
    long long carry = 0;                        // pixels before this chunk's first run, clamped to wh
    long long area = 0, inter = 0, c_min = w, c_max = -1, r_min = h, r_max = -1;
    bool bad = false;
    for (long long base = 0; base < count; base += 64) {
        const long long j = base + lane;
        long long c = j < count ? (long long)rle[first + j] : 0;
        if (c < 0) {
            bad = true;
            c = 0;
        }
        long long incl = c;                     // the wave's inclusive scan: 64 counts of less than 2^31 each
        for (int d = 1; d < 64; d <<= 1) {
            const long long up = __shfl_up(incl, d, 64);
            if (lane >= d) incl += up;
        }
        const long long total = __shfl(incl, 63, 64);
        long long s = carry + (incl - c);
        s = s < wh ? s : wh;
        long long e = s + c;
        e = e < wh ? e : wh;
        carry = carry + total < wh ? carry + total : wh;
        if ((lane & 1) && e > s) {              // base is a multiple of 64: an odd lane holds a run of ones [s, e)
            area += e - s;
            const long long ra = s / w, rb = (e - 1) / w, ca = s - ra * w, cb = (e - 1) - rb * w;
            r_min = ra < r_min ? ra : r_min;
            r_max = rb > r_max ? rb : r_max;
            if (ra == rb) {
                c_min = ca < c_min ? ca : c_min;
                c_max = cb > c_max ? cb : c_max;
            } else {
                c_min = 0;
                c_max = w - 1;
            }
            if constexpr (INTER) {
                if (ra == rb) {
                    if (ra >= R.r0 && ra < R.r1) inter += overlap_1d(ca, cb + 1, R.c0, R.c1);
                } else {
                    if (ra >= R.r0 && ra < R.r1) inter += overlap_1d(ca, w, R.c0, R.c1);
                    if (rb >= R.r0 && rb < R.r1) inter += overlap_1d(0, cb + 1, R.c0, R.c1);
                    inter += overlap_1d(ra + 1, rb, R.r0, R.r1) * (R.c1 - R.c0);
                }
            }
        }
    }
    if (__any(bad)) return false;
    out.area = wave_sum(area);
    if (out.area <= 0) return false;
    out.inter = INTER ? wave_sum(inter) : 0;
    out.c_min = wave_min(c_min);
    out.c_max = wave_max(c_max);
    out.r_min = wave_min(r_min);
    out.r_max = wave_max(r_max);
    return true;
}

}  // namespace

// rects[i] = (min col, min row, max col + 1 - min col, max row + 1 - min row) over mask i's set pixels, in frame pixels, and
// area[i] = |M|; NaNs for an absent mask.  One wave per mask, lane 0 stores.
__global__ void __launch_bounds__(64) track_mask_bounds_kernel(const int* __restrict__ cells, const int* __restrict__ rle, int n_rle,
                                                               double* __restrict__ rects, double* __restrict__ area) {
    const size_t i = blockIdx.x;
    const int* cell = cells + NTK_MASK_CELL_INTS * i;
    MaskSums m;
    const bool present = walk_mask<false>(cell, rle, n_rle, PixelRect(), m);
    if (threadIdx.x != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double* r = rects + 4 * i;
    r[0] = present ? (double)((long long)cell[0] + m.c_min) : nan;
    r[1] = present ? (double)((long long)cell[1] + m.r_min) : nan;
    r[2] = present ? (double)(m.c_max + 1 - m.c_min) : nan;
    r[3] = present ? (double)(m.r_max + 1 - m.r_min) : nan;
    area[i] = present ? (double)m.area : nan;
}

// overlap[i] = (|M n R|, |R|, |M|) of mask i and the pixel set of the rectangle regions[i]; NaNs for an absent mask.
__global__ void __launch_bounds__(64) track_mask_overlaps_kernel(const double* __restrict__ regions, const int* __restrict__ cells,
                                                                 const int* __restrict__ rle, int n_rle, double* __restrict__ overlap) {
#pragma clang fp contract(off)
    const size_t i = blockIdx.x;
    const int* cell = cells + NTK_MASK_CELL_INTS * i;
    const double* p = regions + 4 * i;
    PixelRect R = {0, 0, 0, 0};
    double area_r = 0.0;
    if (isfinite(p[0]) && isfinite(p[1]) && isfinite(p[2]) && isfinite(p[3])) {
        const double x2 = p[0] + fmax(p[2], 0.0), y2 = p[1] + fmax(p[3], 0.0);       // to corners first
        double c_first, c_end, r_first, r_end;
        centre_range(p[0], x2, c_first, c_end);
        centre_range(p[1], y2, r_first, r_end);
        if (isfinite(c_first) && isfinite(c_end) && isfinite(r_first) && isfinite(r_end)) {
            area_r = (c_end - c_first) * (r_end - r_first);
            clip_range(c_first, c_end, cell[0], cell[2] > 0 ? cell[2] : 0, R.c0, R.c1);
            clip_range(r_first, r_end, cell[1], cell[3] > 0 ? cell[3] : 0, R.r0, R.r1);
        }
    }
    MaskSums m;
    const bool present = walk_mask<true>(cell, rle, n_rle, R, m);
    if (threadIdx.x != 0) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double* o = overlap + NTK_MASK_OVERLAP_DOUBLES * i;
    o[0] = present ? (double)m.inter : nan;
    o[1] = present ? area_r : nan;
    o[2] = present ? (double)m.area : nan;
}

extern "C" int ntk_track_mask_bounds(const int* cells, const int* rle, int n_rle, int n, double* rects, double* area, void* stream) {
    NTK_REQUIRE(cells && rle && rects && area, NTK_ERR_BAD_PTR, "ntk_track_mask_bounds: null pointer");
    NTK_REQUIRE(n > 0 && n_rle >= 0, NTK_ERR_BAD_SHAPE, "ntk_track_mask_bounds: n=%d n_rle=%d", n, n_rle);
    track_mask_bounds_kernel<<<n, 64, 0, (hipStream_t)stream>>>(cells, rle, n_rle, rects, area);
    NTK_CHECK_LAUNCH("ntk_track_mask_bounds");
    return NTK_OK;
}

extern "C" int ntk_track_mask_overlaps(const double* regions, const int* cells, const int* rle, int n_rle, int n, double* overlap,
                                       void* stream) {
    NTK_REQUIRE(regions && cells && rle && overlap, NTK_ERR_BAD_PTR, "ntk_track_mask_overlaps: null pointer");
    NTK_REQUIRE(n > 0 && n_rle >= 0, NTK_ERR_BAD_SHAPE, "ntk_track_mask_overlaps: n=%d n_rle=%d", n, n_rle);
    track_mask_overlaps_kernel<<<n, 64, 0, (hipStream_t)stream>>>(regions, cells, rle, n_rle, overlap);
    NTK_CHECK_LAUNCH("ntk_track_mask_overlaps");
    return NTK_OK;
}
