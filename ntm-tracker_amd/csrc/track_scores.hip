// The validation protocol on the device: the overlap of a tracked rectangle with rectangle, polygon or mask ground truth (the VOT /
// OTB overlap, float64; polygons by Sutherland-Hodgman clipping, contract: include/ntmtrack.h, NTK_POLY_*; masks from the pixel
// counts of ntk_track_mask_overlaps, track_masks.hip, NTK_MASK_*), the per-clip overlap tables (NTK_SCORE_*) and the supervised
// protocol's state machine (NTK_SUP_*) and the multi-start protocol's run table (NTK_MS_*; its EAO reduction: track_eao.hip).  One
// thread per slot; no atomics.
#include "common.h"

namespace {      // the overlap functions; the kernels below keep their external names

// Overlap of two rectangles (x, y, w, h) with w, h >= 0, in float64 on real-valued coordinates (the VOT / OTB overlap).  Both are
// taken to corners first and every width is a difference of corners, so the intersection of a box with itself has the box's own
// sides bit for bit: its IoU is a / (a + a - a) = 1.0 exactly, and boxes that only touch meet in a side of exactly 0.
// Contraction is off in these functions (the header's __dmul_rn is a plain product the compiler may still fuse): a product is
// rounded before it is added, so integer-valued boxes give the bits of any IEEE float64 evaluation of the same expression.
__device__ __forceinline__ double rect_iou(double px, double py, double pw, double ph, double gx, double gy, double gw, double gh) {
#pragma clang fp contract(off)
    const double px2 = px + pw, py2 = py + ph, gx2 = gx + gw, gy2 = gy + gh;
    const double ix = fmin(px2, gx2) - fmax(px, gx), iy = fmin(py2, gy2) - fmax(py, gy);
    if (!(ix > 0 && iy > 0)) return 0.0;
    const double inter = ix * iy;
    const double area_p = (px2 - px) * (py2 - py), area_g = (gx2 - gx) * (gy2 - gy);
    const double uni = (area_p + area_g) - inter;
    const double iou = inter / uni;
    if (!(iou > 0)) return 0.0;                 // an intersection that underflowed, or inf / inf of huge boxes
    return iou > 1.0 ? 1.0 : iou;
}

__device__ __forceinline__ bool finite4(const double* r) { return isfinite(r[0]) && isfinite(r[1]) && isfinite(r[2]) && isfinite(r[3]); }

// ---- polygon ground truth (contract: include/ntmtrack.h, NTK_POLY_*) ----------------------------------------------------------
// A region is double[NTK_POLY_DOUBLES]: the leading pairs whose two numbers are both finite are its vertices, the rest is padding.
__device__ __forceinline__ int poly_vertices(const double* g) {
    int n = 0;
    while (n < NTK_POLY_MAX_POINTS && isfinite(g[2 * n]) && isfinite(g[2 * n + 1])) ++n;
    return n;
}

// Shoelace area of n points (x0, y0, x1, y1, ...) about the first one, either orientation.  Integer coordinates give it exactly.
__device__ __forceinline__ double shoelace_area(const double* pts, int n) {
#pragma clang fp contract(off)
    if (n < 3) return 0.0;
    const double ox = pts[0], oy = pts[1];
    double s = 0.0;
    for (int i = 0; i < n; ++i) {
        const int j = i + 1 < n ? i + 1 : 0;
        s += (pts[2 * i] - ox) * (pts[2 * j + 1] - oy) - (pts[2 * j] - ox) * (pts[2 * i + 1] - oy);
    }
    return fabs(s) / 2;
}

// What the ground truth of a frame is: a rectangle, a polygon of NTK_POLY_DOUBLES doubles, or a mask, given as its bounding
// rectangle (ntk_track_mask_bounds) beside the pixel counts of ntk_track_mask_overlaps.
enum class Gt { RECT, POLY, MASK };

template <Gt KIND>
constexpr int gt_doubles() { return KIND == Gt::POLY ? NTK_POLY_DOUBLES : 4; }

// The ground truth of one frame as both kernels see it: the rectangle (the region itself, the polygon's bounding rectangle -- the
// true minimum and maximum over its vertices -- or the mask's), and for a polygon its vertex count and area.
struct Truth {
    double x, y, w, h, area;
    int n;
};

// -> present.  POLY: at least 3 vertices, a bounding rectangle with w > 0 and h > 0, a shoelace area > 0.  MASK: as RECT, on the
// mask's bounding rectangle (four NaNs for an absent mask).
template <Gt KIND>
__device__ __forceinline__ bool read_truth(const double* g, Truth& tr) {
#pragma clang fp contract(off)
    if constexpr (KIND != Gt::POLY) {
        tr.x = g[0]; tr.y = g[1]; tr.w = g[2]; tr.h = g[3];
        tr.area = 0.0; tr.n = 0;
        return finite4(g) && g[2] > 0 && g[3] > 0;
    } else {
        const int n = poly_vertices(g);
        tr.n = n;
        if (n < 3) return false;
        double x0 = g[0], x1 = g[0], y0 = g[1], y1 = g[1];
        for (int i = 1; i < n; ++i) {
            x0 = fmin(x0, g[2 * i]); x1 = fmax(x1, g[2 * i]);
            y0 = fmin(y0, g[2 * i + 1]); y1 = fmax(y1, g[2 * i + 1]);
        }
        tr.x = x0; tr.y = y0; tr.w = x1 - x0; tr.h = y1 - y0;
        if (!(tr.w > 0 && tr.h > 0)) return false;
        tr.area = shoelace_area(g, n);
        return tr.area > 0;
    }
}

// One half-plane of Sutherland-Hodgman: keeps the part of the n-gon ``in`` whose coordinate ``axis`` (0 = x, 1 = y) is strictly
// above (or strictly below) c.  A crossing point gets c itself on that axis, so the next test on it is exact.  -> points written
// to ``out``, never more than POLY_CLIP_MAX (a half-plane turns n points into at most 3n/2: 8 -> 12 -> 18 -> 27 -> 40).
constexpr int POLY_CLIP_MAX = 40;
__device__ __forceinline__ int clip_half_plane(const double* in, int n, double* out, int axis, double c, bool above) {
#pragma clang fp contract(off)
    const int o = 1 - axis;
    int m = 0;
    for (int i = 0; i < n; ++i) {
        const double* a = in + 2 * i;
        const double* b = in + 2 * (i + 1 < n ? i + 1 : 0);
        const bool ia = above ? a[axis] > c : a[axis] < c, ib = above ? b[axis] > c : b[axis] < c;
        if (ia != ib && m < POLY_CLIP_MAX) {
            out[2 * m + axis] = c;
            out[2 * m + o] = a[o] + (b[o] - a[o]) * ((c - a[axis]) / (b[axis] - a[axis]));
            ++m;
        }
        if (ib && m < POLY_CLIP_MAX) {
            out[2 * m] = b[0];
            out[2 * m + 1] = b[1];
            ++m;
        }
    }
    return m;
}

// Overlap of the rectangle (x, y, w, h), w, h >= 0, with a simple polygon of tr.n vertices at g: the polygon is clipped against
// the rectangle's four sides in turn and the shoelace area of what is left is |P n R|.  The inside tests are strict, so a polygon
// that only touches the rectangle, or lies beside it, leaves an empty list and scores exactly 0.0; an axis-aligned integer 4-gon
// goes through exact arithmetic only and gives rect_iou's bits.  No contraction, clamped to [0, 1].
__device__ __forceinline__ double poly_iou(double px, double py, double pw, double ph, const double* g, const Truth& tr) {
#pragma clang fp contract(off)
    const double px2 = px + pw, py2 = py + ph;
    double a[2 * POLY_CLIP_MAX], b[2 * POLY_CLIP_MAX];
    int m = clip_half_plane(g, tr.n, a, 0, px, true);
    if (m) m = clip_half_plane(a, m, b, 0, px2, false);
    if (m) m = clip_half_plane(b, m, a, 1, py, true);
    if (m) m = clip_half_plane(a, m, b, 1, py2, false);
    if (m < 3) return 0.0;
    const double inter = shoelace_area(b, m);
    const double area_p = (px2 - px) * (py2 - py);
    const double uni = (area_p + tr.area) - inter;
    const double iou = inter / uni;
    if (!(iou > 0)) return 0.0;
    return iou > 1.0 ? 1.0 : iou;
}

// Overlap with a mask from ov = (|M n R|, |R|, |M|), whole numbers in doubles: I / ((R + M) - I), one division; 0.0 when I == 0.
__device__ __forceinline__ double mask_iou(const double* ov) {
#pragma clang fp contract(off)
    if (!(ov[0] > 0)) return 0.0;
    return ov[0] / ((ov[1] + ov[2]) - ov[0]);
}

// ov: the frame's NTK_MASK_OVERLAP_DOUBLES counts, read for MASK only.
template <Gt KIND>
__device__ __forceinline__ double truth_iou(double px, double py, double pw, double ph, const double* g, const Truth& tr,
                                            const double* ov) {
    if constexpr (KIND == Gt::POLY) return poly_iou(px, py, pw, ph, g, tr);
    else if constexpr (KIND == Gt::MASK) return mask_iou(ov);
    else return rect_iou(px, py, pw, ph, tr.x, tr.y, tr.w, tr.h);
}

}  // namespace

// (min x, min y, max x - min x, max y - min y) over each region's vertices, four NaNs for an absent one: one thread per region.
__global__ void track_poly_bounds_kernel(const double* __restrict__ poly, int n, double* __restrict__ rects) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Truth tr;
    const bool present = read_truth<Gt::POLY>(poly + (size_t)NTK_POLY_DOUBLES * i, tr);
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    double* r = rects + 4 * (size_t)i;
    r[0] = present ? tr.x : nan; r[1] = present ? tr.y : nan; r[2] = present ? tr.w : nan; r[3] = present ? tr.h : nan;
}

// Per-clip tracking scores kept on the device (row layout: include/ntmtrack.h, NTK_SCORE_*).  One thread per slot walks its T
// frames in order and adds to the row clip_of[b] of the table: the head of the row is carried in registers and written back at the
// end, the threshold counts are incremented in place.  The row belongs to this thread alone (two slots never share a row: the
// caller's contract), so a clip's sums are formed in frame order and no atomics are needed.  A slot whose row is outside
// [0, n_clips) reads nothing but clip_of[b].  POLY: the ground truth is a polygon of NTK_POLY_DOUBLES doubles per frame; the
// overlap is poly_iou and the centre distance is taken to the centre of its bounding rectangle.  MASK: gt holds the masks'
// bounding rectangles and `overlap` [T,B,NTK_MASK_OVERLAP_DOUBLES] their pixel counts against the regions (null otherwise).
template <Gt KIND>
__global__ void track_overlap_scores_kernel(const double* __restrict__ regions, const double* __restrict__ gt,
                                            const double* __restrict__ overlap, const unsigned char* __restrict__ active,
                                            const int* __restrict__ clip_of, int T, int B,
                                            int n_clips, const double* __restrict__ iou_thr, int n_iou,
                                            const double* __restrict__ dist_thr, int n_dist, double* __restrict__ table,
                                            double* __restrict__ frame_iou) {
#pragma clang fp contract(off)
    constexpr int GT = gt_doubles<KIND>();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const int clip = clip_of[b];
    if (clip < 0 || clip >= n_clips) {
        if (frame_iou)
            for (int t = 0; t < T; ++t) frame_iou[(size_t)t * B + b] = nan;
        return;
    }
    double* row = table + (size_t)clip * (NTK_SCORE_HEAD + n_iou + n_dist);
    double frames = row[NTK_SCORE_FRAMES], sum_iou = row[NTK_SCORE_SUM_IOU], sum_dist = row[NTK_SCORE_SUM_DIST];
    double lost = row[NTK_SCORE_LOST], first_lost = row[NTK_SCORE_FIRST_LOST];
    for (int t = 0; t < T; ++t) {
        const size_t at = (size_t)t * B + b;
        const double* g = gt + GT * at;
        Truth tr;
        const bool scored = (!active || active[at]) && read_truth<KIND>(g, tr);
        if (!scored) {
            if (frame_iou) frame_iou[at] = nan;
            continue;
        }
        const double* p = regions + 4 * at;
        double iou = 0.0;
        if (finite4(p)) {
            const double pw = fmax(p[2], 0.0), ph = fmax(p[3], 0.0);
            iou = truth_iou<KIND>(p[0], p[1], pw, ph, g, tr, overlap + NTK_MASK_OVERLAP_DOUBLES * at);
            const double dx = (p[0] + pw / 2) - (tr.x + tr.w / 2), dy = (p[1] + ph / 2) - (tr.y + tr.h / 2);
            const double dist = sqrt(dx * dx + dy * dy);
            sum_dist += dist;
            for (int k = 0; k < n_dist; ++k)
                if (dist <= dist_thr[k]) row[NTK_SCORE_HEAD + n_iou + k] += 1.0;
        }
        if (iou == 0.0) {
            if (first_lost < 0) first_lost = frames;
            lost += 1.0;
        }
        for (int k = 0; k < n_iou; ++k)
            if (iou > iou_thr[k]) row[NTK_SCORE_HEAD + k] += 1.0;
        sum_iou += iou;
        frames += 1.0;
        if (frame_iou) frame_iou[at] = iou;
    }
    row[NTK_SCORE_FRAMES] = frames;
    row[NTK_SCORE_SUM_IOU] = sum_iou;
    row[NTK_SCORE_SUM_DIST] = sum_dist;
    row[NTK_SCORE_LOST] = lost;
    row[NTK_SCORE_FIRST_LOST] = first_lost;
}

// The supervised protocol's state machine (contract: include/ntmtrack.h, NTK_SUP_*), one thread per slot, one frame per call.
// plan decides before the frame's pass what every slot does on it; judge scores the tracked slots after the pass with the one
// overlap of the overlap table and moves a failed slot to WAIT.  The table row belongs to the slot's thread alone.  POLY: the ground
// truth is a polygon, MASK: a mask (judge reads `overlap` [B,NTK_MASK_OVERLAP_DOUBLES]), as in track_overlap_scores_kernel.
template <Gt KIND>
__global__ void track_supervise_plan_kernel(const double* __restrict__ gt, const unsigned char* __restrict__ active,
                                            const int* __restrict__ clip_of, int B, int n_clips, int* __restrict__ state,
                                            double* __restrict__ table, unsigned char* __restrict__ track,
                                            unsigned char* __restrict__ restart, signed char* __restrict__ codes,
                                            double* __restrict__ frame_iou) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    if (frame_iou) frame_iou[b] = __longlong_as_double(0x7ff8000000000000LL);
    const int clip = clip_of[b];
    unsigned char tr = 0, rs = 0;
    signed char code = NTK_SUP_CODE_INACTIVE;
    if (clip >= 0 && clip < n_clips && (!active || active[b])) {
        int* st = state + (size_t)b * NTK_SUP_STATE_INTS;
        double* row = table + (size_t)clip * NTK_SUP_HEAD;
        if (st[NTK_SUP_STATE_MODE] == NTK_SUP_MODE_TRACK) {
            tr = 1;
            code = NTK_SUP_CODE_TRACKED;
        } else {
            const int left = st[NTK_SUP_STATE_COUNTDOWN] > 1 ? st[NTK_SUP_STATE_COUNTDOWN] - 1 : 0;
            st[NTK_SUP_STATE_COUNTDOWN] = left;
            Truth tr;
            if (left == 0 && read_truth<KIND>(gt + gt_doubles<KIND>() * (size_t)b, tr)) {
                rs = 1;
                code = NTK_SUP_CODE_RESTART;
                row[NTK_SUP_RESTARTS] += 1.0;
                st[NTK_SUP_STATE_MODE] = NTK_SUP_MODE_TRACK;
                st[NTK_SUP_STATE_SINCE] = 0;
            } else {
                code = NTK_SUP_CODE_SKIPPED;
                row[NTK_SUP_SKIPPED] += 1.0;
            }
        }
    }
    track[b] = tr;
    restart[b] = rs;
    if (codes) codes[b] = code;
}

template <Gt KIND>
__global__ void track_supervise_judge_kernel(const double* __restrict__ regions, const double* __restrict__ gt,
                                             const double* __restrict__ overlap, const unsigned char* __restrict__ track, const int* __restrict__ clip_of, int B,
                                             int n_clips, int skip, int burn_in, double failure_overlap, int* __restrict__ state,
                                             double* __restrict__ table, signed char* __restrict__ codes,
                                             double* __restrict__ frame_iou) {
#pragma clang fp contract(off)
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int clip = clip_of[b];
    if (clip < 0 || clip >= n_clips || !track[b]) return;
    int* st = state + (size_t)b * NTK_SUP_STATE_INTS;
    const double* g = gt + gt_doubles<KIND>() * (size_t)b;
    Truth tr;
    if (!read_truth<KIND>(g, tr)) {                          // tracked, the object absent: the frame is counted nowhere
        st[NTK_SUP_STATE_SINCE] += 1;
        if (codes) codes[b] = NTK_SUP_CODE_TRACKED;
        return;
    }
    const double* p = regions + 4 * (size_t)b;
    double iou = 0.0;
    if (finite4(p)) iou = truth_iou<KIND>(p[0], p[1], fmax(p[2], 0.0), fmax(p[3], 0.0), g, tr, overlap + NTK_MASK_OVERLAP_DOUBLES * (size_t)b);
    double* row = table + (size_t)clip * NTK_SUP_HEAD;
    const double tracked = row[NTK_SUP_TRACKED];
    row[NTK_SUP_TRACKED] = tracked + 1.0;
    if (frame_iou) frame_iou[b] = iou;
    if (iou <= failure_overlap) {
        row[NTK_SUP_FAILURES] += 1.0;
        if (row[NTK_SUP_FIRST_FAILURE] < 0) row[NTK_SUP_FIRST_FAILURE] = tracked;
        st[NTK_SUP_STATE_MODE] = NTK_SUP_MODE_WAIT;
        st[NTK_SUP_STATE_COUNTDOWN] = skip;
        if (codes) codes[b] = NTK_SUP_CODE_FAILURE;
        return;
    }
    const int since = st[NTK_SUP_STATE_SINCE] + 1;
    st[NTK_SUP_STATE_SINCE] = since;
    if (since > burn_in) {
        row[NTK_SUP_VALID] += 1.0;
        row[NTK_SUP_SUM_IOU] += iou;
    }
    if (codes) codes[b] = NTK_SUP_CODE_TRACKED;
}

// The multi-start protocol's scoring (contract: include/ntmtrack.h, NTK_MS_*): one thread per slot walks its T frames in order.
// Everything the protocol remembers -- the open streak of low frames included, which is what lets the failure look-ahead cross a
// round -- is in the run's table row: the row is carried in registers and written back at the end.  The row and the run's stretch
// of the trace belong to this thread alone.  A slot whose run is outside [0, n_runs) reads nothing but clip_of[b].
template <Gt KIND>
__global__ void track_multistart_kernel(const double* __restrict__ regions, const double* __restrict__ gt,
                                        const double* __restrict__ overlap, const unsigned char* __restrict__ active,
                                        const int* __restrict__ clip_of, int T, int B, int n_runs, double failure_overlap,
                                        int patience, double* __restrict__ table, const long long* __restrict__ trace_first,
                                        double* __restrict__ trace, double* __restrict__ frame_iou) {
#pragma clang fp contract(off)
    constexpr int GT = gt_doubles<KIND>();
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const double nan = __longlong_as_double(0x7ff8000000000000LL);
    const int run = clip_of[b];
    if (run < 0 || run >= n_runs) {
        if (frame_iou)
            for (int t = 0; t < T; ++t) frame_iou[(size_t)t * B + b] = nan;
        return;
    }
    double* row = table + (size_t)run * NTK_MS_HEAD;
    double frames = row[NTK_MS_FRAMES], tracked = row[NTK_MS_TRACKED], sum_iou = row[NTK_MS_SUM_IOU];
    double failed = row[NTK_MS_FAILED], low = row[NTK_MS_LOW], pending = row[NTK_MS_PENDING];
    const long long first = trace_first[run], room = trace_first[run + 1] - first;
    for (int t = 0; t < T; ++t) {
        const size_t at = (size_t)t * B + b;
        const double* g = gt + GT * at;
        Truth tr;
        const bool scored = (!active || active[at]) && read_truth<KIND>(g, tr);
        if (!scored) {
            if (frame_iou) frame_iou[at] = nan;
            continue;
        }
        const double* p = regions + 4 * at;
        double iou = 0.0;
        if (finite4(p))
            iou = truth_iou<KIND>(p[0], p[1], fmax(p[2], 0.0), fmax(p[3], 0.0), g, tr, overlap + NTK_MASK_OVERLAP_DOUBLES * at);
        const long long i = (long long)frames;
        if (first >= 0 && i < room) trace[first + i] = iou;
        if (frame_iou) frame_iou[at] = iou;
        frames += 1.0;
        if (failed != 0.0) continue;
        pending += iou;
        if (iou <= failure_overlap) {
            low += 1.0;
            if (low > (double)patience) {       // frames TRACKED ... TRACKED + patience are all low
                failed = 1.0;
                low = 0.0;
                pending = sum_iou;
            }
        } else {                                // the streak, if one was open, is forgiven
            sum_iou = pending;
            tracked += low + 1.0;
            low = 0.0;
        }
    }
    row[NTK_MS_FRAMES] = frames;
    row[NTK_MS_TRACKED] = tracked;
    row[NTK_MS_SUM_IOU] = sum_iou;
    row[NTK_MS_FAILED] = failed;
    row[NTK_MS_LOW] = low;
    row[NTK_MS_PENDING] = pending;
}

// Which frames of a round a file-fed validation may use (contract: include/ntmtrack.h, NTK_CLIPDEC_*): one thread per slot walks
// its T frames in order, turns off every active frame whose pixels the decoder did not deliver and counts in the row clip_of[b]
// of the table, which belongs to this thread alone.  status is read only at indices inside [0, n_status).
__global__ void track_decode_mask_kernel(const int* __restrict__ status, int n_status, const int* __restrict__ cell_index,
                                         const int* __restrict__ start_index, const int* __restrict__ clip_of, int T, int B,
                                         int n_clips, unsigned char* __restrict__ dead, unsigned char* __restrict__ active,
                                         long long* __restrict__ table) {
    const int b = blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= B) return;
    const int clip = clip_of[b];
    if (clip < 0 || clip >= n_clips) return;
    long long* row = table + (size_t)clip * NTK_CLIPDEC_HEAD;
    const int start = start_index[b];
    unsigned char is_dead = dead[b];
    if (start >= 0) {
        const int s = start < n_status ? status[start] : NTK_JPEG_STATUS_BAD_DESC;
        is_dead = s != 0;
        dead[b] = is_dead;
        row[NTK_CLIPDEC_START_STATUS] = s;
    }
    long long decoded = row[NTK_CLIPDEC_DECODED], failed = row[NTK_CLIPDEC_FAILED], masked = row[NTK_CLIPDEC_MASKED];
    long long first_failed = row[NTK_CLIPDEC_FIRST_FAILED], first_status = row[NTK_CLIPDEC_FIRST_STATUS];
    for (int t = 0; t < T; ++t) {
        const size_t at = (size_t)t * B + b;
        if (!active[at]) continue;
        const int i = cell_index[at];
        const int s = i < 0 ? 0 : (i < n_status ? status[i] : NTK_JPEG_STATUS_BAD_DESC);
        if (is_dead) {
            active[at] = 0;
            masked += 1;
        } else if (s != 0) {
            active[at] = 0;
            if (first_failed < 0) {
                first_failed = decoded + failed + masked;
                first_status = s;
            }
            failed += 1;
        } else {
            decoded += 1;
        }
    }
    row[NTK_CLIPDEC_DECODED] = decoded;
    row[NTK_CLIPDEC_FAILED] = failed;
    row[NTK_CLIPDEC_MASKED] = masked;
    row[NTK_CLIPDEC_FIRST_FAILED] = first_failed;
    row[NTK_CLIPDEC_FIRST_STATUS] = first_status;
}

extern "C" int ntk_track_poly_bounds(const double* poly, int n, double* rects, void* stream) {
    NTK_REQUIRE(poly && rects, NTK_ERR_BAD_PTR, "ntk_track_poly_bounds: null pointer");
    NTK_REQUIRE(n > 0, NTK_ERR_BAD_SHAPE, "ntk_track_poly_bounds: n=%d", n);
    track_poly_bounds_kernel<<<(n + 63) / 64, 64, 0, (hipStream_t)stream>>>(poly, n, rects);
    NTK_CHECK_LAUNCH("ntk_track_poly_bounds");
    return NTK_OK;
}

template <Gt KIND>
static int track_overlap_scores(const char* name, const double* regions, const double* gt, const double* overlap,
                                const unsigned char* active, const int* clip_of, int T, int B, int n_clips, const double* iou_thr,
                                int n_iou, const double* dist_thr, int n_dist, double* table, double* frame_iou, void* stream) {
    NTK_REQUIRE(regions && gt && clip_of && table && (KIND != Gt::MASK || overlap), NTK_ERR_BAD_PTR, "%s: null pointer", name);
    NTK_REQUIRE(T > 0 && B > 0 && B <= 65535 && n_clips > 0, NTK_ERR_BAD_SHAPE, "%s: T=%d B=%d (1..65535) n_clips=%d", name, T, B, n_clips);
    NTK_REQUIRE(n_iou >= 0 && n_iou <= NTK_SCORE_MAX_THRESHOLDS && n_dist >= 0 && n_dist <= NTK_SCORE_MAX_THRESHOLDS, NTK_ERR_BAD_SHAPE,
                "%s: n_iou=%d n_dist=%d (0..%d each)", name, n_iou, n_dist, NTK_SCORE_MAX_THRESHOLDS);
    NTK_REQUIRE((n_iou == 0 || iou_thr) && (n_dist == 0 || dist_thr), NTK_ERR_BAD_SHAPE, "%s: n_iou=%d n_dist=%d but %s is null", name,
                n_iou, n_dist, (n_iou > 0 && !iou_thr) ? "iou_thr" : "dist_thr");
    track_overlap_scores_kernel<KIND><<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(regions, gt, overlap, active, clip_of, T, B, n_clips,
                                                                                    iou_thr, n_iou, dist_thr, n_dist, table, frame_iou);
    NTK_CHECK_LAUNCH(name);
    return NTK_OK;
}

extern "C" int ntk_track_overlap_scores(const double* regions, const double* gt, const unsigned char* active, const int* clip_of,
                                        int T, int B, int n_clips, const double* iou_thr, int n_iou, const double* dist_thr,
                                        int n_dist, double* table, double* frame_iou, void* stream) {
    return track_overlap_scores<Gt::RECT>("ntk_track_overlap_scores", regions, gt, nullptr, active, clip_of, T, B, n_clips, iou_thr, n_iou,
                                          dist_thr, n_dist, table, frame_iou, stream);
}

extern "C" int ntk_track_overlap_scores_poly(const double* regions, const double* gt, const unsigned char* active, const int* clip_of,
                                             int T, int B, int n_clips, const double* iou_thr, int n_iou, const double* dist_thr,
                                             int n_dist, double* table, double* frame_iou, void* stream) {
    return track_overlap_scores<Gt::POLY>("ntk_track_overlap_scores_poly", regions, gt, nullptr, active, clip_of, T, B, n_clips, iou_thr,
                                          n_iou, dist_thr, n_dist, table, frame_iou, stream);
}

extern "C" int ntk_track_overlap_scores_mask(const double* regions, const double* rects, const double* overlap,
                                             const unsigned char* active, const int* clip_of, int T, int B, int n_clips,
                                             const double* iou_thr, int n_iou, const double* dist_thr, int n_dist, double* table,
                                             double* frame_iou, void* stream) {
    return track_overlap_scores<Gt::MASK>("ntk_track_overlap_scores_mask", regions, rects, overlap, active, clip_of, T, B, n_clips, iou_thr,
                                          n_iou, dist_thr, n_dist, table, frame_iou, stream);
}

template <Gt KIND>
static int track_supervise(const char* name, int phase, const double* regions, const double* gt, const double* overlap,
                           const unsigned char* active, const int* clip_of, int B, int n_clips, int skip, int burn_in, double failure_overlap, int* state,
                           double* table, unsigned char* track, unsigned char* restart, signed char* codes, double* frame_iou,
                           void* stream) {
    NTK_REQUIRE(phase == NTK_SUP_PLAN || phase == NTK_SUP_JUDGE, NTK_ERR_BAD_SHAPE, "%s: phase=%d (NTK_SUP_PLAN or NTK_SUP_JUDGE)", name,
                phase);
    NTK_REQUIRE(gt && clip_of && state && table && track && (phase == NTK_SUP_PLAN ? restart != nullptr : regions != nullptr) &&
                    (KIND != Gt::MASK || phase == NTK_SUP_PLAN || overlap),
                NTK_ERR_BAD_PTR, "%s: null pointer", name);
    NTK_REQUIRE(B > 0 && B <= 65535 && n_clips > 0, NTK_ERR_BAD_SHAPE, "%s: B=%d (1..65535) n_clips=%d", name, B, n_clips);
    NTK_REQUIRE(skip >= 1 && burn_in >= 0 && failure_overlap >= 0 && failure_overlap < 1, NTK_ERR_BAD_SHAPE,
                "%s: skip=%d (>= 1) burn_in=%d (>= 0) failure_overlap=%g (in [0,1))", name, skip, burn_in, failure_overlap);
    if (phase == NTK_SUP_PLAN)
        track_supervise_plan_kernel<KIND><<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(gt, active, clip_of, B, n_clips, state, table,
                                                                                        track, restart, codes, frame_iou);
    else
        track_supervise_judge_kernel<KIND><<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(regions, gt, overlap, track, clip_of, B, n_clips,
                                                                                         skip, burn_in, failure_overlap, state, table,
                                                                                         codes, frame_iou);
    NTK_CHECK_LAUNCH(name);
    return NTK_OK;
}

extern "C" int ntk_track_supervise(int phase, const double* regions, const double* gt, const unsigned char* active,
                                   const int* clip_of, int B, int n_clips, int skip, int burn_in, double failure_overlap,
                                   int* state, double* table, unsigned char* track, unsigned char* restart, signed char* codes,
                                   double* frame_iou, void* stream) {
    return track_supervise<Gt::RECT>("ntk_track_supervise", phase, regions, gt, nullptr, active, clip_of, B, n_clips, skip, burn_in,
                                     failure_overlap, state, table, track, restart, codes, frame_iou, stream);
}

extern "C" int ntk_track_supervise_poly(int phase, const double* regions, const double* gt, const unsigned char* active,
                                        const int* clip_of, int B, int n_clips, int skip, int burn_in, double failure_overlap,
                                        int* state, double* table, unsigned char* track, unsigned char* restart, signed char* codes,
                                        double* frame_iou, void* stream) {
    return track_supervise<Gt::POLY>("ntk_track_supervise_poly", phase, regions, gt, nullptr, active, clip_of, B, n_clips, skip, burn_in,
                                     failure_overlap, state, table, track, restart, codes, frame_iou, stream);
}

extern "C" int ntk_track_supervise_mask(int phase, const double* regions, const double* rects, const double* overlap,
                                        const unsigned char* active, const int* clip_of, int B, int n_clips, int skip, int burn_in,
                                        double failure_overlap, int* state, double* table, unsigned char* track,
                                        unsigned char* restart, signed char* codes, double* frame_iou, void* stream) {
    return track_supervise<Gt::MASK>("ntk_track_supervise_mask", phase, regions, rects, overlap, active, clip_of, B, n_clips, skip, burn_in,
                                     failure_overlap, state, table, track, restart, codes, frame_iou, stream);
}

template <Gt KIND>
static int track_multistart(const char* name, const double* regions, const double* gt, const double* overlap,
                            const unsigned char* active, const int* clip_of, int T, int B, int n_runs, double failure_overlap,
                            int patience, double* table, const long long* trace_first, double* trace, double* frame_iou,
                            void* stream) {
    NTK_REQUIRE(regions && gt && clip_of && table && trace_first && trace && (KIND != Gt::MASK || overlap), NTK_ERR_BAD_PTR,
                "%s: null pointer", name);
    NTK_REQUIRE(T > 0 && B > 0 && B <= 65535 && n_runs > 0, NTK_ERR_BAD_SHAPE, "%s: T=%d B=%d (1..65535) n_runs=%d", name, T, B, n_runs);
    NTK_REQUIRE(patience >= 0 && failure_overlap >= 0 && failure_overlap < 1, NTK_ERR_BAD_SHAPE,
                "%s: patience=%d (>= 0) failure_overlap=%g (in [0,1))", name, patience, failure_overlap);
    track_multistart_kernel<KIND><<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(regions, gt, overlap, active, clip_of, T, B, n_runs,
                                                                                failure_overlap, patience, table, trace_first, trace,
                                                                                frame_iou);
    NTK_CHECK_LAUNCH(name);
    return NTK_OK;
}

extern "C" int ntk_track_multistart(const double* regions, const double* gt, const unsigned char* active, const int* clip_of, int T,
                                    int B, int n_runs, double failure_overlap, int patience, double* table,
                                    const long long* trace_first, double* trace, double* frame_iou, void* stream) {
    return track_multistart<Gt::RECT>("ntk_track_multistart", regions, gt, nullptr, active, clip_of, T, B, n_runs, failure_overlap,
                                      patience, table, trace_first, trace, frame_iou, stream);
}

extern "C" int ntk_track_multistart_poly(const double* regions, const double* gt, const unsigned char* active, const int* clip_of,
                                         int T, int B, int n_runs, double failure_overlap, int patience, double* table,
                                         const long long* trace_first, double* trace, double* frame_iou, void* stream) {
    return track_multistart<Gt::POLY>("ntk_track_multistart_poly", regions, gt, nullptr, active, clip_of, T, B, n_runs, failure_overlap,
                                      patience, table, trace_first, trace, frame_iou, stream);
}

extern "C" int ntk_track_multistart_mask(const double* regions, const double* rects, const double* overlap,
                                         const unsigned char* active, const int* clip_of, int T, int B, int n_runs,
                                         double failure_overlap, int patience, double* table, const long long* trace_first,
                                         double* trace, double* frame_iou, void* stream) {
    return track_multistart<Gt::MASK>("ntk_track_multistart_mask", regions, rects, overlap, active, clip_of, T, B, n_runs,
                                      failure_overlap, patience, table, trace_first, trace, frame_iou, stream);
}

extern "C" int ntk_track_decode_mask(const int* status, int n_status, const int* cell_index, const int* start_index,
                                     const int* clip_of, int T, int B, int n_clips, unsigned char* dead, unsigned char* active,
                                     long long* table, void* stream) {
    NTK_REQUIRE(status && cell_index && start_index && clip_of && dead && active && table, NTK_ERR_BAD_PTR,
                "ntk_track_decode_mask: null pointer");
    NTK_REQUIRE(T > 0 && B > 0 && B <= 65535 && n_clips > 0 && n_status > 0, NTK_ERR_BAD_SHAPE,
                "ntk_track_decode_mask: T=%d B=%d (1..65535) n_clips=%d n_status=%d", T, B, n_clips, n_status);
    track_decode_mask_kernel<<<(B + 63) / 64, 64, 0, (hipStream_t)stream>>>(status, n_status, cell_index, start_index, clip_of, T, B,
                                                                           n_clips, dead, active, table);
    NTK_CHECK_LAUNCH("ntk_track_decode_mask");
    return NTK_OK;
}
