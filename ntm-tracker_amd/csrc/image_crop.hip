// The image stages of the trackers' input: tf.image.resize_images and tf.image.crop_and_resize (bilinear, TF-1 defaults) for one
// box, for B trackers, and fused over the frame records of a training batch.
//
// Rounding of the image stages.  The two per-pixel functions below say which operations round: the sample positions and the
// fractions are separate multiplications, additions and subtractions, each rounded (contraction is off inside the functions), and
// each of the three interpolations a + (b - a) * t is ONE fused multiply-add, written as fmaf.  Left to the compiler, the choice
// depends on the code around the inlined function -- it fused `sy - floor(sy)` with the product behind sy in one kernel and not in
// another -- and the same stage would give different bits from different kernels.
#include "common.h"

namespace {      // the accessors and the per-pixel functions; the kernels below keep their external names

// Sources of the image kernels.  A stage reads its input through an accessor, at(y, x, c) -> the fp32 value of one pixel, so that
// a stage is written ONCE and runs the same expressions whether its input lies in memory or is computed on the fly.
// DenseImage: a whole row-major image [H,W,C] in memory; PixelT float, or unsigned char (converted to fp32 exactly).
template <typename PixelT>
struct DenseImage {
    const PixelT* __restrict__ img;
    int W, C;
    __device__ __forceinline__ float at(int y, int x, int c) const { return (float)img[((size_t)y * W + x) * C + c]; }
};

// PackedRect: the sub-rectangle (y0, x0, h, w) of a uint8 image, stored row-major on its own at an arbitrary byte address (byte
// loads only: no alignment is assumed).  Indices are those of the FULL image; each is clamped into the rectangle before the load,
// so no index can leave the h * w * C bytes (a rectangle that covers every tap is read exactly as the full image would be).
struct PackedRect {
    const unsigned char* __restrict__ pix;
    int y0, x0, h, w, C;
    __device__ __forceinline__ float at(int y, int x, int c) const {
        const int yy = min(max(y - y0, 0), h - 1), xx = min(max(x - x0, 0), w - 1);
        return (float)pix[((size_t)yy * w + xx) * C + c];
    }
};

// One output element of tf.image.resize_images(..., BILINEAR) with TF-1 defaults (align_corners=False, no half-pixel centres):
// src = dst * (in / out); neighbours floor(src) and min(floor(src)+1, in-1).  The ONE copy of the per-pixel arithmetic, shared
// by resize_bilinear_kernel and (through ResizedView) by the fused frames kernel.
template <typename Src>
__device__ __forceinline__ float resize_bilinear_pixel(const Src& src, int H, int W, int OH, int OW, int y, int x, int c) {
#pragma clang fp contract(off)      // see "Rounding of the image stages" above: the fused multiply-adds are the three written out
    const float sy = (float)y * ((float)H / (float)OH), sx = (float)x * ((float)W / (float)OW);
    const int y0 = (int)floorf(sy), x0 = (int)floorf(sx);
    const int y1 = min(y0 + 1, H - 1), x1 = min(x0 + 1, W - 1);
    const float fy = sy - (float)y0, fx = sx - (float)x0;
    const float tl = src.at(y0, x0, c), tr = src.at(y0, x1, c);
    const float bl = src.at(y1, x0, c), br = src.at(y1, x1, c);
    const float top = fmaf(fx, tr - tl, tl), bot = fmaf(fx, br - bl, bl);
    return fmaf(fy, bot - top, top);
}

// ResizedView: the [OH,OW,C] bilinear resize of a source [H,W,C] that is never stored: every pixel is computed when it is read.
template <typename Src>
struct ResizedView {
    Src src;
    int H, W, OH, OW;
    __device__ __forceinline__ float at(int y, int x, int c) const { return resize_bilinear_pixel(src, H, W, OH, OW, y, x, c); }
};

// One output element of tf.image.crop_and_resize (bilinear, normalised box y1,x1,y2,x2) of (image - mean): the ONE copy of the
// per-pixel arithmetic, shared by the one-box kernel, the batched kernel and the fused frames kernel, so that the same box on
// the same image gives the same bits from every entry.  src: an accessor (above) of an image [H,W,C].
template <typename Src>
__device__ __forceinline__ float crop_resize_pixel(const Src& src, int H, int W, const float* __restrict__ mean,
                                                   float y1, float x1, float y2, float x2, int ch, int cw, float extrapolation,
                                                   int y, int x, int c) {
#pragma clang fp contract(off)      // see "Rounding of the image stages" above
    const float hs = (ch > 1) ? (y2 - y1) * (float)(H - 1) / (float)(ch - 1) : 0.f;
    const float wsc = (cw > 1) ? (x2 - x1) * (float)(W - 1) / (float)(cw - 1) : 0.f;
    const float in_y = (ch > 1) ? y1 * (float)(H - 1) + (float)y * hs : 0.5f * (y1 + y2) * (float)(H - 1);
    const float in_x = (cw > 1) ? x1 * (float)(W - 1) + (float)x * wsc : 0.5f * (x1 + x2) * (float)(W - 1);
    float v = extrapolation;
    if (in_y >= 0.f && in_y <= (float)(H - 1) && in_x >= 0.f && in_x <= (float)(W - 1)) {
        const int ty = (int)floorf(in_y), by = (int)ceilf(in_y);
        const int lx = (int)floorf(in_x), rx = (int)ceilf(in_x);
        const float yl = in_y - (float)ty, xl = in_x - (float)lx;
        const float m = mean ? mean[c] : 0.f;
        const float tl = src.at(ty, lx, c) - m, tr = src.at(ty, rx, c) - m;
        const float bl = src.at(by, lx, c) - m, br = src.at(by, rx, c) - m;
        const float top = fmaf(xl, tr - tl, tl), bot = fmaf(xl, br - bl, bl);
        v = fmaf(yl, bot - top, top);
    }
    return v;
}

}  // namespace

// tf.image.resize_images(..., BILINEAR) with TF-1 defaults: one thread per output element (resize_bilinear_pixel)
__global__ void resize_bilinear_kernel(const float* __restrict__ img, int H, int W, int C, float* __restrict__ out,
                                       int OH, int OW) {
    const size_t idx = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= (size_t)OH * OW * C) return;
    const int c = (int)(idx % C), x = (int)((idx / C) % OW), y = (int)(idx / ((size_t)C * OW));
    out[idx] = resize_bilinear_pixel(DenseImage<float>{img, W, C}, H, W, OH, OW, y, x, c);
}

// tf.image.crop_and_resize (bilinear, one box) of (image - mean): out[y][x][c], extrapolation outside the image
__global__ void crop_resize_kernel(const float* __restrict__ img, int H, int W, int C, const float* __restrict__ mean,
                                   float y1, float x1, float y2, float x2, float* __restrict__ out, int ch, int cw,
                                   float extrapolation) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    if (idx >= ch * cw * C) return;
    const int c = idx % C, x = (idx / C) % cw, y = idx / (C * cw);
    out[idx] = crop_resize_pixel(DenseImage<float>{img, W, C}, H, W, mean, y1, x1, y2, x2, ch, cw, extrapolation, y, x, c);
}

// The same for B boxes in one launch (blockIdx.y = tracker b): tracker b crops frame frame_of[b] of images [F,H,W,C] to boxes[b]
// (both read from device memory).  A frame index outside [0, F) is never dereferenced: that tracker's crop is the extrapolation value.
template <typename PixelT>
__global__ void crop_resize_batch_kernel(const PixelT* __restrict__ images, int F, int H, int W, int C,
                                         const int* __restrict__ frame_of, const float* __restrict__ boxes,
                                         const float* __restrict__ mean, float* __restrict__ out, int ch, int cw,
                                         float extrapolation) {
    const int idx = blockIdx.x * blockDim.x + threadIdx.x;
    const int total = ch * cw * C;
    if (idx >= total) return;
    const int b = blockIdx.y;
    const int f = frame_of[b];
    float v = extrapolation;
    if (f >= 0 && f < F) {
        const int c = idx % C, x = (idx / C) % cw, y = idx / (C * cw);
        const float* box = boxes + 4 * (size_t)b;
        v = crop_resize_pixel(DenseImage<PixelT>{images + (size_t)f * H * W * C, W, C}, H, W, mean, box[0], box[1], box[2], box[3],
                              ch, cw, extrapolation, y, x, c);
    }
    out[(size_t)b * total + idx] = v;
}

// The training input of n frames in one launch (blockIdx.y = frame, one thread per output pixel, all C channels): the crop of
// (resize(frame) - mean), the resized image [RH,RW,C] never stored -- each of the crop stage's four taps is a pixel of
// ResizedView, computed from four source bytes.  table int64 [n,7]: byte_offset, H, W, y0, x0, h, w (include/ntmtrack.h).  A row
// whose rectangle is empty, leaves its image or leaves [0, pixels_bytes) is never dereferenced: its crop is the extrapolation
// value everywhere (so is one of a frame above 2^30 rows or columns: the stages' int indices stay far from overflow).  flip_x: output
// column x holds crop column cw-1-x.
__global__ void frames_crop_batch_kernel(const unsigned char* __restrict__ pixels, long long pixels_bytes,
                                         const long long* __restrict__ table, const float* __restrict__ boxes,
                                         const float* __restrict__ mean, float* __restrict__ out, int C, int RH, int RW, int ch, int cw,
                                         int flip_x, float extrapolation) {
    const int p = blockIdx.x * blockDim.x + threadIdx.x;
    if (p >= ch * cw) return;
    const int f = blockIdx.y;
    const long long* row = table + 7 * (size_t)f;
    const long long off = row[0], H = row[1], W = row[2], y0 = row[3], x0 = row[4], h = row[5], w = row[6];
    const bool ok = H >= 1 && W >= 1 && H <= (1LL << 30) && W <= (1LL << 30) && h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 &&
                    y0 <= H - h && x0 <= W - w && off >= 0 && off < pixels_bytes && h <= (pixels_bytes - off) / (w * C);
    const int x = p % cw, y = p / cw;
    float* o = out + ((size_t)f * ch * cw + p) * C;
    if (!ok) {
        for (int c = 0; c < C; ++c) o[c] = extrapolation;
        return;
    }
    const ResizedView<PackedRect> view{PackedRect{pixels + off, (int)y0, (int)x0, (int)h, (int)w, C}, (int)H, (int)W, RH, RW};
    const float* box = boxes + 4 * (size_t)f;
    const float by1 = box[0], bx1 = box[1], by2 = box[2], bx2 = box[3];
    const int sx = flip_x ? cw - 1 - x : x;
    for (int c = 0; c < C; ++c)
        o[c] = crop_resize_pixel(view, RH, RW, mean, by1, bx1, by2, bx2, ch, cw, extrapolation, y, sx, c);
}

extern "C" int ntk_resize_bilinear(const float* image, int H, int W, int C, float* out, int out_h, int out_w, void* stream) {
    NTK_REQUIRE(image && out, NTK_ERR_BAD_PTR, "ntk_resize_bilinear: null pointer");
    NTK_REQUIRE(H > 0 && W > 0 && C > 0 && out_h > 0 && out_w > 0, NTK_ERR_BAD_SHAPE, "ntk_resize_bilinear: %dx%dx%d -> %dx%d", H, W, C, out_h, out_w);
    const size_t total = (size_t)out_h * out_w * C;
    resize_bilinear_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(image, H, W, C, out, out_h, out_w);
    NTK_CHECK_LAUNCH("ntk_resize_bilinear");
    return NTK_OK;
}

extern "C" int ntk_crop_and_resize(const float* image, int H, int W, int C, const float* mean, float y1, float x1,
                                   float y2, float x2, float* out, int crop_h, int crop_w, float extrapolation,
                                   void* stream) {
    NTK_REQUIRE(image && out, NTK_ERR_BAD_PTR, "ntk_crop_and_resize: null pointer");
    NTK_REQUIRE(H > 0 && W > 0 && C > 0 && crop_h > 0 && crop_w > 0, NTK_ERR_BAD_SHAPE,
                "ntk_crop_and_resize: H=%d W=%d C=%d crop=%dx%d", H, W, C, crop_h, crop_w);
    const long total = (long)crop_h * crop_w * C;
    NTK_REQUIRE(total < 2147483647L - 256, NTK_ERR_BAD_SHAPE, "ntk_crop_and_resize: crop=%dx%d C=%d: too many elements", crop_h, crop_w, C);
    crop_resize_kernel<<<(unsigned)((total + 255) / 256), 256, 0, (hipStream_t)stream>>>(image, H, W, C, mean, y1, x1, y2, x2, out,
                                                                             crop_h, crop_w, extrapolation);
    NTK_CHECK_LAUNCH("ntk_crop_and_resize");
    return NTK_OK;
}

extern "C" int ntk_crop_and_resize_batch(const void* images, int dtype, int F, int H, int W, int C, const int* frame_of,
                                         const float* boxes, const float* mean, float* out, int B, int crop_h, int crop_w,
                                         float extrapolation, void* stream) {
    NTK_REQUIRE(images && frame_of && boxes && out, NTK_ERR_BAD_PTR, "ntk_crop_and_resize_batch: null pointer");
    NTK_REQUIRE(dtype == NTK_IMAGE_F32 || dtype == NTK_IMAGE_U8, NTK_ERR_BAD_SHAPE,
                "ntk_crop_and_resize_batch: dtype=%d (NTK_IMAGE_F32 or NTK_IMAGE_U8)", dtype);
    NTK_REQUIRE(B > 0 && B <= 65535 && F > 0 && H > 0 && W > 0 && C > 0 && crop_h > 0 && crop_w > 0, NTK_ERR_BAD_SHAPE,
                "ntk_crop_and_resize_batch: B=%d (1..65535) F=%d H=%d W=%d C=%d crop=%dx%d", B, F, H, W, C, crop_h, crop_w);
    const long total = (long)crop_h * crop_w * C;
    NTK_REQUIRE(total < 2147483647L - 256, NTK_ERR_BAD_SHAPE, "ntk_crop_and_resize_batch: crop=%dx%d C=%d: too many elements per box",
                crop_h, crop_w, C);
    const dim3 grid((unsigned)((total + 255) / 256), (unsigned)B);
    if (dtype == NTK_IMAGE_U8)
        crop_resize_batch_kernel<unsigned char><<<grid, 256, 0, (hipStream_t)stream>>>(
            (const unsigned char*)images, F, H, W, C, frame_of, boxes, mean, out, crop_h, crop_w, extrapolation);
    else
        crop_resize_batch_kernel<float><<<grid, 256, 0, (hipStream_t)stream>>>((const float*)images, F, H, W, C, frame_of, boxes, mean,
                                                                               out, crop_h, crop_w, extrapolation);
    NTK_CHECK_LAUNCH("ntk_crop_and_resize_batch");
    return NTK_OK;
}

extern "C" int ntk_frames_crop_batch(const unsigned char* pixels, long long pixels_bytes, const long long* frame_table,
                                     const float* boxes, const float* mean, float* out, int n, int C, int resize_h, int resize_w,
                                     int crop_h, int crop_w, int flip_x, float extrapolation, void* stream) {
    NTK_REQUIRE(pixels && frame_table && boxes && out, NTK_ERR_BAD_PTR, "ntk_frames_crop_batch: null pointer");
    NTK_REQUIRE(n > 0 && n <= 65535 && C > 0 && C <= 4 && resize_h > 0 && resize_w > 0 && crop_h > 0 && crop_w > 0 && pixels_bytes > 0,
                NTK_ERR_BAD_SHAPE, "ntk_frames_crop_batch: n=%d (1..65535) C=%d (1..4) resize=%dx%d crop=%dx%d pixels_bytes=%lld", n, C,
                resize_h, resize_w, crop_h, crop_w, pixels_bytes);
    const long total = (long)crop_h * crop_w * C;
    NTK_REQUIRE(total < 2147483648L - 256, NTK_ERR_BAD_SHAPE, "ntk_frames_crop_batch: crop=%dx%d C=%d: too many elements per frame",
                crop_h, crop_w, C);
    const dim3 grid((unsigned)(((long)crop_h * crop_w + 255) / 256), (unsigned)n);
    frames_crop_batch_kernel<<<grid, 256, 0, (hipStream_t)stream>>>(pixels, pixels_bytes, frame_table, boxes, mean, out, C, resize_h,
                                                                    resize_w, crop_h, crop_w, flip_x ? 1 : 0, extrapolation);
    NTK_CHECK_LAUNCH("ntk_frames_crop_batch");
    return NTK_OK;
}
