// Baseline JPEG on the device: ntk_jpeg_parse (host, jpeg_parse.h), ntk_jpeg_decode_workspace_bytes (host) and
// ntk_jpeg_decode_batch -- three launches over the frames of a batch:
//   jpeg_entropy_kernel   one wave per frame; lane l decodes restart segments l, l + 64, ... (jpeg_entropy.h) into int16
//                         coefficients of the frame's MCU window; the frame's Huffman tables sit in LDS
//   jpeg_idct_kernel      one thread per 8x8 block: dequantise, 13-bit fixed-point inverse DCT (columns descaled by 11 bits, rows by
//                         18), + 128, clamp -> uint8 planes of the window
//   jpeg_colour_kernel    one thread per pixel of the rectangle: triangle chroma upsampling, YCbCr -> RGB, three byte stores
// All arithmetic is int32 in plain C++, libjpeg's default pipeline restated (include/ntmtrack.h).  Every kernel validates the frame
// (jpeg_frame_check) before it touches anything: a frame that leaves the sizes the entry was given is skipped.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "common.h"
#include "jpeg_entropy.h"

namespace {

struct JpegFrame {
    const NtkJpegDesc* d;
    JpegWindow win;
    int y0, x0, h, w;
    long long pix_off;
    int16_t* coef;
    uint8_t* planes;
    int status;                  // NTK_JPEG_STATUS_OK: the fields above are valid and every range is inside the buffers
    bool skip;                   // a frame the host decoded
};

struct JpegBatch {
    const unsigned char* streams;
    long long streams_bytes;
    const NtkJpegDesc* descs;
    const int* segments;
    long long n_segments;
    const long long* table;
    unsigned char* pixels;
    long long pixels_bytes;
    unsigned char* ws;
    long long ws_bytes;
    int* status;
};

// hdr: the frame's header words (global or LDS)
__device__ JpegFrame jpeg_frame_check(const JpegBatch& B, int f, const int32_t* hdr) {
    JpegFrame F;
    F.d = B.descs + f;
    F.skip = hdr[NTK_JPEG_DESC_NCOMP] == 0;
    F.status = NTK_JPEG_STATUS_BAD_DESC;
    F.coef = nullptr;
    F.planes = nullptr;
    F.win = JpegWindow{0, 0, 0, 0};
    F.y0 = F.x0 = F.h = F.w = 0;
    F.pix_off = 0;
    if (F.skip) { F.status = NTK_JPEG_STATUS_OK; return F; }
    if (!jpeg_desc_ok(hdr)) return F;
    const long long* row = B.table + (size_t)f * NTK_FRAME_TABLE_COLS;
    const long long off = row[0], y0 = row[3], x0 = row[4], h = row[5], w = row[6];
    if (!jpeg_rect_ok(hdr, row[1], row[2], y0, x0, h, w)) return F;
    if (off < 0 || off > B.pixels_bytes || h * w * 3 > B.pixels_bytes - off) return F;
    const long long so = jpeg_hdr_get64(hdr, NTK_JPEG_DESC_STREAM_OFF), sb = hdr[NTK_JPEG_DESC_STREAM_BYTES];
    if (so < 0 || so > B.streams_bytes || sb > B.streams_bytes - so) return F;
    const long long sf = hdr[NTK_JPEG_DESC_SEG_FIRST], ns = hdr[NTK_JPEG_DESC_NSEG];
    if (sf < 0 || sf > B.n_segments || ns + 1 > B.n_segments - sf) return F;
    F.y0 = (int)y0; F.x0 = (int)x0; F.h = (int)h; F.w = (int)w;
    F.pix_off = off;
    F.win = jpeg_window(hdr, F.y0, F.x0, F.h, F.w);
    const long long blocks = jpeg_window_blocks(hdr, F.win);
    const long long wo = jpeg_hdr_get64(hdr, NTK_JPEG_DESC_WS_OFF);
    F.status = NTK_JPEG_STATUS_WORKSPACE;
    if (wo < 0 || (wo & 15) || wo > B.ws_bytes || blocks * NTK_JPEG_WS_BYTES_PER_BLOCK > B.ws_bytes - wo) return F;
    F.coef = reinterpret_cast<int16_t*>(B.ws + wo);
    F.planes = B.ws + wo + blocks * 128;
    F.status = NTK_JPEG_STATUS_OK;
    return F;
}

__global__ __launch_bounds__(64) void jpeg_entropy_kernel(JpegBatch B) {
    __shared__ int32_t s_hdr[NTK_JPEG_DESC_HDR_WORDS];
    __shared__ __attribute__((aligned(16))) NtkJpegHuff s_huff[8];
    __shared__ uint8_t s_natural[64];
    const int f = blockIdx.x, lane = threadIdx.x;
    const NtkJpegDesc* d = B.descs + f;
    if (lane < NTK_JPEG_DESC_HDR_WORDS) s_hdr[lane] = d->hdr[lane];
    {   // zigzag position -> natural position, computed (no table in memory to copy): walk the anti-diagonals
        if (lane == 0) {
            int k = 0;
            for (int sum = 0; sum < 15; ++sum)
                for (int i = 0; i <= sum; ++i) {
                    const int y = (sum & 1) ? i : sum - i, x = sum - y;
                    if (y < 8 && x < 8) s_natural[k++] = (uint8_t)(y * 8 + x);
                }
        }
    }
    __syncthreads();
    const JpegFrame F = jpeg_frame_check(B, f, s_hdr);
    if (F.skip) return;
    if (F.status != NTK_JPEG_STATUS_OK) {
        if (lane == 0) B.status[f] = F.status;
        return;
    }
    {
        const uint32_t* src = reinterpret_cast<const uint32_t*>(d->huff);
        uint32_t* dst = reinterpret_cast<uint32_t*>(s_huff);
        for (int i = lane; i < (int)(sizeof(s_huff) / 4); i += 64) dst[i] = src[i];
    }
    __syncthreads();
    const int mcus_x = s_hdr[NTK_JPEG_DESC_MCUS_X];
    const int total = mcus_x * s_hdr[NTK_JPEG_DESC_MCUS_Y];
    const int interval = s_hdr[NTK_JPEG_DESC_RESTART] > 0 ? s_hdr[NTK_JPEG_DESC_RESTART] : total;
    const int stop = (F.win.my0 + F.win.myn) * mcus_x;           // nothing below the window's last MCU row is decoded
    const int start = F.win.my0 * mcus_x;
    const int needed = (stop + interval - 1) / interval;          // segments up to the window's end
    const int nseg = s_hdr[NTK_JPEG_DESC_NSEG];
    const int sbytes = s_hdr[NTK_JPEG_DESC_STREAM_BYTES];
    const unsigned char* s = B.streams + jpeg_hdr_get64(s_hdr, NTK_JPEG_DESC_STREAM_OFF);
    const int* seg = B.segments + s_hdr[NTK_JPEG_DESC_SEG_FIRST];
    if (lane == 0 && nseg < needed) B.status[f] = NTK_JPEG_STATUS_SEGMENTS;
    for (int k = lane; k < needed && k < nseg; k += 64) {
        const int first = k * interval;
        int last = first + interval;
        if (last > stop) last = stop;
        if (last <= start) continue;                             // the whole segment lies above the window
        int begin = seg[k], end = seg[k + 1];
        begin = begin < 0 ? 0 : (begin > sbytes ? sbytes : begin);
        end = end < begin ? begin : (end > sbytes ? sbytes : end);
        const int st = jpeg_decode_segment(s_hdr, s_huff, s_natural, s, begin, end, first, last, F.win, F.coef);
        if (st != NTK_JPEG_STATUS_OK) B.status[f] = st;
    }
}

// libjpeg's "slow integer" inverse DCT of 8 values, 13-bit constants; the results are descaled by `shift` bits with rounding
template <int SHIFT>
__device__ __forceinline__ void jpeg_idct8(int& v0, int& v1, int& v2, int& v3, int& v4, int& v5, int& v6, int& v7) {
    int z2 = v2, z3 = v6;
    int z1 = (z2 + z3) * 4433;
    int tmp2 = z1 - z3 * 15137;
    int tmp3 = z1 + z2 * 6270;
    z2 = v0; z3 = v4;
    int tmp0 = (z2 + z3) * 8192;
    int tmp1 = (z2 - z3) * 8192;
    const int tmp10 = tmp0 + tmp3, tmp13 = tmp0 - tmp3, tmp11 = tmp1 + tmp2, tmp12 = tmp1 - tmp2;
    tmp0 = v7; tmp1 = v5; tmp2 = v3; tmp3 = v1;
    z1 = tmp0 + tmp3; z2 = tmp1 + tmp2; z3 = tmp0 + tmp2;
    int z4 = tmp1 + tmp3;
    const int z5 = (z3 + z4) * 9633;
    tmp0 *= 2446; tmp1 *= 16819; tmp2 *= 25172; tmp3 *= 12299;
    z1 *= -7373; z2 *= -20995; z3 *= -16069; z4 *= -3196;
    z3 += z5; z4 += z5;
    tmp0 += z1 + z3; tmp1 += z2 + z4; tmp2 += z2 + z3; tmp3 += z1 + z4;
    constexpr int R = 1 << (SHIFT - 1);
    v0 = (tmp10 + tmp3 + R) >> SHIFT; v7 = (tmp10 - tmp3 + R) >> SHIFT;
    v1 = (tmp11 + tmp2 + R) >> SHIFT; v6 = (tmp11 - tmp2 + R) >> SHIFT;
    v2 = (tmp12 + tmp1 + R) >> SHIFT; v5 = (tmp12 - tmp1 + R) >> SHIFT;
    v3 = (tmp13 + tmp0 + R) >> SHIFT; v4 = (tmp13 - tmp0 + R) >> SHIFT;
}

__device__ __forceinline__ uint32_t jpeg_clamp8(int v) { return (uint32_t)(v < 0 ? 0 : (v > 255 ? 255 : v)); }

// plane geometry of a window: Y is (myn * 8 vs) x (mxn * 8 hs), Cb and Cr (myn * 8) x (mxn * 8), one after another
struct JpegPlanes {
    int yw, cw_;                 // row lengths of Y and of a chroma plane
    long long cb, cr;            // byte offsets of Cb and Cr behind Y
};
__device__ __forceinline__ JpegPlanes jpeg_planes(const int32_t* hdr, JpegWindow win) {
    JpegPlanes P;
    P.yw = win.mxn * 8 * hdr[NTK_JPEG_DESC_HS];
    P.cw_ = win.mxn * 8;
    P.cb = (long long)P.yw * win.myn * 8 * hdr[NTK_JPEG_DESC_VS];
    P.cr = P.cb + (long long)P.cw_ * win.myn * 8;
    return P;
}

__global__ __launch_bounds__(256) void jpeg_idct_kernel(JpegBatch B) {
    const int f = blockIdx.y;
    const int32_t* hdr = B.descs[f].hdr;
    const JpegFrame F = jpeg_frame_check(B, f, hdr);
    if (F.skip || F.status != NTK_JPEG_STATUS_OK) return;
    const int hs = hdr[NTK_JPEG_DESC_HS], nc = hdr[NTK_JPEG_DESC_NCOMP];
    const int nluma = nc == 1 ? 1 : hs * hdr[NTK_JPEG_DESC_VS], bpm = nc == 1 ? 1 : nluma + 2;
    const JpegPlanes P = jpeg_planes(hdr, F.win);
    const long long blocks = (long long)F.win.mxn * F.win.myn * bpm;
    for (long long blk = (long long)blockIdx.x * 256 + threadIdx.x; blk < blocks; blk += (long long)gridDim.x * 256) {
        const int b = (int)(blk % bpm);
        const int mcu = (int)(blk / bpm);
        const int wx = mcu % F.win.mxn, wy = mcu / F.win.mxn;
        const int comp = b < nluma ? 0 : b - nluma + 1;
        const uint16_t* q = F.d->quant[hdr[NTK_JPEG_DESC_TQ + comp]];
        const int16_t* c = F.coef + blk * 64;
        int v[64];
#pragma unroll
        for (int i = 0; i < 64; ++i) v[i] = (int)c[i] * (int)q[i];
#pragma unroll
        for (int x = 0; x < 8; ++x) jpeg_idct8<11>(v[x], v[8 + x], v[16 + x], v[24 + x], v[32 + x], v[40 + x], v[48 + x], v[56 + x]);
        uint8_t* dst;
        int pitch;
        if (comp == 0) {
            pitch = P.yw;
            dst = F.planes + (long long)(wy * (nluma / hs) + b / hs) * 8 * pitch + (wx * hs + b % hs) * 8;
        } else {
            pitch = P.cw_;
            dst = F.planes + (comp == 1 ? P.cb : P.cr) + (long long)wy * 8 * pitch + wx * 8;
        }
#pragma unroll
        for (int y = 0; y < 8; ++y) {
            jpeg_idct8<18>(v[8 * y], v[8 * y + 1], v[8 * y + 2], v[8 * y + 3], v[8 * y + 4], v[8 * y + 5], v[8 * y + 6], v[8 * y + 7]);
            uint2 o;
            o.x = jpeg_clamp8(v[8 * y] + 128) | (jpeg_clamp8(v[8 * y + 1] + 128) << 8) | (jpeg_clamp8(v[8 * y + 2] + 128) << 16) |
                  (jpeg_clamp8(v[8 * y + 3] + 128) << 24);
            o.y = jpeg_clamp8(v[8 * y + 4] + 128) | (jpeg_clamp8(v[8 * y + 5] + 128) << 8) | (jpeg_clamp8(v[8 * y + 6] + 128) << 16) |
                  (jpeg_clamp8(v[8 * y + 7] + 128) << 24);
            *reinterpret_cast<uint2*>(dst + (long long)y * pitch) = o;
        }
    }
}

__global__ __launch_bounds__(256) void jpeg_colour_kernel(JpegBatch B) {
    const int f = blockIdx.y;
    const int32_t* hdr = B.descs[f].hdr;
    const JpegFrame F = jpeg_frame_check(B, f, hdr);
    if (F.skip || F.status != NTK_JPEG_STATUS_OK) return;
    const int hs = hdr[NTK_JPEG_DESC_HS], vs = hdr[NTK_JPEG_DESC_VS], nc = hdr[NTK_JPEG_DESC_NCOMP];
    const JpegPlanes P = jpeg_planes(hdr, F.win);
    const int cn_x = (hdr[NTK_JPEG_DESC_W] + 1) >> 1, cn_y = (hdr[NTK_JPEG_DESC_H] + 1) >> 1;   // chroma samples of real data
    const int wy0 = F.win.my0 * 8 * vs, wx0 = F.win.mx0 * 8 * hs;                                // window origin, luma pixels
    const int cy0 = F.win.my0 * 8, cx0 = F.win.mx0 * 8;                                          // and in chroma samples
    const uint8_t* Yp = F.planes;
    unsigned char* out = B.pixels + F.pix_off;
    const long long count = (long long)F.h * F.w;
    for (long long i = (long long)blockIdx.x * 256 + threadIdx.x; i < count; i += (long long)gridDim.x * 256) {
        const int ry = (int)(i / F.w), rx = (int)(i % F.w);
        const int y = F.y0 + ry, x = F.x0 + rx;
        const int Y = Yp[(long long)(y - wy0) * P.yw + (x - wx0)];
        int R = Y, G = Y, Bl = Y;
        if (nc == 3) {
            int cc[2];
#pragma unroll
            for (int p = 0; p < 2; ++p) {
                const uint8_t* C = F.planes + (p == 0 ? P.cb : P.cr);
                auto at = [&](int cy, int cx) { return (int)C[(long long)(cy - cy0) * P.cw_ + (cx - cx0)]; };
                int s;
                if (hs == 1) {
                    s = at(y, x);
                } else if (vs == 1) {
                    const int cx = x >> 1;
                    s = at(y, cx);
                    if (x & 1) { if (cx < cn_x - 1) s = (3 * s + at(y, cx + 1) + 2) >> 2; }
                    else       { if (cx > 0) s = (3 * s + at(y, cx - 1) + 1) >> 2; }
                } else {
                    const int cx = x >> 1, cy = y >> 1;
                    int far = (y & 1) ? cy + 1 : cy - 1;
                    far = far < 0 ? 0 : (far > cn_y - 1 ? cn_y - 1 : far);
                    const int v = 3 * at(cy, cx) + at(far, cx);
                    if (x & 1) s = cx < cn_x - 1 ? (3 * v + 3 * at(cy, cx + 1) + at(far, cx + 1) + 7) >> 4 : (4 * v + 7) >> 4;
                    else       s = cx > 0 ? (3 * v + 3 * at(cy, cx - 1) + at(far, cx - 1) + 8) >> 4 : (4 * v + 8) >> 4;
                }
                cc[p] = s - 128;
            }
            const int cb = cc[0], cr = cc[1];
            R = Y + ((91881 * cr + 32768) >> 16);
            G = Y + ((-22554 * cb - 46802 * cr + 32768) >> 16);
            Bl = Y + ((116130 * cb + 32768) >> 16);
        }
        unsigned char* o = out + i * 3;
        o[0] = (unsigned char)jpeg_clamp8(R);
        o[1] = (unsigned char)jpeg_clamp8(G);
        o[2] = (unsigned char)jpeg_clamp8(Bl);
    }
}

}  // namespace

extern "C" int ntk_jpeg_parse(const unsigned char* file, long long file_bytes, void* desc, unsigned char* stream_dst,
                              long long stream_cap, int* segments, int segment_cap, long long* stream_bytes, int* n_segments) {
    NTK_REQUIRE(file, NTK_ERR_BAD_PTR, "ntk_jpeg_parse: null pointer");
    NTK_REQUIRE(file_bytes >= 0 && (!stream_dst || (stream_cap >= 0 && segments && segment_cap >= 2)), NTK_ERR_BAD_SHAPE,
                "ntk_jpeg_parse: file_bytes=%lld stream_cap=%lld segment_cap=%d (a stream destination needs a segment table of 2 or more)",
                file_bytes, stream_cap, segment_cap);
    char why[400] = "";
    const int rc = jpeg_parse(file, file_bytes, static_cast<NtkJpegDesc*>(desc), stream_dst, stream_cap, stream_dst ? segments : nullptr,
                              segment_cap, stream_bytes, n_segments, why, (int)sizeof(why));
    if (rc < 0) ntk_set_error("ntk_jpeg_parse: %s", why);
    return rc;
}

extern "C" int ntk_jpeg_decode_workspace_bytes(void* descs_host, const long long* frame_table_host, int n, long long* bytes) {
    NTK_REQUIRE(descs_host && frame_table_host && bytes, NTK_ERR_BAD_PTR, "ntk_jpeg_decode_workspace_bytes: null pointer");
    NTK_REQUIRE(n > 0 && n <= 65535, NTK_ERR_BAD_SHAPE, "ntk_jpeg_decode_workspace_bytes: n=%d (1..65535)", n);
    NtkJpegDesc* d = static_cast<NtkJpegDesc*>(descs_host);
    long long off = 0;
    for (int i = 0; i < n; ++i) {
        const long long* row = frame_table_host + (size_t)i * NTK_FRAME_TABLE_COLS;
        long long blocks = 1;                                      // a frame the host decoded keeps one block: no frame has none
        if (d[i].hdr[NTK_JPEG_DESC_NCOMP] != 0) {
            NTK_REQUIRE(jpeg_desc_ok(d[i].hdr), NTK_ERR_BAD_SHAPE, "ntk_jpeg_decode_workspace_bytes: descriptor %d is not one ntk_jpeg_parse wrote", i);
            NTK_REQUIRE(jpeg_rect_ok(d[i].hdr, row[1], row[2], row[3], row[4], row[5], row[6]), NTK_ERR_BAD_SHAPE,
                        "ntk_jpeg_decode_workspace_bytes: frame table row %d: rectangle y0=%lld x0=%lld h=%lld w=%lld of a %lldx%lld image "
                        "does not fit the file's %dx%d", i, row[3], row[4], row[5], row[6], row[1], row[2], d[i].hdr[NTK_JPEG_DESC_H],
                        d[i].hdr[NTK_JPEG_DESC_W]);
            blocks = jpeg_window_blocks(d[i].hdr, jpeg_window(d[i].hdr, (int)row[3], (int)row[4], (int)row[5], (int)row[6]));
        }
        jpeg_hdr_set64(d[i].hdr, NTK_JPEG_DESC_WS_OFF, off);
        off += blocks * NTK_JPEG_WS_BYTES_PER_BLOCK;
    }
    *bytes = off;
    return NTK_OK;
}

extern "C" int ntk_jpeg_decode_batch(const unsigned char* streams, long long streams_bytes, const void* descs, const int* segments,
                                     long long n_segments, const long long* frame_table, unsigned char* pixels, long long pixels_bytes,
                                     void* workspace, long long workspace_bytes, int* status, int n, void* stream) {
    NTK_REQUIRE(streams && descs && segments && frame_table && pixels && workspace && status, NTK_ERR_BAD_PTR,
                "ntk_jpeg_decode_batch: null pointer");
    NTK_REQUIRE(n > 0 && n <= 65535 && streams_bytes > 0 && n_segments > 0 && pixels_bytes > 0, NTK_ERR_BAD_SHAPE,
                "ntk_jpeg_decode_batch: n=%d (1..65535) streams_bytes=%lld n_segments=%lld pixels_bytes=%lld", n, streams_bytes, n_segments,
                pixels_bytes);
    NTK_REQUIRE(workspace_bytes >= (long long)n * NTK_JPEG_WS_BYTES_PER_BLOCK, NTK_ERR_BAD_SHAPE,
                "ntk_jpeg_decode_batch: workspace_bytes=%lld is short of %lld for n=%d", workspace_bytes,
                (long long)n * NTK_JPEG_WS_BYTES_PER_BLOCK, n);
    NTK_REQUIRE((reinterpret_cast<uintptr_t>(workspace) & 15u) == 0 && (reinterpret_cast<uintptr_t>(descs) & 7u) == 0, NTK_ERR_BAD_PTR,
                "ntk_jpeg_decode_batch: workspace must be 16-byte and descs 8-byte aligned");
    hipStream_t st = (hipStream_t)stream;
    JpegBatch B{streams, streams_bytes, static_cast<const NtkJpegDesc*>(descs), segments, n_segments, frame_table, pixels, pixels_bytes,
                static_cast<unsigned char*>(workspace), workspace_bytes, status};
    hipError_t e = hipMemsetAsync(workspace, 0, (size_t)workspace_bytes, st);
    if (e == hipSuccess) e = hipMemsetAsync(status, 0, sizeof(int) * (size_t)n, st);
    if (e != hipSuccess) {
        ntk_set_error("ntk_jpeg_decode_batch: hipMemsetAsync: %s", hipGetErrorString(e));
        return NTK_ERR_HIP;
    }
    jpeg_entropy_kernel<<<(unsigned)n, 64, 0, st>>>(B);
    NTK_CHECK_LAUNCH("ntk_jpeg_decode_batch (entropy)");
    jpeg_idct_kernel<<<dim3(16, (unsigned)n), 256, 0, st>>>(B);
    NTK_CHECK_LAUNCH("ntk_jpeg_decode_batch (idct)");
    jpeg_colour_kernel<<<dim3(64, (unsigned)n), 256, 0, st>>>(B);
    NTK_CHECK_LAUNCH("ntk_jpeg_decode_batch (colour)");
    return NTK_OK;
}
