// The parts of the device JPEG decoder that the host can run as well: the MCU window of a rectangle, the workspace of a frame and the
// Huffman decoding of one restart segment.  jpeg_decode.hip runs them on the device (one lane per segment);
// tests/host/jpeg_decode_check.cpp runs the same functions on the CPU under the address and undefined-behaviour sanitizers, on good
// files and on thousands of corrupted ones, before a GPU sees a malformed stream.
//
// Bounds hold by construction, not by trust in the stream: a stream byte is read only inside [begin, end) of its segment (zeros
// beyond), a coefficient is stored only at an index checked < 64 in a block of the window, a bit pattern no code matches ends the
// segment, and the number of MCUs comes from the descriptor.
#pragma once

#include "jpeg_parse.h"

#if defined(__HIPCC__)
#define NTK_JPEG_HD __host__ __device__ inline
#else
#define NTK_JPEG_HD static inline
#endif

struct JpegWindow {
    int mx0, my0, mxn, myn;      // first MCU column / row, MCU columns / rows
};

NTK_JPEG_HD long long jpeg_hdr_get64(const int32_t* hdr, int word) {
    return (long long)(((unsigned long long)(uint32_t)hdr[word + 1] << 32) | (unsigned long long)(uint32_t)hdr[word]);
}

// One axis of the window: pixels [p0, p0 + n) of a side of `size` pixels with luma sampling s (1 or 2) -> MCUs [first, last].  With
// s = 2 the triangle filter reads one chroma sample beyond the rectangle's on either side, clamped to the ceil(size / 2) samples.
NTK_JPEG_HD void jpeg_window_axis(int p0, int n, int size, int s, int mcus, int* first, int* last) {
    int a = p0, b = p0 + n - 1;
    if (s == 2) {
        const int cn = (size + 1) >> 1;
        a = (p0 >> 1) - 1;
        b = ((p0 + n - 1) >> 1) + 1;
        if (a < 0) a = 0;
        if (b > cn - 1) b = cn - 1;
    }
    a >>= 3;                     // 8 samples of the subsampled axis (or 8 pixels) per MCU
    b >>= 3;
    if (b > mcus - 1) b = mcus - 1;
    if (a > b) a = b;
    *first = a;
    *last = b;
}

// hdr describes an accepted frame and the rectangle lies inside it (jpeg_desc_ok, jpeg_rect_ok)
NTK_JPEG_HD JpegWindow jpeg_window(const int32_t* hdr, int y0, int x0, int h, int w) {
    int a, b;
    JpegWindow win;
    jpeg_window_axis(x0, w, hdr[NTK_JPEG_DESC_W], hdr[NTK_JPEG_DESC_HS], hdr[NTK_JPEG_DESC_MCUS_X], &a, &b);
    win.mx0 = a;
    win.mxn = b - a + 1;
    jpeg_window_axis(y0, h, hdr[NTK_JPEG_DESC_H], hdr[NTK_JPEG_DESC_VS], hdr[NTK_JPEG_DESC_MCUS_Y], &a, &b);
    win.my0 = a;
    win.myn = b - a + 1;
    return win;
}

NTK_JPEG_HD int jpeg_blocks_per_mcu(const int32_t* hdr) {
    return hdr[NTK_JPEG_DESC_NCOMP] == 1 ? 1 : hdr[NTK_JPEG_DESC_HS] * hdr[NTK_JPEG_DESC_VS] + 2;
}

// int16 coefficients (128 bytes a block), then the planes (64 bytes a block): Y, Cb, Cr
NTK_JPEG_HD long long jpeg_window_blocks(const int32_t* hdr, JpegWindow win) {
    return (long long)win.mxn * win.myn * jpeg_blocks_per_mcu(hdr);
}

// the descriptor's own consistency (what jpeg_parse writes); nothing of it is taken on trust by the kernels
NTK_JPEG_HD bool jpeg_desc_ok(const int32_t* h) {
    const int H = h[NTK_JPEG_DESC_H], W = h[NTK_JPEG_DESC_W], nc = h[NTK_JPEG_DESC_NCOMP], hs = h[NTK_JPEG_DESC_HS],
              vs = h[NTK_JPEG_DESC_VS];
    if (H < NTK_JPEG_MIN_SIDE || H > 65535 || W < NTK_JPEG_MIN_SIDE || W > 65535 || (nc != 1 && nc != 3)) return false;
    if (!((hs == 1 && vs == 1) || (nc == 3 && hs == 2 && (vs == 1 || vs == 2)))) return false;
    if (h[NTK_JPEG_DESC_MCUS_X] != (W + 8 * hs - 1) / (8 * hs) || h[NTK_JPEG_DESC_MCUS_Y] != (H + 8 * vs - 1) / (8 * vs)) return false;
    if (h[NTK_JPEG_DESC_RESTART] < 0 || h[NTK_JPEG_DESC_RESTART] > 65535 || h[NTK_JPEG_DESC_NSEG] < 1 ||
        h[NTK_JPEG_DESC_STREAM_BYTES] < 0)
        return false;
    for (int c = 0; c < 3; ++c)
        if ((unsigned)h[NTK_JPEG_DESC_TQ + c] > 3u || (unsigned)h[NTK_JPEG_DESC_TD + c] > 3u || (unsigned)h[NTK_JPEG_DESC_TA + c] > 3u)
            return false;
    return true;
}

NTK_JPEG_HD bool jpeg_rect_ok(const int32_t* hdr, long long H, long long W, long long y0, long long x0, long long h, long long w) {
    return H == hdr[NTK_JPEG_DESC_H] && W == hdr[NTK_JPEG_DESC_W] && h >= 1 && w >= 1 && y0 >= 0 && x0 >= 0 && y0 + h <= H && x0 + w <= W;
}

struct JpegBits {
    uint64_t buf;                // the next bits, left-aligned
    int bits;                    // how many of them are valid
    int pos;                     // next byte to load (may run past `end`: zeros are fed then)
};

NTK_JPEG_HD void jpeg_refill(JpegBits& r, const uint8_t* s, int end) {
    while (r.bits <= 56) {
        const uint64_t b = r.pos < end ? s[r.pos] : 0;
        ++r.pos;
        r.buf |= b << (56 - r.bits);
        r.bits += 8;
    }
}

// n in 1..16; the buffer holds at least 32 bits
NTK_JPEG_HD int jpeg_take(JpegBits& r, int n) {
    const int v = (int)(r.buf >> (64 - n));
    r.buf <<= n;
    r.bits -= n;
    return v;
}

// One Huffman value: >= 0, or -1 when no code matches the next 16 bits
NTK_JPEG_HD int jpeg_symbol(JpegBits& r, const NtkJpegHuff* t) {
    const int e = t->look[(int)(r.buf >> 56)];
    if (e) {
        jpeg_take(r, e >> 8);
        return e & 255;
    }
    for (int l = 9; l <= 16; ++l) {
        const int code = (int)(r.buf >> (64 - l));
        if (code <= t->maxcode[l]) {
            jpeg_take(r, l);
            return t->val[(code + t->valoff[l]) & 255];
        }
    }
    return -1;
}

NTK_JPEG_HD int jpeg_extend(int v, int s) { return v < (1 << (s - 1)) ? v - (1 << s) + 1 : v; }

// MCUs [first, last) of one restart segment: bytes [begin, end) of `s` (the frame's unstuffed stream).  The blocks of MCUs inside `win`
// are stored at coef[((wy * win.mxn + wx) * bpm + block) * 64 + natural index], only their non-zero coefficients (the caller
// cleared them); everything else is decoded and dropped.  `natural`: kJpegNaturalOrder or a copy of it.
// -> NTK_JPEG_STATUS_OK / _BAD_CODE / _TRUNCATED.
NTK_JPEG_HD int jpeg_decode_segment(const int32_t* hdr, const NtkJpegHuff* huff, const uint8_t* natural, const uint8_t* s, int begin,
                                    int end, int first, int last, JpegWindow win, int16_t* coef) {
    const int mcus_x = hdr[NTK_JPEG_DESC_MCUS_X];
    const int nc = hdr[NTK_JPEG_DESC_NCOMP];
    const int nluma = nc == 1 ? 1 : hdr[NTK_JPEG_DESC_HS] * hdr[NTK_JPEG_DESC_VS];
    const int bpm = nc == 1 ? 1 : nluma + 2;
    JpegBits r;
    r.buf = 0;
    r.bits = 0;
    r.pos = begin;
    int pred0 = 0, pred1 = 0, pred2 = 0;
    int mx = first % mcus_x, my = first / mcus_x;
    for (int mcu = first; mcu < last; ++mcu) {
        const int wx = mx - win.mx0, wy = my - win.my0;
        const bool inside = wx >= 0 && wx < win.mxn && wy >= 0 && wy < win.myn;
        for (int b = 0; b < bpm; ++b) {
            const int comp = b < nluma ? 0 : b - nluma + 1;
            const NtkJpegHuff* dc = huff + hdr[NTK_JPEG_DESC_TD + comp];
            const NtkJpegHuff* ac = huff + 4 + hdr[NTK_JPEG_DESC_TA + comp];
            int16_t* blk = inside ? coef + ((long long)(wy * win.mxn + wx) * bpm + b) * 64 : nullptr;
            jpeg_refill(r, s, end);
            int sym = jpeg_symbol(r, dc);
            if (sym < 0) return NTK_JPEG_STATUS_BAD_CODE;
            sym &= 15;
            int diff = 0;
            if (sym) diff = jpeg_extend(jpeg_take(r, sym), sym);
            int pred = comp == 0 ? pred0 : (comp == 1 ? pred1 : pred2);
            pred = (int)(int16_t)(pred + diff);
            if (comp == 0) pred0 = pred; else if (comp == 1) pred1 = pred; else pred2 = pred;
            if (blk && pred) blk[0] = (int16_t)pred;
            int k = 1;
            while (k < 64) {
                jpeg_refill(r, s, end);
                sym = jpeg_symbol(r, ac);
                if (sym < 0) return NTK_JPEG_STATUS_BAD_CODE;
                const int run = sym >> 4, size = sym & 15;
                if (size == 0) {
                    if (run != 15) break;                         // end of block
                    k += 16;
                    continue;
                }
                k += run;
                const int v = jpeg_extend(jpeg_take(r, size), size);
                if (k >= 64) return NTK_JPEG_STATUS_BAD_CODE;
                if (blk) blk[natural[k]] = (int16_t)v;
                ++k;
            }
            // bits taken so far against the bits the segment has
            if ((long long)(r.pos - begin) * 8 - r.bits > (long long)(end - begin) * 8) return NTK_JPEG_STATUS_TRUNCATED;
        }
        if (++mx == mcus_x) { mx = 0; ++my; }
    }
    return NTK_JPEG_STATUS_OK;
}
