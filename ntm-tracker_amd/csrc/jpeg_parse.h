// Host half of the device JPEG decoder: walk the markers of one baseline file, fill the fixed-size descriptor the kernels read
// (include/ntmtrack.h, NTK_JPEG_DESC_*) and copy the scan's entropy-coded bytes with the stuffing removed, split at the restart
// markers.  Pure host code, no device types: jpeg_decode.hip exports it as ntk_jpeg_parse, and tests/host/jpeg_decode_check.cpp runs
// it under the address and undefined-behaviour sanitizers.  Every read is checked against the file's length first.
#pragma once

#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "../../include/ntmtrack.h"

// One Huffman table in the form the segment decoder reads (jpeg_entropy.h): look[b] = (length << 8) | value for the code that the 8
// bits b start with (0: the code is longer than 8 bits); for a longer code of length l, code <= maxcode[l] decides the length
// (-1: no code of that length) and val[(code + valoff[l]) & 255] is the value.
struct NtkJpegHuff {
    uint16_t look[256];
    int32_t maxcode[18];
    int32_t valoff[18];
    uint8_t val[256];
};

struct NtkJpegDesc {
    int32_t hdr[NTK_JPEG_DESC_HDR_WORDS];
    uint16_t quant[4][64];       // natural (row-major) order
    NtkJpegHuff huff[8];         // 0..3 DC, 4..7 AC
};
static_assert(sizeof(NtkJpegDesc) == NTK_JPEG_DESC_BYTES, "NTK_JPEG_DESC_BYTES is the descriptor's size");

// zigzag position -> natural (row-major) position
static const uint8_t kJpegNaturalOrder[64] = {
    0,  1,  8,  16, 9,  2,  3,  10, 17, 24, 32, 25, 18, 11, 4,  5,  12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6,  7,  14, 21, 28,
    35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63};

#define NTK_JPEG_BAD(...)                                   \
    do {                                                    \
        if (err && errn > 0) snprintf(err, errn, __VA_ARGS__); \
        return NTK_ERR_BAD_DATA;                            \
    } while (0)

static inline void jpeg_hdr_set64(int32_t* hdr, int word, long long v) { memcpy(hdr + word, &v, sizeof(v)); }
static inline long long jpeg_hdr_get64_host(const int32_t* hdr, int word) {
    long long v;
    memcpy(&v, hdr + word, sizeof(v));
    return v;
}

// counts[16] codes per length, vals[nvals] in code order -> table; false: more codes of a length than that length has room for
static inline bool jpeg_build_huff(NtkJpegHuff* t, const uint8_t* counts, const uint8_t* vals) {
    memset(t, 0, sizeof(*t));
    for (int l = 0; l < 18; ++l) t->maxcode[l] = -1;
    int code = 0, k = 0;
    for (int l = 1; l <= 16; ++l) {
        const int n = counts[l - 1];
        if (code + n > (1 << l)) return false;
        if (n) {
            t->valoff[l] = k - code;
            t->maxcode[l] = code + n - 1;
            if (l <= 8)
                for (int i = 0; i < n; ++i)
                    for (int j = 0; j < (1 << (8 - l)); ++j)
                        t->look[((code + i) << (8 - l)) | j] = (uint16_t)((l << 8) | vals[k + i]);
            for (int i = 0; i < n; ++i) t->val[k + i] = vals[k + i];
        }
        k += n;
        code = (code + n) << 1;
    }
    return true;
}

// See ntk_jpeg_parse in include/ntmtrack.h.  `err` (errn bytes, nullable) receives the reason of NTK_ERR_BAD_DATA / _BAD_SHAPE.
static inline int jpeg_parse(const uint8_t* f, long long nb, NtkJpegDesc* d, uint8_t* dst, long long dst_cap, int32_t* seg, int seg_cap,
                             long long* stream_bytes, int* n_segments, char* err, int errn) {
    if (d) memset(d->hdr, 0, sizeof(d->hdr));
    if (stream_bytes) *stream_bytes = 0;
    if (n_segments) *n_segments = 0;
    if (nb < 4 || nb >= 2147483647LL || f[0] != 0xFF || f[1] != 0xD8) return NTK_JPEG_HOST_PATH;
    long long pos = 2;
    bool have_sof = false, jfif = false, adobe = false;
    int H = 0, W = 0, nc = 0, restart = 0;
    int cid[3] = {0, 0, 0}, ch[3] = {1, 1, 1}, cv[3] = {1, 1, 1}, tq[3] = {0, 0, 0}, td[3] = {0, 0, 0}, ta[3] = {0, 0, 0};
    bool qdef[4] = {false, false, false, false}, hdef[8] = {false, false, false, false, false, false, false, false};
    // scratch tables when the caller wants no descriptor
    NtkJpegDesc local;
    NtkJpegDesc* D = d ? d : &local;
    for (;;) {
        if (pos + 2 > nb) NTK_JPEG_BAD("the file ends before the scan (byte %lld)", pos);
        if (f[pos] != 0xFF) NTK_JPEG_BAD("no marker at byte %lld", pos);
        while (pos + 2 < nb && f[pos + 1] == 0xFF) ++pos;          // fill bytes
        const int m = f[pos + 1];
        pos += 2;
        if (m == 0x01 || (m >= 0xD0 && m <= 0xD7)) continue;       // stand-alone
        if (m == 0xD8 || m == 0xD9 || m == 0x00 || m == 0xFF) NTK_JPEG_BAD("marker FF%02X before the scan (byte %lld)", m, pos - 2);
        if (pos + 2 > nb) NTK_JPEG_BAD("the file ends inside a segment header (byte %lld)", pos);
        const int L = (f[pos] << 8) | f[pos + 1];
        if (L < 2 || pos + L > nb) NTK_JPEG_BAD("segment FF%02X at byte %lld: length %d leaves the file of %lld bytes", m, pos - 2, L, nb);
        const uint8_t* b = f + pos + 2;
        const int n = L - 2;
        pos += L;
        if (m == 0xC0) {
            if (have_sof) NTK_JPEG_BAD("a second frame header");
            if (n < 6) NTK_JPEG_BAD("frame header of %d bytes", n);
            const int precision = b[0];
            H = (b[1] << 8) | b[2];
            W = (b[3] << 8) | b[4];
            nc = b[5];
            if (n != 6 + 3 * nc) NTK_JPEG_BAD("frame header: %d components in %d bytes", nc, n);
            if (precision != 8 || (nc != 1 && nc != 3) || H == 0) return NTK_JPEG_HOST_PATH;
            if (W == 0) NTK_JPEG_BAD("frame header: width 0");
            for (int c = 0; c < nc; ++c) {
                cid[c] = b[6 + 3 * c];
                ch[c] = b[7 + 3 * c] >> 4;
                cv[c] = b[7 + 3 * c] & 15;
                tq[c] = b[8 + 3 * c];
                if (tq[c] > 3) NTK_JPEG_BAD("frame header: quantisation table index %d", tq[c]);
                if (ch[c] < 1 || ch[c] > 4 || cv[c] < 1 || cv[c] > 4) NTK_JPEG_BAD("frame header: sampling %dx%d", ch[c], cv[c]);
            }
            if (nc == 1) {
                ch[0] = cv[0] = 1;                                  // a single component is never interleaved: one block per MCU
            } else {
                if (ch[1] != 1 || cv[1] != 1 || ch[2] != 1 || cv[2] != 1) return NTK_JPEG_HOST_PATH;
                if (!((ch[0] == 1 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 1) || (ch[0] == 2 && cv[0] == 2))) return NTK_JPEG_HOST_PATH;
            }
            if (H < NTK_JPEG_MIN_SIDE || W < NTK_JPEG_MIN_SIDE) return NTK_JPEG_HOST_PATH;
            have_sof = true;
        } else if ((m >= 0xC1 && m <= 0xCF && m != 0xC4 && m != 0xC8) || m == 0xDC) {
            return NTK_JPEG_HOST_PATH;                              // any other SOF, arithmetic conditioning, DNL
        } else if (m == 0xDB) {
            int i = 0;
            while (i < n) {
                const int pq = b[i] >> 4, t = b[i] & 15;
                if (t > 3) NTK_JPEG_BAD("quantisation table index %d", t);
                if (pq == 1) return NTK_JPEG_HOST_PATH;
                if (pq > 1) NTK_JPEG_BAD("quantisation table precision %d", pq);
                if (i + 65 > n) NTK_JPEG_BAD("quantisation table %d ends after %d of 64 values", t, n - i - 1);
                for (int k = 0; k < 64; ++k) D->quant[t][kJpegNaturalOrder[k]] = b[i + 1 + k];
                qdef[t] = true;
                i += 65;
            }
        } else if (m == 0xC4) {
            int i = 0;
            while (i < n) {
                const int tc = b[i] >> 4, t = b[i] & 15;
                if (tc > 1 || t > 3) NTK_JPEG_BAD("Huffman table class %d index %d", tc, t);
                if (i + 17 > n) NTK_JPEG_BAD("Huffman table %d/%d ends inside its counts", tc, t);
                int total = 0;
                for (int k = 0; k < 16; ++k) total += b[i + 1 + k];
                if (total > 256) NTK_JPEG_BAD("Huffman table %d/%d: %d codes (at most 256)", tc, t, total);
                if (i + 17 + total > n) NTK_JPEG_BAD("Huffman table %d/%d: %d values in %d bytes", tc, t, total, n - i - 17);
                if (!jpeg_build_huff(&D->huff[tc * 4 + t], b + i + 1, b + i + 17))
                    NTK_JPEG_BAD("Huffman table %d/%d: more codes of a length than fit", tc, t);
                if (tc == 0)
                    for (int k = 0; k < total; ++k)
                        if (b[i + 17 + k] > 11) NTK_JPEG_BAD("Huffman table 0/%d: DC category %d", t, b[i + 17 + k]);
                hdef[tc * 4 + t] = true;
                i += 17 + total;
            }
        } else if (m == 0xDD) {
            if (n != 2) NTK_JPEG_BAD("restart interval segment of %d bytes", n);
            restart = (b[0] << 8) | b[1];
        } else if (m == 0xE0) {
            if (n >= 5 && memcmp(b, "JFIF\0", 5) == 0) jfif = true;
        } else if (m == 0xEE) {
            if (n >= 5 && memcmp(b, "Adobe", 5) == 0) adobe = true;
        } else if (m == 0xDA) {
            if (!have_sof) NTK_JPEG_BAD("a scan before the frame header");
            if (n < 1 || n != 4 + 2 * b[0]) NTK_JPEG_BAD("scan header of %d bytes", n);
            if (b[0] != nc) return NTK_JPEG_HOST_PATH;
            for (int c = 0; c < nc; ++c) {
                if (b[1 + 2 * c] != cid[c]) return NTK_JPEG_HOST_PATH;
                td[c] = b[2 + 2 * c] >> 4;
                ta[c] = b[2 + 2 * c] & 15;
                if (td[c] > 3 || ta[c] > 3) NTK_JPEG_BAD("scan header: Huffman table index %d/%d", td[c], ta[c]);
                if (!qdef[tq[c]] || !hdef[td[c]] || !hdef[4 + ta[c]]) NTK_JPEG_BAD("component %d uses a table the file does not define", c);
            }
            if (b[1 + 2 * nc] != 0 || b[2 + 2 * nc] != 63 || b[3 + 2 * nc] != 0) return NTK_JPEG_HOST_PATH;
            if (nc == 3 && !(jfif || (!adobe && cid[0] == 1 && cid[1] == 2 && cid[2] == 3))) return NTK_JPEG_HOST_PATH;
            break;
        }
    }
    const int hs = ch[0], vs = cv[0];
    const int mcus_x = (W + 8 * hs - 1) / (8 * hs), mcus_y = (H + 8 * vs - 1) / (8 * vs);
    const long long total = (long long)mcus_x * mcus_y;
    const long long expected = restart ? (total + restart - 1) / restart : 1;

    // the scan: copy up to the first marker that is not a restart, without the stuffing
    long long out = 0;
    int ns = 0;
    bool out_of_sequence = false;
    long long p = pos;
    for (;;) {
        if (seg) {
            if (ns >= seg_cap) {
                if (err && errn > 0) snprintf(err, errn, "segment table of %d entries is too short", seg_cap);
                return NTK_ERR_BAD_SHAPE;
            }
            seg[ns] = (int32_t)out;
        }
        ++ns;
        bool more = false;
        while (p < nb) {
            const uint8_t* q = (const uint8_t*)memchr(f + p, 0xFF, (size_t)(nb - p));
            const long long run = q ? (long long)(q - (f + p)) : nb - p;
            if (dst) {
                if (out + run > dst_cap) {
                    if (err && errn > 0) snprintf(err, errn, "stream destination of %lld bytes is too short", dst_cap);
                    return NTK_ERR_BAD_SHAPE;
                }
                memcpy(dst + out, f + p, (size_t)run);
            }
            out += run;
            p += run;
            if (p + 1 >= nb) { p = nb; break; }                   // the file ends, perhaps on a lone FF
            const int c2 = f[p + 1];
            if (c2 == 0x00) {
                if (dst) {
                    if (out >= dst_cap) {
                        if (err && errn > 0) snprintf(err, errn, "stream destination of %lld bytes is too short", dst_cap);
                        return NTK_ERR_BAD_SHAPE;
                    }
                    dst[out] = 0xFF;
                }
                ++out;
                p += 2;
            } else if (c2 == 0xFF) {
                ++p;
            } else if (c2 >= 0xD0 && c2 <= 0xD7) {
                if (c2 - 0xD0 != ((ns - 1) & 7)) out_of_sequence = true;
                p += 2;
                more = true;
                break;
            } else {
                break;                                            // any other marker ends the scan
            }
        }
        if (!more) break;
        if (ns > 65535 * 64) return NTK_JPEG_HOST_PATH;
    }
    if (seg) {
        if (ns >= seg_cap) {
            if (err && errn > 0) snprintf(err, errn, "segment table of %d entries is too short", seg_cap);
            return NTK_ERR_BAD_SHAPE;
        }
        seg[ns] = (int32_t)out;
    }
    if (out_of_sequence || ns > expected) return NTK_JPEG_HOST_PATH;
    // what follows the scan: a second scan or a DNL makes the file the host's; anything unreadable is ignored as libjpeg ignores it
    while (p + 4 <= nb && f[p] == 0xFF) {
        const int m = f[p + 1];
        if (m == 0xFF) { ++p; continue; }
        if (m == 0xD9) break;
        if (m == 0xDA || m == 0xDC) return NTK_JPEG_HOST_PATH;
        const int L = (f[p + 2] << 8) | f[p + 3];
        if (L < 2) break;
        p += 2 + (long long)L;
    }
    if (stream_bytes) *stream_bytes = out;
    if (n_segments) *n_segments = ns;
    if (d) {
        int32_t* h = d->hdr;
        h[NTK_JPEG_DESC_H] = H;
        h[NTK_JPEG_DESC_W] = W;
        h[NTK_JPEG_DESC_NCOMP] = nc;
        h[NTK_JPEG_DESC_HS] = hs;
        h[NTK_JPEG_DESC_VS] = vs;
        h[NTK_JPEG_DESC_RESTART] = restart;
        h[NTK_JPEG_DESC_MCUS_X] = mcus_x;
        h[NTK_JPEG_DESC_MCUS_Y] = mcus_y;
        h[NTK_JPEG_DESC_NSEG] = ns;
        h[NTK_JPEG_DESC_STREAM_BYTES] = (int32_t)out;
        for (int c = 0; c < 3; ++c) {
            h[NTK_JPEG_DESC_TQ + c] = tq[c];
            h[NTK_JPEG_DESC_TD + c] = td[c];
            h[NTK_JPEG_DESC_TA + c] = ta[c];
        }
    }
    return NTK_OK;
}
