// Host check of the device JPEG decoder's bounds: csrc/jpeg_parse.h (marker walk, unstuffing) and csrc/jpeg_entropy.h (the
// per-segment Huffman loop the GPU runs, the MCU window), built with -fsanitize=address,undefined.  Every buffer handed to them is a
// heap block of exactly the size the contract names, so that one byte outside it stops the program.
//   jpeg_decode_check DIR N   DIR/files.txt names the files; each is decoded whole and its coefficients are written to
//                             DIR/<name>.coef (int16 [mcu][block][64], natural order); then N seeded corruptions of every file
//                             (header and scan bytes flipped, truncations, restart intervals that disagree with the data, random
//                             rectangles) go through the parser and the segment decoder.
// Prints "jpeg decode check: ok" and exits 0.
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "jpeg_entropy.h"

static uint64_t g_rng = 0x9E3779B97F4A7C15ull;
static uint32_t rnd() {
    g_rng ^= g_rng << 13;
    g_rng ^= g_rng >> 7;
    g_rng ^= g_rng << 17;
    return (uint32_t)(g_rng >> 16);
}
static int rnd_below(int n) { return n > 0 ? (int)(rnd() % (uint32_t)n) : 0; }

struct Exact {                   // a heap block of exactly n bytes (n = 0 included)
    uint8_t* p;
    explicit Exact(size_t n) : p((uint8_t*)malloc(n)) {}
    ~Exact() { free(p); }
};

struct Counts { long accepted = 0, host = 0, malformed = 0, decoded_ok = 0, flagged = 0; };

// Parse `file` (sizing pass, then the copying pass into exact buffers) and, when accepted, decode the window of rectangle
// (y0, x0, h, w) -- chosen by `pick` from the frame's size -- segment by segment as the kernel does.  -> parser's return code;
// coefficients to `dump` when given.
template <class Pick, class Tweak>
static int run(const std::vector<uint8_t>& file, Pick pick, Tweak tweak, Counts& cnt, std::vector<int16_t>* dump) {
    Exact in(file.size());
    if (!file.empty()) memcpy(in.p, file.data(), file.size());
    char why[256];
    long long sbytes = 0;
    int nseg = 0;
    NtkJpegDesc* d = (NtkJpegDesc*)malloc(sizeof(NtkJpegDesc));
    int rc = jpeg_parse(in.p, (long long)file.size(), d, nullptr, 0, nullptr, 0, &sbytes, &nseg, why, sizeof(why));
    if (rc != NTK_OK) {
        if (rc == NTK_JPEG_HOST_PATH) ++cnt.host; else if (rc == NTK_ERR_BAD_DATA) ++cnt.malformed; else { printf("sizing pass: %d %s\n", rc, why); exit(1); }
        free(d);
        return rc;
    }
    ++cnt.accepted;
    Exact stream((size_t)sbytes);
    Exact segs(sizeof(int32_t) * (size_t)(nseg + 1));
    long long sbytes2 = 0;
    int nseg2 = 0;
    rc = jpeg_parse(in.p, (long long)file.size(), d, stream.p, sbytes, (int32_t*)segs.p, nseg + 1, &sbytes2, &nseg2, why, sizeof(why));
    if (rc != NTK_OK || sbytes2 != sbytes || nseg2 != nseg) { printf("the two passes disagree: %d %lld/%lld %d/%d %s\n", rc, sbytes, sbytes2, nseg, nseg2, why); exit(1); }
    tweak(d->hdr);
    if (!jpeg_desc_ok(d->hdr)) { free(d); return rc; }
    int y0, x0, h, w;
    pick(d->hdr[NTK_JPEG_DESC_H], d->hdr[NTK_JPEG_DESC_W], y0, x0, h, w);
    if (!jpeg_rect_ok(d->hdr, d->hdr[NTK_JPEG_DESC_H], d->hdr[NTK_JPEG_DESC_W], y0, x0, h, w)) { printf("bad rectangle\n"); exit(1); }
    const JpegWindow win = jpeg_window(d->hdr, y0, x0, h, w);
    const int mcus_x = d->hdr[NTK_JPEG_DESC_MCUS_X], mcus_y = d->hdr[NTK_JPEG_DESC_MCUS_Y];
    if (win.mx0 < 0 || win.my0 < 0 || win.mxn < 1 || win.myn < 1 || win.mx0 + win.mxn > mcus_x || win.my0 + win.myn > mcus_y) { printf("window outside the grid\n"); exit(1); }
    const long long blocks = jpeg_window_blocks(d->hdr, win);
    Exact coef((size_t)blocks * 128);
    memset(coef.p, 0, (size_t)blocks * 128);
    // the kernel's segment loop
    const int total = mcus_x * mcus_y;
    const int interval = d->hdr[NTK_JPEG_DESC_RESTART] > 0 ? d->hdr[NTK_JPEG_DESC_RESTART] : total;
    const int stop = (win.my0 + win.myn) * mcus_x, start = win.my0 * mcus_x;
    const int needed = (stop + interval - 1) / interval;
    const int32_t* seg = (const int32_t*)segs.p;
    int status = nseg < needed ? NTK_JPEG_STATUS_SEGMENTS : 0;
    for (int k = 0; k < needed && k < nseg; ++k) {
        const int first = k * interval;
        int last = first + interval;
        if (last > stop) last = stop;
        if (last <= start) continue;
        int begin = seg[k], end = seg[k + 1];
        begin = begin < 0 ? 0 : (begin > sbytes ? (int)sbytes : begin);
        end = end < begin ? begin : (end > sbytes ? (int)sbytes : end);
        const int st = jpeg_decode_segment(d->hdr, d->huff, kJpegNaturalOrder, stream.p, begin, end, first, last, win, (int16_t*)coef.p);
        if (st) status = st;
    }
    if (status) ++cnt.flagged; else ++cnt.decoded_ok;
    if (dump) dump->assign((int16_t*)coef.p, (int16_t*)coef.p + blocks * 64);
    free(d);
    return status ? 100 + status : rc;
}

static std::vector<uint8_t> read_file(const std::string& path) {
    FILE* fp = fopen(path.c_str(), "rb");
    if (!fp) { printf("cannot open %s\n", path.c_str()); exit(1); }
    std::vector<uint8_t> v;
    uint8_t buf[65536];
    size_t n;
    while ((n = fread(buf, 1, sizeof(buf), fp)) > 0) v.insert(v.end(), buf, buf + n);
    fclose(fp);
    return v;
}

int main(int argc, char** argv) {
    if (argc < 3) { printf("usage: jpeg_decode_check DIR N\n"); return 2; }
    const std::string dir = argv[1];
    const int N = atoi(argv[2]);
    std::vector<std::string> names;
    {
        FILE* fp = fopen((dir + "/files.txt").c_str(), "r");
        if (!fp) { printf("no files.txt\n"); return 2; }
        char line[512];
        while (fgets(line, sizeof(line), fp)) {
            std::string s(line);
            while (!s.empty() && (s.back() == '\n' || s.back() == '\r')) s.pop_back();
            if (!s.empty()) names.push_back(s);
        }
        fclose(fp);
    }
    auto whole = [](int H, int W, int& y0, int& x0, int& h, int& w) { y0 = 0; x0 = 0; h = H; w = W; };
    auto random_rect = [](int H, int W, int& y0, int& x0, int& h, int& w) {
        y0 = rnd_below(H); x0 = rnd_below(W);
        h = 1 + rnd_below(H - y0); w = 1 + rnd_below(W - x0);
    };
    auto keep = [](int32_t*) {};
    Counts good, bad;
    for (const std::string& name : names) {
        const std::vector<uint8_t> file = read_file(dir + "/" + name);
        std::vector<int16_t> coef;
        const int rc = run(file, whole, keep, good, &coef);
        if (rc != NTK_OK) { printf("%s: expected a clean decode, got %d\n", name.c_str(), rc); return 1; }
        FILE* fp = fopen((dir + "/" + name + ".coef").c_str(), "wb");
        fwrite(coef.data(), sizeof(int16_t), coef.size(), fp);
        fclose(fp);
        // every rectangle of an untouched file decodes clean as well
        for (int i = 0; i < 8; ++i)
            if (run(file, random_rect, keep, good, nullptr) != NTK_OK) { printf("%s: a rectangle did not decode\n", name.c_str()); return 1; }
        // a header cut at every byte position
        const size_t head = file.size() < 700 ? file.size() : 700;
        for (size_t cut = 0; cut < head; ++cut) run(std::vector<uint8_t>(file.begin(), file.begin() + cut), whole, keep, bad, nullptr);
        // the scan's start: where the last FF DA segment ends
        size_t scan = 0;
        for (size_t i = 2; i + 3 < file.size(); ++i)
            if (file[i] == 0xFF && file[i + 1] == 0xDA) { scan = i + 2 + ((file[i + 2] << 8) | file[i + 3]); break; }
        for (int it = 0; it < N; ++it) {
            std::vector<uint8_t> f = file;
            int new_interval = -1;
            switch (rnd_below(5)) {
                case 0:                                            // bytes flipped in the headers
                    for (int k = 1 + rnd_below(4); k > 0; --k) f[rnd_below((int)scan)] ^= (uint8_t)(1 + rnd_below(255));
                    break;
                case 1:                                            // bytes flipped in the scan
                    for (int k = 1 + rnd_below(8); k > 0; --k) f[scan + rnd_below((int)(f.size() - scan))] ^= (uint8_t)(1 + rnd_below(255));
                    break;
                case 2:                                            // truncation
                    f.resize(rnd_below((int)f.size()));
                    break;
                case 3:                                            // a restart interval the data does not have
                    new_interval = rnd_below(3) == 0 ? 0 : 1 + rnd_below(40);
                    break;
                default:                                           // random bytes written over a random stretch
                    for (int k = rnd_below(32), at = rnd_below((int)f.size()); k > 0 && at < (int)f.size(); --k, ++at) f[at] = (uint8_t)rnd();
                    break;
            }
            auto tweak = [&](int32_t* hdr) { if (new_interval >= 0) hdr[NTK_JPEG_DESC_RESTART] = new_interval; };
            run(f, random_rect, tweak, bad, nullptr);
        }
    }
    printf("good files: %ld decodes; corrupted: %ld accepted (%ld decoded without a flag, %ld flagged), %ld to the host, %ld malformed\n",
           good.decoded_ok, bad.accepted, bad.decoded_ok, bad.flagged, bad.host, bad.malformed);
    if (bad.flagged == 0 || bad.malformed == 0) { printf("the corruptions reached neither the decoder's nor the parser's refusals\n"); return 1; }
    printf("jpeg decode check: ok\n");
    return 0;
}
