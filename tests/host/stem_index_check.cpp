// Host check of csrc/conv_stem.h, the fused stem's index arithmetic: build with -fsanitize=address,undefined and run (exit 0 = pass).
// For every sub-block shape of the four-wave split form and sub-blocks at every kind of frame position, the frame patch is filled
// through stem_fp_elem / stem_fp_src into a buffer of exactly stem_fp_floats() floats (an index past it is a sanitizer report), and
// every operand k = tap * 3 + c of every patch pixel is read back through stem_pixel / stem_fp_corner / stem_fp_k and compared with
// the zero-padded frame; stem_inside must be the frame test of that pixel.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "conv_stem.h"

static int fails = 0;
#define CHECK(c, ...) do { if (!(c)) { if (++fails < 20) { std::printf("FAIL %s:%d: ", __FILE__, __LINE__); std::printf(__VA_ARGS__); std::printf("\n"); } } } while (0)

static float frame_at(const std::vector<float>& fr, int H, int W, int y, int x, int c) {
    return (y >= 0 && y < H && x >= 0 && x < W) ? fr[((size_t)y * W + x) * 3 + c] : 0.f;
}

static void run(int tw, int th, int nsub, int H, int W) {
    std::vector<float> fr((size_t)H * W * 3);
    for (size_t i = 0; i < fr.size(); ++i) fr[i] = 1.f + (float)i;             // no zero inside the frame
    // the workgroup's sub-blocks: walk the frame's sub-blocks in groups of nsub (the last group may be ragged: those stay at the origin)
    const int bxN = W / tw, byN = H / th, NQ = bxN * byN;
    for (int g = 0; g * nsub < NQ; ++g) {
        std::vector<int> sby(nsub, 0), sbx(nsub, 0);
        for (int i = 0; i < nsub && g * nsub + i < NQ; ++i) { sby[i] = th * ((g * nsub + i) / bxN); sbx[i] = tw * ((g * nsub + i) % bxN); }
        const int n = stem_fp_floats(tw, th, nsub);
        std::vector<float> fp((size_t)n, -1.f);
        for (int e = 0; e < n; ++e) {
            int q, fy, fx, c, y, x;
            stem_fp_elem(e, tw, th, q, fy, fx, c);
            CHECK(q >= 0 && q < nsub && fy >= 0 && fy < th + 4 && fx >= 0 && fx < tw + 4 && c >= 0 && c < 3, "elem %d", e);
            const bool in = stem_fp_src(fy, fx, sby[q], sbx[q], H, W, y, x);
            CHECK(in == (y >= 0 && y < H && x >= 0 && x < W), "src %d", e);
            fp[e] = in ? fr[((size_t)y * W + x) * 3 + c] : 0.f;
        }
        const int pw = tw + 2, ph = th + 2, npx = stem_patch_pixels(tw, th, nsub);
        CHECK(npx == nsub * ph * pw, "patch pixels");
        for (int lp = 0; lp < npx; ++lp) {
            int q, py, px;
            stem_pixel(lp, tw, th, q, py, px);
            CHECK(q >= 0 && q < nsub && py >= 0 && py < ph && px >= 0 && px < pw && lp == (q * ph + py) * pw + px, "pixel %d", lp);
            const int corner = stem_fp_corner(q, py, px, tw, th);
            const int Y = sby[q] - 1 + py, X = sbx[q] - 1 + px;                 // the patch pixel's frame coordinates
            CHECK(stem_inside(py, px, sby[q], sbx[q], H, W) == (Y >= 0 && Y < H && X >= 0 && X < W), "inside %d", lp);
            for (int k = 0; k < 27; ++k) {
                const int tap = k / 3, c = k % 3, dy = tap / 3, dx = tap % 3;
                const int o = corner + stem_fp_k(k, tw);
                CHECK(o >= 0 && o < n, "operand offset %d of %d", o, n);
                const float want = frame_at(fr, H, W, Y + dy - 1, X + dx - 1, c);
                CHECK(fp.at((size_t)o) == want, "operand %d of pixel %d: %g != %g", k, lp, fp.at((size_t)o), want);
            }
        }
    }
}

int main() {
    const int shapes[3][3] = {{32, 8, 1}, {16, 16, 1}, {8, 8, 4}};
    for (const auto& s : shapes)
        for (int hm = 1; hm <= 3; ++hm)
            for (int wm = 1; wm <= 3; ++wm) run(s[0], s[1], s[2], s[1] * hm, s[0] * wm);
    run(8, 8, 4, 8, 8);                                                          // a single sub-block in a group of four
    if (fails) { std::printf("%d checks failed\n", fails); return 1; }
    std::printf("stem index check: ok\n");
    return 0;
}
