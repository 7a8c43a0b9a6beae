// Index arithmetic of the fused stem (conv_bf16p.hip, template flag STEM): conv1_1 computed inside conv1_2's staging.  Host-callable,
// no device types: tests/host/stem_index_check.cpp runs every function here on the CPU under the address and undefined-behaviour
// sanitizers.
//
// Three pixel grids, all relative to a sub-block of th x tw output pixels whose first pixel is frame pixel (sby, sbx):
//   * conv1_2's PATCH, (th + 2) x (tw + 2): patch pixel (py, px) is frame pixel (sby - 1 + py, sbx - 1 + px).  A patch pixel outside
//     the frame is ZERO (conv1_2's SAME padding) -- not conv1_1 evaluated outside the frame: stem_inside;
//   * the FRAME PATCH, (th + 4) x (tw + 4) pixels of 3 floats: frame-patch pixel (fy, fx) is frame pixel (sby - 2 + fy, sbx - 2 + fx),
//     zero outside the frame (conv1_1's SAME padding): stem_fp_elem, stem_fp_src;
//   * conv1_1's tap (dy, dx), dy, dx in 0 .. 2, of patch pixel (py, px) reads frame-patch pixel (py + dy, px + dx).
// The patch pixels of a workgroup are numbered lp = (q (th + 2) + py)(tw + 2) + px over its sub-blocks q (stem_pixel); operand
// k = tap * 3 + c of pixel lp is float stem_fp_corner() + stem_fp_k() of the frame patches.
#pragma once

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NTK_STEM_HD __host__ __device__ __forceinline__
#else
#define NTK_STEM_HD static inline
#endif

NTK_STEM_HD int stem_fp_w(int tw) { return tw + 4; }
NTK_STEM_HD int stem_fp_h(int th) { return th + 4; }
// floats of the frame patches of a workgroup's nsub sub-blocks
NTK_STEM_HD int stem_fp_floats(int tw, int th, int nsub) { return nsub * stem_fp_h(th) * stem_fp_w(tw) * 3; }

// float e of the frame patches -> (sub-block q, frame-patch pixel (fy, fx), channel c)
NTK_STEM_HD void stem_fp_elem(int e, int tw, int th, int& q, int& fy, int& fx, int& c) {
    const int fpw = stem_fp_w(tw), fph = stem_fp_h(th);
    c = e % 3;
    const int p = e / 3;
    fx = p % fpw;
    const int r = p / fpw;
    fy = r % fph;
    q = r / fph;
}

// frame-patch pixel (fy, fx) of the sub-block at (sby, sbx) -> frame pixel (y, x); false: outside the H x W frame (the patch holds 0)
NTK_STEM_HD bool stem_fp_src(int fy, int fx, int sby, int sbx, int H, int W, int& y, int& x) {
    y = sby - 2 + fy;
    x = sbx - 2 + fx;
    return y >= 0 && y < H && x >= 0 && x < W;
}

// patch pixel lp (of nsub (th + 2)(tw + 2)) -> (sub-block q, patch row py, patch column px)
NTK_STEM_HD int stem_patch_pixels(int tw, int th, int nsub) { return nsub * (th + 2) * (tw + 2); }
NTK_STEM_HD void stem_pixel(int lp, int tw, int th, int& q, int& py, int& px) {
    const int pw = tw + 2, ph = th + 2;
    px = lp % pw;
    const int r = lp / pw;
    py = r % ph;
    q = r / ph;
}

// float offset, inside the frame patches, of the corner of the pixel's 3 x 3 window: frame-patch pixel (py, px) of sub-block q
NTK_STEM_HD int stem_fp_corner(int q, int py, int px, int tw, int th) {
    return ((q * stem_fp_h(th) + py) * stem_fp_w(tw) + px) * 3;
}
// ... and of conv1_1's operand k = tap * 3 + c (tap = 3 dy + dx, k < 27) relative to the corner
NTK_STEM_HD int stem_fp_k(int k, int tw) {
    const int tap = k / 3, c = k - tap * 3;
    return ((tap / 3) * stem_fp_w(tw) + tap % 3) * 3 + c;
}

// is patch pixel (py, px) of the sub-block at (sby, sbx) a pixel of the frame?  (else conv1_2 reads zero there)
NTK_STEM_HD bool stem_inside(int py, int px, int sby, int sbx, int H, int W) {
    const int y = sby - 1 + py, x = sbx - 1 + px;
    return y >= 0 && y < H && x >= 0 && x < W;
}
