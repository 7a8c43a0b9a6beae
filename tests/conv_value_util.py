"""CPU, float64: what the value tests of the trunk's conv forms (tests/test_conv_values_host.py, tests/test_conv_values_gpu.py) share.

  * the MAGNITUDE map A = sum |x| |w| + |b| that every rounding error of a convolution scales with;
  * the PARTS of the split form (csrc/conv_bf16p.hip X3) as the kernels make them -- an activation's high part rounded toward zero
    and saturating at 65504, its low part to nearest; a layer's weights scaled by one power of two (largest in [2^13, 2^14)), high
    part to nearest, low part the rest -- their errors dx, dw and the pointwise bound D of one split layer derived from them;
  * a MODEL of the kernel's arithmetic (xh wh + xh wl + xl wh, sums in float64: no accumulation error) and two MUTANTS of it that
    flush fp16 subnormal parts to zero, one for the weights, one for the activations: what a matrix pipe without fp16 subnormals,
    or a packing that drops them, would compute;
  * the value REGIMES R0 .. R5 built from the suite's operands with powers of two (exact in fp32);
  * the fp32 numpy restatement of the Winograd kernels' arithmetic (F(2x2,3x3), F(4x4,3x3)); scripts/dev_wino43_numerics.py imports it.
Activations are >= 0 everywhere here (post-ReLU maps, as the trunk's)."""
import functools

import numpy as np
import torch

FP16_MAX, S3_MAX = 65504.0, 131008.0       # the high part saturates at FP16_MAX; a split value (hi + lo) at S3_MAX
FP16_MIN_NORMAL = 2.0 ** -14


# ---- convolutions
def conv_pre(x, w, b=None, dtype=np.float64):
    """conv3x3 SAME + bias WITHOUT the ReLU on torch-CPU in `dtype`: x [F,H,W,Cin], w [3,3,Cin,Cout], b [Cout] -> [F,H,W,Cout]"""
    td = torch.float64 if dtype == np.float64 else torch.float32
    xt = torch.as_tensor(np.ascontiguousarray(x, dtype=dtype)).permute(0, 3, 1, 2)
    wt = torch.as_tensor(np.ascontiguousarray(w, dtype=dtype)).permute(3, 2, 0, 1)
    bt = None if b is None else torch.as_tensor(np.ascontiguousarray(b, dtype=dtype))
    with torch.no_grad():
        y = torch.nn.functional.conv2d(xt.to(td), wt.to(td), bt, padding=1)
    return y.permute(0, 2, 3, 1).contiguous().numpy()


def conv_abs(x, w):
    """sum over taps and channels of |x| |w| (float64, SAME)"""
    return conv_pre(np.abs(np.asarray(x, np.float64)), np.abs(np.asarray(w, np.float64)))


def magnitude(x, w, b):
    """A = conv_abs(|x|, |w|) + |b|"""
    return conv_abs(x, w) + np.abs(np.asarray(b, np.float64))


def maxpool2x2(y):
    F, H, W, C = y.shape
    return y.reshape(F, H // 2, 2, W // 2, 2, C).max(axis=(2, 4))


def bf16_round(x):
    """fp32 -> bf16 (to nearest even), as fp32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return ((u + ((u >> 16) & 1) + np.uint32(0x7FFF)) & np.uint32(0xFFFF0000)).view(np.float32)


def accumulation_unit(x, w, b, ref_pre, A):
    """c_ref = max |conv_fp32_cpu - ref64| / A: what one fp32 summation of these operands costs, from the reference side only"""
    return float(np.max(np.abs(conv_pre(x, w, b, dtype=np.float32).astype(np.float64) - ref_pre) / A))


# ---- the split form's parts
def rtz_fp16(v):
    """float64 v >= 0 -> fp16 rounded toward zero, saturating at 65504 (v_cvt_pkrtz_f16_f32), as float64"""
    v = np.asarray(v, np.float64)
    assert (v >= 0).all()
    t = np.minimum(v, FP16_MAX)
    h = t.astype(np.float16)
    bits = h.view(np.uint16) - (h.astype(np.float64) > t).astype(np.uint16)    # one ulp toward zero where nearest rounded up
    return bits.view(np.float16).astype(np.float64)


def _flush(p):
    """fp16 subnormals -> 0"""
    return np.where(np.abs(p) < FP16_MIN_NORMAL, 0.0, p)


def x_parts(x, flush=False):
    """(xh, xl) of activations x >= 0 as s3_split4 makes them after the clamp at 131008: xh = rtz_fp16, xl = fp16(x - xh) to nearest"""
    xc = np.minimum(np.asarray(x, np.float64), S3_MAX)
    xh = rtz_fp16(xc)
    xl = (xc - xh).astype(np.float16).astype(np.float64)
    return (_flush(xh), _flush(xl)) if flush else (xh, xl)


def w_scale(w):
    """the power of two split3_scale_kernel multiplies a layer's weights by: the largest |w| lands in [2^13, 2^14)"""
    m = float(np.max(np.abs(w)))
    _f, e = np.frexp(m)
    scale = 2.0 ** (14 - int(e))
    assert 2.0 ** 13 <= m * scale < 2.0 ** 14
    return scale


def w_parts(w, flush=False):
    """(wh, wl, scale): the SCALED parts split3_pack_kernel stores: wh = fp16(w scale) to nearest, wl = fp16(w scale - wh)"""
    scale = w_scale(w)
    ws = np.asarray(w, np.float64) * scale
    wh = ws.astype(np.float16).astype(np.float64)
    wl = (ws - wh).astype(np.float16).astype(np.float64)
    return (_flush(wh), _flush(wl), scale) if flush else (wh, wl, scale)


def dx(v):
    """bound on |v - (xh + xl)| for v in [0, 131008]: 0 at 0; up to 65504 eleven + eleven bits, 2^-22 v, but never below half the
    spacing of fp16's subnormals, 2^-25 (the low part of v < 2^-3 is one); above 65504 the high part IS 65504 and the low part
    carries v - 65504 at fp16's spacing there"""
    v = np.asarray(v, np.float64)
    rest = np.where(v > FP16_MAX, v - FP16_MAX, 1.0)
    half_spacing = 2.0 ** (np.maximum(np.floor(np.log2(rest)), -14) - 11)
    d = np.where(v > FP16_MAX, half_spacing, np.maximum(2.0 ** -22 * v, 2.0 ** -25))
    return np.where(v == 0, 0.0, d)


def dw(w):
    """bound on |w - (wh + wl) / scale|: max(2^-22 |w scale|, 2^-25) / scale"""
    scale = w_scale(w)
    return np.maximum(2.0 ** -22 * np.abs(np.asarray(w, np.float64)) * scale, 2.0 ** -25) / scale


def split_bound(x, w):
    """D: the pointwise bound on |model - float64| of one split layer, before the ReLU (which is 1-Lipschitz): the two part errors
    and the product of the two low parts, which the kernel drops.  x: the activations as the reference reads them (<= 131008)."""
    x = np.asarray(x, np.float64)
    assert (x <= S3_MAX).all()
    _xh, xl = x_parts(x)
    _wh, wl, scale = w_parts(w)
    return conv_abs(dx(x), w) + conv_abs(x, dw(w)) + conv_abs(xl, wl / scale)


def split_model(x, w, b, flush_w=False, flush_x=False):
    """the kernel's arithmetic without its accumulation error: (xh wh + xh wl + xl wh) / scale + b in float64, before the ReLU.
    flush_w / flush_x: the mutants -- fp16 subnormal weight / activation parts are zero."""
    xh, xl = x_parts(x, flush_x)
    wh, wl, scale = w_parts(w, flush_w)
    return (conv_pre(xh, wh) + conv_pre(xh, wl) + conv_pre(xl, wh)) / scale + np.asarray(b, np.float64)


# ---- the shapes: one per instantiation of the split form -- the thirteen rows of tests/test_vgg_gpu.py
# test_conv3x3_relu_split_form_matches_float64_oracle (one per sub-block form, input kind and output kind) with channel counts above
# 128 cut to 128: 128 columns keep the 128-column block, 128 input channels keep eight chunks and the eight-wave form.
# (F, H, W, cin, cout, pool, in_f32, out_f32)
SPLIT_SHAPES = (
    (2, 16, 32, 64, 64, True, True, False),       # four waves, 32x8 sub-blocks, fp32 input split by the staging, pool
    (2, 16, 32, 64, 64, False, False, False),     # ... from a split map, un-pooled
    (3, 16, 16, 64, 64, True, True, True),        # four waves, 16x16, fp32 in and out
    (5, 8, 8, 32, 64, False, True, False),        # four waves, 8x8 x 4, ragged last block, two chunks
    (1, 32, 64, 64, 128, False, False, False),    # eight waves, 32x16, 128 columns
    (3, 16, 16, 128, 128, True, False, False),    # 16x16 x 2: a block spans two frames
    (5, 8, 8, 128, 256, False, False, False),     # 8x8 x 8, ragged last block, two column blocks
    (2, 24, 8, 128, 128, True, False, True),      # 8x8 with the pool, fp32 output
    (3, 28, 28, 128, 128, False, False, False),   # 28 wide: runs of 512 pixels, two of them across a frame boundary
    (2, 28, 28, 128, 128, False, False, True),    # ... fp32 output
    (5, 20, 28, 16, 64, False, False, False),     # 28 wide, 20 rows, one chunk, 64 columns on eight waves
    (2, 24, 28, 128, 128, False, False, False),   # 28 wide, a multiple of 8 rows
    (2, 32, 28, 128, 128, False, False, True),    # ... 32 rows, fp32 output
)
# the other forms: each on those of these that its predicate accepts, pooled and un-pooled
OTHER_SHAPES = ((3, 8, 8, 32, 64), (3, 20, 28, 64, 64))

# ---- the value regimes
REGIMES =("R0", "R1", "R2", "R3", "R4", "R5")
R1_BITS, R2_BITS = 16, 12
SATURATION_FACTOR = 2.0 ** 15              # relu(N(0,1)) 3 x 2^15: N = 0.67 is 65504, N = 1.33 is 131008
FLOOR_FACTOR = 2.0 ** -12                  # the suite's activations stay below 16: all of them then below 2^-3


def base_operands(F, H, W, cin, cout, seed=23):
    """R0, the suite's operands: relu(N(0,1)) 3 activations, He-scaled weights, biases N(0, 0.1) -- with the output channel that
    holds the largest |w| moved to channel 0, so that a regime that leaves channel 0 alone leaves the layer's weight scale alone"""
    rng = np.random.default_rng([seed, F, H, W, cin, cout])
    x = (np.maximum(rng.standard_normal((F, H, W, cin)), 0) * 3).astype(np.float32)
    w = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
    b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
    n = int(np.argmax(np.abs(w).max(axis=(0, 1, 2))))
    w[..., [0, n]] = w[..., [n, 0]]
    b[[0, n]] = b[[n, 0]]
    return x, w, b


def _spread(count, period, bits):
    """exponents 0 .. bits over `count` channels: every run of `period` channels sees the whole spread, permuted; channel 0 gets 0"""
    p = (np.arange(count) % period) * 37 % period              # 37 is odd and no multiple of 3: a permutation of 0 .. period - 1
    return np.rint(bits * p / float(period - 1)).astype(np.int64)


def r1_exponents(cout):
    return _spread(cout, 64, R1_BITS)


def r2_exponents(cin):
    return _spread(cin, cin, R2_BITS)


def regime_operands(regime, x, w, b):
    """R0's operands (x, w, b) -> the regime's (x, w, b), float32, and what the reference reads as its input (x clamped at 131008)"""
    x, w, b = x.copy(), w.copy(), b.copy()
    if regime == "R1":                     # output-channel gains: weights and biases of channel n x 2^-k_n
        g = (2.0 ** -r1_exponents(w.shape[3])).astype(np.float32)
        w, b = w * g, b * g
    elif regime == "R2":                   # input-channel gains: x[..., c] 2^-k_c, w[:, :, c, :] 2^k_c: every product keeps its bits
        g = (2.0 ** -r2_exponents(w.shape[2])).astype(np.float32)
        x, w = x * g, w / g[:, None]
    elif regime == "R3":
        x = x * np.float32(SATURATION_FACTOR)
    elif regime == "R4":
        x = x * np.float32(FLOOR_FACTOR)
    elif regime == "R5":                   # channels 3 j dead, 3 j + 1 always alive, the rest as they were
        c = conv_pre(x, w)
        top = np.abs(c).max(axis=(0, 1, 2))
        shift = (2 * top + 1).astype(np.float32)
        n = np.arange(w.shape[3])
        b = np.where(n % 3 == 0, -shift, np.where(n % 3 == 1, shift, b)).astype(np.float32)
    else:
        assert regime in ("R0",), regime
    assert x.dtype == np.float32 and w.dtype == np.float32 and b.dtype == np.float32
    return x, w, b


class Case(object):
    """One (regime, layer shape): the operands, the float64 pre-activation of the reference (input clamped at 131008 as every entry
    to the split form clamps it), A, D, c_ref and the bound D + c_acc A, un-pooled.  c_acc = ACC_MARGIN c_ref: 4 covers a summation
    order other than the reference's and the split form's three partial products per term; it never sees a kernel's output."""
    ACC_MARGIN = 4.0

    def __init__(self, regime, F, H, W, cin, cout, split=True, bf16=False):
        """split: the reference reads min(x, 131008) and D is the split layer's; else D = 0.  bf16 (the bf16 forms): the activations
        are bf16 numbers and the reference multiplies them by bf16-rounded weights (self.w stays what the packing is given)."""
        self.regime, self.shape = regime, (F, H, W, cin, cout)
        self.x0, self.w0, self.b0 = base_operands(F, H, W, cin, cout)
        if bf16:
            self.x0 = bf16_round(self.x0)
        self.x, self.w, self.b = regime_operands(regime, self.x0, self.w0, self.b0)
        self.wref = bf16_round(self.w) if bf16 else self.w
        self.xref = np.minimum(self.x.astype(np.float64), S3_MAX) if split else self.x.astype(np.float64)
        self.pre = conv_pre(self.xref, self.wref, self.b)
        self.A = magnitude(self.xref, self.wref, self.b)
        self.c_ref = accumulation_unit(self.xref.astype(np.float32), self.wref, self.b, self.pre, self.A)
        self.c_acc = self.ACC_MARGIN * self.c_ref
        self.D = split_bound(self.xref, self.w) if split else np.zeros_like(self.A)
        self.bound = self.D + self.c_acc * self.A

    def ref(self, pool=False, clamp_out=False):
        y = np.maximum(self.pre, 0)
        if clamp_out:
            y = np.minimum(y, S3_MAX)
        return maxpool2x2(y) if pool else y

    def pooled(self, a, pool):
        return maxpool2x2(a) if pool else a


@functools.lru_cache(maxsize=None)
def case(regime, shape):
    """the split form's (regime, shape): computed once, shared by the host and the GPU tests, never changed"""
    return Case(regime, *shape)


def accepts(form, frames, H, W, cin, cout, pool):
    """does `form`'s own predicate take the layer?  (the bf16 tile and the direct kernel have none: their shape rules in
    include/ntmtrack.h)"""
    from ntmtrack import vgg, _lib
    if form == "split3":
        return vgg.split3_supported(H, W, cin, cout, pool)
    if form == "bf16p":
        return bool(_lib.lib().ntk_vgg_bf16p_supported(H, W, cin, cout, 1 if pool else 0))
    if form == "wino43":
        return vgg.wino43_supported(cin, cout, H, W, frames)
    if form == "wino":
        return vgg.wino_supported(cin, cout, H, W, frames)
    if not (H % 4 == 0 and W % 4 == 0 and cout % 64 == 0):
        return False
    return cin % 64 == 0 if form == "bf16" else (cin == 3 or cin % 32 == 0)


# ---- the Winograd kernels' arithmetic in fp32 numpy (weights transformed in float64 and stored fp32, fp32 input transform, fp32
# products accumulated over channels two at a time as the fp32 MFMA does, fp32 output transform)
BT4 = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]], np.float64)
G4 = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]], np.float64)
AT4 = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], np.float64)
BT2 = np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, 1, 0, -1]], np.float64)
G2 = np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]], np.float64)
AT2 = np.array([[1, 1, 1, 0], [0, 1, -1, -1]], np.float64)


def wino(x, w, BT, G, AT, m):
    """x [H,W,C] fp32 (H, W multiples of m), w [3,3,C,O] -> y [H,W,O] fp32; SAME padding."""
    H, W, C = x.shape
    O = w.shape[3]
    a = m + 2
    f32 = np.float32
    U = np.einsum("ik,klco,jl->ijco", G, w.astype(np.float64), G).astype(f32)      # weights transformed in float64, stored fp32
    xp = np.zeros((H + 2, W + 2, C), f32)
    xp[1:-1, 1:-1] = x
    y = np.zeros((H, W, O), f32)
    BTf, ATf = BT.astype(f32), AT.astype(f32)
    for ty in range(H // m):
        for tx in range(W // m):
            d = xp[ty * m:ty * m + a, tx * m:tx * m + a]                              # [a,a,C]
            t = np.einsum("ik,klc->ilc", BTf, d).astype(f32)
            V = np.einsum("ilc,jl->ijc", t, BTf).astype(f32)
            M = np.zeros((a, a, O), f32)
            for c0 in range(0, C, 2):                                                   # MFMA k = 2 accumulation order
                M = (M + np.einsum("ijc,ijco->ijo", V[:, :, c0:c0 + 2], U[:, :, c0:c0 + 2])).astype(f32)
            z = np.einsum("ik,klo->ilo", ATf, M).astype(f32)
            y[ty * m:(ty + 1) * m, tx * m:(tx + 1) * m] = np.einsum("ilo,jl->ijo", z, ATf).astype(f32)
    return y


def wino23(x, w):
    return wino(x, w, BT2, G2, AT2, 2)


def wino43(x, w):
    return wino(x, w, BT4, G4, AT4, 4)


def direct64(x, w):
    """x [H,W,C], w [3,3,C,O] -> the float64 convolution [H,W,O], SAME"""
    H, W, C = x.shape
    xp = np.zeros((H + 2, W + 2, C)); xp[1:-1, 1:-1] = x
    y = np.zeros((H, W, w.shape[3]))
    for ky in range(3):
        for kx in range(3):
            y += xp[ky:ky + H, kx:kx + W] @ w[ky, kx].astype(np.float64)
    return y
