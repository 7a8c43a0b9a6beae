"""GPU: the fused stem (ntk_vgg_conv3x3_relu_split3_stem, csrc/conv_bf16p.hip STEM: conv1_1 computed inside conv1_2's staging) on
every frame shape its predicate accepts over a grid, and where conv1_1's values leave fp16's range.

tests/test_conv_shapes_cabi.py holds the entry to its predicate without a device; tests/test_vgg_stem_gpu.py runs five hand-picked
shapes, none with more than eight workgroups.  Here:
  * the GRID: H, W in STEM_SIDES on three frames, pooled or not, split or fp32 output.  The launcher cuts a frame into 32x8 sub-blocks
    where W % 32 == 0, else 16x16 where both sides are multiples of 16, else four 8x8 sub-blocks per workgroup; the grid holds 16 / 8 /
    40 maps of the three forms, every residue of the ragged last group of four and, per form, maps of more than eight workgroups (the
    second grid slot of conv_tile_wg) -- asserted before anything runs.  Every case: against a float64 convolution of both layers
    (SPLIT_LAYER_BOUND), against the separate pair conv3x3_relu -> conv3x3_relu_split3(fp32 in) (bit for bit where W % 32 == 0: the
    row kernel sums in the same order; elsewhere within d2, the bound tests/test_vgg_stem_gpu.py derives from the inputs), the split
    map against to_split() of the fp32 map, a guard buffer round the output, and the first frame of three against a call on one frame;
  * the same on a SHIFTED conv1_1 bias (+0.5): conv1_1 evaluated outside the frame would then give relu(b1) > 0 where conv1_2's zero
    padding belongs, at every border pixel;
  * RANGE: conv1_1 scaled until its values pass 65504 (fp16's largest: the high part saturates, the low part carries the rest) and
    131008 (the clamp of stem_put), and scaled down below 6e-5 (fp16's subnormals); one NaN or infinite frame pixel must stay inside
    its 5 x 5 window of output pixels.
Every bound but SPLIT_LAYER_BOUND is computed in float64 from the inputs."""
import functools

import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O
from oracle import ntm_oracle_torch as OT
from test_conv_shapes_gpu import _Checks
from test_vgg_stem_gpu import SPLIT_LAYER_BOUND, _guarded

pytestmark = pytest.mark.gpu

F = 3
STEM_SIDES = (8, 16, 24, 32, 40, 48, 56, 64)          # 48 and 64: more than one sub-block per row in every form
GRID = [(H, W) for H in STEM_SIDES for W in STEM_SIDES]
# the shifted-bias sweep: every map of the 32x8 and 16x16 forms and these of 8x8x4 (residues 3 F bx by % 4 = 3, 2, 1, 0, 3, 1, 1, 0)
SHIFTED_8X8X4 = ((8, 8), (8, 16), (8, 24), (32, 8), (24, 24), (40, 56), (56, 40), (32, 24))
FP16_MAX, S3_MAX = 65504.0, 131008.0                  # csrc/conv_bf16p.hip: the high part saturates at FP16_MAX, stem_put clamps at S3_MAX


def _form(H, W):
    """bf16p_launch's rule for four-wave workgroups: (name, TW, TH, sub-blocks per workgroup)"""
    if W % 32 == 0:
        return "32x8", 32, 8, 1
    if H % 16 == 0 and W % 16 == 0:
        return "16x16", 16, 16, 1
    return "8x8x4", 8, 8, 4


def _workgroups(frames, H, W):
    _name, tw, th, nsub = _form(H, W)
    return -(-(frames * (W // tw) * (H // th)) // nsub)


def _assert_selection():
    """the grid selects what it is meant to select"""
    from ntmtrack import vgg
    assert sum(vgg.split3_stem_supported(H, W, pool) for H, W in GRID for pool in (False, True)) == 128
    forms = {}
    for H, W in GRID:
        forms.setdefault(_form(H, W)[0], []).append((H, W))
    counts = {k: len(v) for k, v in forms.items()}
    residues = sorted({F * (H // 8) * (W // 8) % 4 for H, W in forms["8x8x4"]})
    most = {k: max(_workgroups(F, H, W) for H, W in v) for k, v in forms.items()}
    print("stem grid: maps per form %s; 8x8x4 last-group residues %s; most workgroups per form %s" % (counts, residues, most))
    assert counts == {"32x8": 16, "16x16": 8, "8x8x4": 40}, counts
    assert residues == [0, 1, 2, 3], residues
    assert all(n > 8 for n in most.values()), most                             # the second grid slot (sp = slot * 8 + xcd) runs
    shifted = [m for m in GRID if _form(*m)[0] != "8x8x4"] + list(SHIFTED_8X8X4)
    assert len(shifted) == 32 and all(_form(*m)[0] == "8x8x4" for m in SHIFTED_8X8X4)
    assert sorted({F * (H // 8) * (W // 8) % 4 for H, W in SHIFTED_8X8X4}) == [0, 1, 2, 3]
    return shifted


def _conv_abs(x, w):
    """sum over taps and channels of |x| |w| (float64, SAME): what rounding errors of a convolution scale with"""
    return OT.conv3x3_same_relu(np.abs(x), np.abs(w), np.zeros(w.shape[3]))


@functools.lru_cache(maxsize=None)
def _weights(bias1):
    """one weight set for a whole sweep (tests/test_vgg_stem_gpu.py _case: He-scaled, nonzero biases); bias1 shifts conv1_1's bias"""
    rng = np.random.default_rng(20)
    w1 = (rng.standard_normal((3, 3, 3, 64)) * np.sqrt(2.0 / 27)).astype(np.float32)
    w2 = (rng.standard_normal((3, 3, 64, 64)) * np.sqrt(2.0 / (9 * 64))).astype(np.float32)
    b1 = (rng.standard_normal(64) * 0.1 + bias1).astype(np.float32)
    b2 = (rng.standard_normal(64) * 0.1).astype(np.float32)
    return w1, b1, w2, b2


def _frames(frames, H, W):
    rng = np.random.default_rng([frames, H, W])
    return rng.uniform(0, 255, size=(frames, H, W, 3)).astype(np.float32) - O.VGG_MEAN


def _map(H, W, bias1):
    """frames, the float64 reference of both layers (un-pooled, pooled) and d2, the bound on |fused - separate| where the separate
    conv1_1 sums in another order (the derivation of tests/test_vgg_stem_gpu.py _case)"""
    w1, b1, w2, b2 = _weights(bias1)
    x = _frames(F, H, W)
    y1 = OT.conv3x3_same_relu(x, w1, b1)
    y2 = OT.conv3x3_same_relu(y1, w2, b2)
    d1 = 2 * 28 * 2.0 ** -24 * (_conv_abs(x, w1) + np.abs(b1.astype(np.float64))) + 2 * 2.0 ** -22 * np.abs(y1)
    return x, {False: y2, True: O.maxpool2x2(y2)}, float(_conv_abs(d1, w2).max())


class _StemChecks(_Checks):
    def within(self, what, shape, value, bound):
        """value <= bound; the worst value / bound is kept"""
        self.n += 1
        self.worst[what] = max(self.worst.get(what, 0.0), value / bound)
        if not value <= bound:
            self.bad.append("%s %s: %.3e, bound %.3e" % (what, shape, value, bound))


def _sweep(cuda, maps, bias1, name):
    from ntmtrack import _lib, vgg
    w1, b1, w2, b2 = _weights(bias1)
    t = lambda a: torch.from_numpy(a).to(cuda)
    w1p, b1t, w2t, b2t = vgg.pack_weights(t(w1)), t(b1), t(w2), t(b2)
    stem = (w1p, b1t)
    c = _StemChecks()
    for H, W in maps:
        form = _form(H, W)[0]
        x64, refs, d2 = _map(H, W, bias1)
        x = t(x64)
        for pool in (False, True):
            shape = "F=%d H=%d W=%d pool=%d" % (F, H, W, pool)
            ref = refs[pool]
            oh, ow = (H // 2, W // 2) if pool else (H, W)
            try:
                if not pool:
                    w2p = vgg.pack_weights_split3(w2t, H, W)
                    y1 = vgg.conv3x3_relu(x, w1p, b1t, 3, 64)
                y32 = None
                for out_f32 in (True, False):
                    dst = "nhwc" if out_f32 else "split"
                    out, guard = _guarded(vgg._map_shape(dst, F, oh, ow, 64), vgg._MAP_DTYPE[dst], cuda)
                    got = vgg.conv3x3_relu_split3(x, w2p, b2t, 64, 64, fuse_pool=pool, out_f32=out_f32, out=out, stem=stem)
                    torch.cuda.synchronize()
                    c.n += 1
                    try:
                        guard()
                    except AssertionError as e:
                        c.bad.append("%s %s f32=%d: %s" % (form, shape, out_f32, e))
                    sep = vgg.conv3x3_relu_split3(y1, w2p, b2t, 64, 64, fuse_pool=pool, out_f32=out_f32)
                    g32, s32 = (got, sep) if out_f32 else (vgg.from_split(got), vgg.from_split(sep))
                    c.close(form + " vs float64", shape + " f32=%d" % out_f32, g32, ref, SPLIT_LAYER_BOUND)
                    if W % 32 == 0:                   # conv1_1's k order and fp32 matrix arithmetic are the row kernel's: the same bits
                        c.same(form + " vs the separate pair", shape + " f32=%d" % out_f32, got, sep)
                    c.within(form + " |fused - separate| of d2", shape + " f32=%d" % out_f32,
                             float((g32.double() - s32.double()).abs().max()), d2)
                    if out_f32:
                        y32 = got
                    else:
                        c.same(form + " split map vs to_split(its fp32 map)", shape, got, vgg.to_split(y32))
                if not pool:                          # groups of sub-blocks that span frames must not leak
                    one = vgg.conv3x3_relu_split3(x[:1].contiguous(), w2p, b2t, 64, 64, out_f32=True, stem=stem)
                    c.same(form + " frame 0 of %d vs a call on one frame" % F, shape, y32[:1], one)
            except _lib.NtkError as e:               # a shape the predicate accepts that an entry refuses
                c.bad.append("%s %s: %s" % (form, shape, e))
    c.verdict(name)


def test_every_accepted_stem_geometry_matches_float64_and_the_separate_pair(cuda):
    _assert_selection()
    _sweep(cuda, GRID, 0.0, "fused stem, geometry grid")


def test_stem_borders_with_a_shifted_conv1_1_bias(cuda):
    """b1 + 0.5: relu(b1) > 0 in nearly every channel, so a patch pixel outside the frame that held conv1_1 of the zero padding
    instead of zero would show in every output pixel on the frame's border"""
    shifted = _assert_selection()
    assert float(np.mean(_weights(0.5)[1] > 0.1)) > 0.9
    _sweep(cuda, shifted, 0.5, "fused stem, conv1_1 bias + 0.5")


# ---- where conv1_1's values leave fp16's range
RANGE_SHAPES = ((2, 16, 32), (1, 16, 16), (3, 8, 8))   # one map per sub-block form
# relu(conv1_1) of these inputs peaks at 480 and half of it is ReLU zeros: x 1024, 23 % / 15 % / 9 % of its elements lie in
# (0, 65504] / (65504, 131008] / above (x 512: under 1 % above); x 2^-23, its largest is 5.7e-5
SATURATION_FACTOR = 1024.0
FLOOR_FACTOR = 2.0 ** -23


def _rtz_fp16(v):
    """float64 v >= 0 -> fp16 rounded toward zero, saturating at 65504 (v_cvt_pkrtz_f16_f32), as float64"""
    t = np.minimum(v, FP16_MAX)
    h = t.astype(np.float16)
    bits = h.view(np.uint16) - (h.astype(np.float64) > t).astype(np.uint16)    # one ulp toward zero where nearest rounded up
    return bits.view(np.float16).astype(np.float64)


def _w2_low_part(w2):
    """the low part of conv1_2's weights as packed (split3_scale_kernel, split3_pack_kernel): scaled by the power of two that puts
    the largest |w| in [2^13, 2^14), high part = fp16 to nearest, low = the rest -- here unscaled again, float64"""
    _f, e = np.frexp(float(np.max(np.abs(w2))))
    k = 14 - int(e)
    ws = w2.astype(np.float64) * 2.0 ** k
    assert 2.0 ** 13 <= np.max(np.abs(ws)) < 2.0 ** 14
    return (ws - ws.astype(np.float16).astype(np.float64)) * 2.0 ** -k


@functools.lru_cache(maxsize=None)
def _range_case(frames, H, W, factor):
    """conv1_1 scaled by `factor`: inputs, float64 relu(conv1_1), the oracle (conv1_2 of min(relu(conv1_1), 131008)) and the bound
    on |fused - oracle| per output pixel, un-pooled and pooled, all from the inputs:
      sum |w2| d1, d1 = 2 gamma_28 (sum |x w1| + |b1|) for conv1_1's fp32 summation + the split error of y1c = hi + lo -- above
          65504 hi IS 65504 and lo = fp16(y1c - 65504): half fp16's spacing there; below, 2^-22 |y1c|; below fp16's normal range
          (6.1e-5) hi and lo are multiples of 2^-24: 2^-25;
      + sum |lo(y1c)| |wl(w2)|: the product of the two low parts, which the kernel drops (lo(v) = v - rtz_fp16(v));
      + SPLIT_LAYER_BOUND max |ref|: conv1_2 itself."""
    w1, b1, w2, b2 = _weights(0.0)
    w1, b1 = w1 * np.float32(factor), b1 * np.float32(factor)
    x = _frames(frames, H, W)
    y1 = OT.conv3x3_same_relu(x, w1, b1)
    y1c = np.minimum(y1, S3_MAX)
    y2 = OT.conv3x3_same_relu(y1c, w2, b2)
    over = y1c > FP16_MAX
    rest = np.where(over, y1c - FP16_MAX, 1.0)
    half_spacing = 2.0 ** (np.maximum(np.floor(np.log2(rest)), -14) - 11)
    split = np.where(over, half_spacing, np.where(y1c < 2.0 ** -14, 2.0 ** -25, 2.0 ** -22 * y1c))
    split = np.where(y1c == 0, 0.0, split)
    d1 = 2 * 28 * 2.0 ** -24 * (_conv_abs(x, w1) + np.abs(b1.astype(np.float64))) + split
    bound = _conv_abs(d1, w2) + _conv_abs(y1c - _rtz_fp16(y1c), _w2_low_part(w2)) + SPLIT_LAYER_BOUND * np.max(np.abs(y2))
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, y1=y1, ref={False: y2, True: O.maxpool2x2(y2)},
                bound={False: bound, True: O.maxpool2x2(bound)})


def _run_range(cuda, case, frames, H, W, pool, what):
    """the fused stem on a range case: finite, within the case's bound of the oracle, and on (2, 16, 32) the separate pair's bits
    (the separate conv1_1 writes the un-clamped fp32 value; f32_put clamps it to the same 131008)"""
    from ntmtrack import vgg
    t = lambda a: torch.from_numpy(a).to(cuda)
    x, w1p, b1, b2 = t(case["x"]), vgg.pack_weights(t(case["w1"])), t(case["b1"]), t(case["b2"])
    w2p = vgg.pack_weights_split3(t(case["w2"]), H, W)
    got = vgg.conv3x3_relu_split3(x, w2p, b2, 64, 64, fuse_pool=pool, out_f32=True, stem=(w1p, b1))
    g = got.cpu().numpy().astype(np.float64)
    ref, bound = case["ref"][pool], case["bound"][pool]
    assert g.shape == ref.shape and np.isfinite(g).all()
    err = np.abs(g - ref)
    print("stem %s %s pool=%d: |fused - float64| %.3e of max |y| = %.3e, at most %.3f of its bound (the bound: up to %.3e of max |y|)"
          % (what, (frames, H, W), pool, err.max() / np.abs(ref).max(), np.abs(ref).max(), (err / bound).max(),
             bound.max() / np.abs(ref).max()))
    assert (err <= bound).all(), (float((err / bound).max()), int((err > bound).sum()))
    if (frames, H, W) == (2, 16, 32):
        sep = vgg.conv3x3_relu_split3(vgg.conv3x3_relu(x, w1p, b1, 3, 64), w2p, b2, 64, 64, fuse_pool=pool, out_f32=True)
        assert torch.equal(got, sep)


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("frames,H,W", RANGE_SHAPES)
def test_stem_where_conv1_1_saturates_fp16(cuda, frames, H, W, pool):
    case = _range_case(frames, H, W, SATURATION_FACTOR)
    y1 = case["y1"]
    bands = [float(np.mean((y1 > lo) & (y1 <= hi))) for lo, hi in ((0.0, FP16_MAX), (FP16_MAX, S3_MAX), (S3_MAX, np.inf))]
    print("relu(conv1_1) x %g on %s: %.1f %% in (0, 65504], %.1f %% in (65504, 131008], %.1f %% above"
          % ((SATURATION_FACTOR, (frames, H, W)) + tuple(100 * b for b in bands)))
    assert min(bands) >= 0.01, bands
    _run_range(cuda, case, frames, H, W, pool, "saturating")


@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("frames,H,W", RANGE_SHAPES)
def test_stem_where_conv1_1_is_below_the_fp16_floor(cuda, frames, H, W, pool):
    case = _range_case(frames, H, W, FLOOR_FACTOR)
    y1 = case["y1"]
    assert 0 < y1.max() < 6e-5 and float(np.mean(y1 > 2.0 ** -24)) > 0.25, (y1.max(), float(np.mean(y1 > 2.0 ** -24)))
    _run_range(cuda, case, frames, H, W, pool, "below 6e-5")


@pytest.mark.parametrize("frames,H,W", [(1, 16, 32), (1, 16, 16), (2, 8, 8)])
def test_stem_contains_one_bad_frame_pixel(cuda, frames, H, W):
    """one NaN or infinite frame pixel (all three channels): conv1_1 spreads it by one pixel, conv1_2 by one more -- every output
    pixel more than 2 rows or 2 columns away, and every other frame, has the clean run's bits (inside the window: not asserted)"""
    from ntmtrack import vgg
    w1, b1, w2, b2 = _weights(0.0)
    t = lambda a: torch.from_numpy(a).to(cuda)
    w1p, b1t, b2t, w2p = vgg.pack_weights(t(w1)), t(b1), t(b2), vgg.pack_weights_split3(t(w2), H, W)
    run = lambda x: vgg.conv3x3_relu_split3(x, w2p, b2t, 64, 64, out_f32=True, stem=(w1p, b1t))
    x = t(_frames(frames, H, W))
    clean = run(x)
    assert bool(torch.isfinite(clean).all())
    ys, xs = torch.arange(H, device=cuda)[:, None], torch.arange(W, device=cuda)[None, :]
    for f, y0, x0 in ((0, H // 2, W // 2 - 1), (frames - 1, H - 1, W - 1), (0, 0, 0)):     # interior; frame corners
        far = ((ys - y0).abs() > 2) | ((xs - x0).abs() > 2)
        assert int(far.sum()) > 0
        for bad in (float("nan"), float("inf")):
            xb = x.clone()
            xb[f, y0, x0, :] = bad
            got = run(xb)
            assert torch.equal(got[f][far], clean[f][far]), (f, y0, x0, bad)
            others = [g for g in range(frames) if g != f]
            assert torch.equal(got[others], clean[others]), (f, y0, x0, bad)
