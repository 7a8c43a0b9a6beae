"""GPU: the fused stem -- conv1_1 computed inside conv1_2's staging (ntk_vgg_conv3x3_relu_split3_stem, csrc/conv_bf16p.hip STEM) --
against (a) the separate pair conv3x3_relu -> conv3x3_relu_split3(fp32 in) on the same inputs and (b) a float64 convolution of both
layers; then the default (fused) trunk against the float64 oracle and the separate-stem trunk.

The fused kernel evaluates conv1_1 as a chain of v_mfma_f32_16x16x4_f32 over k = tap * 3 + c in order, from a zero accumulator, bias
added last.  On frames whose width is a multiple of 32 the separate conv1_1 is the row kernel (csrc/conv_direct.hip conv_c3_rows_kernel):
the same k order on v_mfma_f32_32x32x2_f32, whose steps round like the same sequence of fused multiply-adds -- there (a) is asserted
BIT FOR BIT.  On narrower frames the separate conv1_1 is the tile kernel, which sums in another order; what may differ then is
bounded here from the inputs, in float64, not from what the kernels give:
  * two fp32 summations of the same 27 products + bias differ by at most 2 gamma_28 (sum |x w| + |b|), gamma_n = n 2^-24;
  * the two values are then split into fp16 hi + lo, each to 2^-22 of its magnitude (csrc/conv_bf16p.hip s3_split4);
  * conv1_2 is linear before its ReLU, ReLU and max-pool are 1-Lipschitz: the difference reaches the output through sum |w2| d1.
"""
import functools

import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O

pytestmark = pytest.mark.gpu

SHAPES = [
    (1, 8, 32),       # one 32x8 sub-block, every border at once
    (2, 16, 32),      # a block boundary inside a frame and a frame boundary
    (1, 16, 16),      # the 16x16 form
    (3, 8, 8),        # 8x8x4 with a ragged last group and a group spanning frames
    (1, 32, 64),      # interior sub-blocks
]
SPLIT_LAYER_BOUND = 4e-6      # tests/test_vgg_gpu.py: a split-form layer against float64, of max |y|


def _conv_abs(x, w):
    """sum over taps and channels of |x| |w| (float64, SAME): what rounding errors of a convolution scale with"""
    return O.conv3x3_same_relu(np.abs(x), np.abs(w), np.zeros(w.shape[3]))


@functools.lru_cache(maxsize=None)
def _case(F, H, W, bias1):
    """inputs, the float64 reference of both layers (un-pooled and pooled) and the bound on |fused - separate|; computed once per shape"""
    rng = np.random.default_rng(1000 * H + 10 * W + F)
    x = (rng.uniform(0, 255, size=(F, H, W, 3)).astype(np.float32) - O.VGG_MEAN)
    w1 = (rng.standard_normal((3, 3, 3, 64)) * np.sqrt(2.0 / 27)).astype(np.float32)
    w2 = (rng.standard_normal((3, 3, 64, 64)) * np.sqrt(2.0 / (9 * 64))).astype(np.float32)
    b1 = (rng.standard_normal(64) * 0.1 + bias1).astype(np.float32)
    b2 = (rng.standard_normal(64) * 0.1).astype(np.float32)
    x64, w164, w264 = x.astype(np.float64), w1.astype(np.float64), w2.astype(np.float64)
    y1 = O.conv3x3_same_relu(x64, w164, b1.astype(np.float64))
    y2 = O.conv3x3_same_relu(y1, w264, b2.astype(np.float64))
    d1 = 2 * 28 * 2.0 ** -24 * (_conv_abs(x64, w164) + np.abs(b1)) + 2 * 2.0 ** -22 * np.abs(y1)
    d2 = _conv_abs(d1, w264)
    return dict(x=x, w1=w1, b1=b1, w2=w2, b2=b2, ref={False: y2, True: O.maxpool2x2(y2)}, d2=float(d2.max()))


def _device(case, cuda, H, W):
    from ntmtrack import vgg
    t = lambda a: torch.from_numpy(a).to(cuda)
    return dict(x=t(case["x"]), w1=vgg.pack_weights(t(case["w1"])), b1=t(case["b1"]),
                w2=vgg.pack_weights_split3(t(case["w2"]), H, W), b2=t(case["b2"]))


def _guarded(shape, dtype, cuda, fill=777.0, pad=2048):
    """an output map inside a larger buffer of guard values: (view, check) -- check() asserts nothing outside the view was written"""
    n = int(np.prod(shape))
    big = torch.full((n + 2 * pad,), fill, device=cuda, dtype=dtype)
    def check():
        assert bool((big[:pad] == fill).all()) and bool((big[pad + n:] == fill).all()), "wrote outside the batch"
    return big[pad:pad + n].view(shape), check


@pytest.mark.parametrize("out_f32", [False, True])
@pytest.mark.parametrize("pool", [False, True])
@pytest.mark.parametrize("F,H,W", SHAPES)
def test_fused_stem_matches_separate_pair_and_float64(cuda, F, H, W, pool, out_f32):
    from ntmtrack import vgg
    assert vgg.split3_stem_supported(H, W, pool)
    case = _case(F, H, W, 0.0)
    d = _device(case, cuda, H, W)
    ref = case["ref"][pool]
    scale = np.max(np.abs(ref))
    dst = "nhwc" if out_f32 else "split"
    oh, ow = (H // 2, W // 2) if pool else (H, W)
    out, check = _guarded(vgg._map_shape(dst, F, oh, ow, 64), vgg._MAP_DTYPE[dst], cuda)
    got = vgg.conv3x3_relu_split3(d["x"], d["w2"], d["b2"], 64, 64, fuse_pool=pool, out_f32=out_f32, out=out, stem=(d["w1"], d["b1"]))
    torch.cuda.synchronize()
    check()
    # (a) the separate pair
    y1 = vgg.conv3x3_relu(d["x"], d["w1"], d["b1"], 3, 64)
    sep = vgg.conv3x3_relu_split3(y1, d["w2"], d["b2"], 64, 64, fuse_pool=pool, out_f32=out_f32)
    as_f32 = lambda m: (m if out_f32 else vgg.from_split(m)).cpu().numpy().astype(np.float64)
    g, s = as_f32(got), as_f32(sep)
    assert g.shape == ref.shape
    err_fused, err_sep, diff = np.max(np.abs(g - ref)) / scale, np.max(np.abs(s - ref)) / scale, np.max(np.abs(g - s))
    print("stem %s pool=%d f32=%d: fused %.3e  separate %.3e  |fused - separate| %.3e (bound %.3e) of max |y| %.3e"
          % ((F, H, W), pool, out_f32, err_fused, err_sep, diff, case["d2"], scale))
    # (b) float64, with the bound of a split-form layer; and no worse than the separate form by more than conv1_1's rounding explains
    assert err_fused < SPLIT_LAYER_BOUND, err_fused
    assert diff <= case["d2"], (diff, case["d2"])
    if W % 32 == 0:                               # conv1_1's k order and fp32 matrix arithmetic are the row kernel's: the same bits
        assert torch.equal(got, sep)
    assert err_fused <= err_sep + case["d2"] / scale, (err_fused, err_sep)
    if not out_f32:                               # the split map is to_split() of the fp32 map of the same call; a second call gives the same bits
        y32 = vgg.conv3x3_relu_split3(d["x"], d["w2"], d["b2"], 64, 64, fuse_pool=pool, out_f32=True, stem=(d["w1"], d["b1"]))
        assert torch.equal(got, vgg.to_split(y32))
    again = vgg.conv3x3_relu_split3(d["x"], d["w2"], d["b2"], 64, 64, fuse_pool=pool, out_f32=out_f32, stem=(d["w1"], d["b1"]))
    assert torch.equal(got, again)


@pytest.mark.parametrize("F,H,W", [(2, 16, 32), (3, 8, 8)])
def test_fused_stem_where_conv1_1_is_all_relu_zeros(cuda, F, H, W):
    """a large negative conv1_1 bias: every patch is ReLU zeros, conv1_2 is relu(b2) everywhere -- in both forms, bit for bit"""
    from ntmtrack import vgg
    case = _case(F, H, W, -1.0e4)
    d = _device(case, cuda, H, W)
    assert float(np.max(O.conv3x3_same_relu(case["x"].astype(np.float64), case["w1"].astype(np.float64), case["b1"].astype(np.float64)))) == 0.0
    got = vgg.conv3x3_relu_split3(d["x"], d["w2"], d["b2"], 64, 64, out_f32=True, stem=(d["w1"], d["b1"]))
    sep = vgg.conv3x3_relu_split3(vgg.conv3x3_relu(d["x"], d["w1"], d["b1"], 3, 64), d["w2"], d["b2"], 64, 64, out_f32=True)
    assert torch.equal(got, sep)
    assert torch.equal(got, torch.clamp(d["b2"], min=0).expand_as(got))


def test_fused_stem_refusals(cuda):
    from ntmtrack import _lib, vgg
    assert not vgg.split3_stem_supported(28, 28) and not vgg.split3_stem_supported(12, 16) and vgg.split3_stem_supported(224, 224, True)
    case = _case(1, 16, 16, 0.0)
    d = _device(case, cuda, 16, 16)
    with pytest.raises(_lib.NtkError):            # not frames
        vgg.conv3x3_relu_split3(torch.zeros((1, 16, 16, 64), device=cuda), d["w2"], d["b2"], 64, 64, stem=(d["w1"], d["b1"]))
    with pytest.raises(_lib.NtkError):            # a shape the split form does not cut into sub-blocks
        vgg.conv3x3_relu_split3(torch.zeros((1, 12, 16, 3), device=cuda), d["w2"], d["b2"], 64, 64, stem=(d["w1"], d["b1"]))


# ---- trunk level
@pytest.fixture(scope="module")
def trunk224(cuda):
    from ntmtrack import vgg
    from oracle import ntm_oracle_torch as OT
    rng = np.random.default_rng(11)
    ws = O.init_vgg_weights(rng)
    for k in ws:
        ws[k] = (ws[k][0], (rng.standard_normal(ws[k][1].shape) * 0.05).astype(np.float32))
    frames = (rng.uniform(0, 255, size=(2, 224, 224, 3)).astype(np.float32) - O.VGG_MEAN)
    ref = OT.vgg16_conv43(frames.astype(np.float64), {k: (w.astype(np.float64), b.astype(np.float64)) for k, (w, b) in ws.items()})
    fused = vgg.VGG16Conv43(ws, device=cuda)
    separate = vgg.VGG16Conv43(ws, device=cuda)
    separate.stem = "separate"
    return fused, separate, torch.from_numpy(frames).to(cuda), ref


def test_default_trunk_fuses_the_stem_and_matches_float64(cuda, trunk224, monkeypatch):
    from ntmtrack import vgg
    fused, separate, x, ref = trunk224
    assert fused.stem == "fused" and fused.split3
    log = []
    for name in ("conv3x3_relu", "conv3x3_relu_split3"):
        def spy(*a, _real=getattr(vgg, name), _name=name, **k):
            log.append(_name)
            return _real(*a, **k)
        monkeypatch.setattr(vgg, name, spy)
    got = fused(x)
    monkeypatch.undo()
    assert log == ["conv3x3_relu_split3"] * 9, log                         # no conv3x3_relu launch on the fused route
    plan = fused.last_plan
    assert len(plan) == 10 and (plan[0].kernel, plan[0].dst, plan[1].kernel, plan[1].src) == ("direct", "stem", "split3", "stem")
    sep = separate(x)
    assert separate.last_plan[0].dst == "nhwc" and separate.last_plan[1].src == "nhwc"
    scale = np.max(np.abs(ref))
    err_fused = np.max(np.abs(got.cpu().numpy() - ref)) / scale
    err_sep = np.max(np.abs(sep.cpu().numpy() - ref)) / scale
    diff = float((got - sep).abs().max()) / scale
    print("224 x 224 trunk vs float64: fused stem %.3e  separate stem %.3e  |fused - separate| %.3e of max |y|" % (err_fused, err_sep, diff))
    assert err_fused < 1e-5, err_fused
    # 224 is a multiple of 32: conv1_1 is computed in the row kernel's k order on the same fp32 matrix arithmetic, and everything
    # after it is the same code -- fp32 rounding here means no difference at all
    assert torch.equal(got, sep)


def test_fused_trunk_is_frame_invariant_bit_for_bit(cuda, trunk224):
    fused, _separate, x, _ref = trunk224
    assert torch.equal(fused(x)[:1], fused(x[:1].contiguous()))
    rng = np.random.default_rng(5)
    y = torch.from_numpy(rng.uniform(0, 255, size=(5, 64, 96, 3)).astype(np.float32) - O.VGG_MEAN).to(cuda)
    full = fused(y)
    for k in (1, 3):
        assert torch.equal(full[:k], fused(y[:k].contiguous()))
