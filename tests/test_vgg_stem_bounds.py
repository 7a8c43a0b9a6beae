"""CPU: the oracles and bounds of tests/test_vgg_stem_shapes_gpu.py have teeth, and admit the arithmetic the fused stem is meant to do.

No device: float64 models of conv1_2's input map stand in for the kernel.  The RIGHT model (conv1_1 rounded to fp32, clamped to
[0, 131008], split into fp16 hi (toward zero, saturating) + lo (to nearest), the product of the two low parts dropped) must lie
inside each case's bound; each WRONG model -- conv1_1 evaluated outside the frame, the high part alone or saturating at 65504 with
nothing carried, no clamp at 131008, values under fp16's normal range flushed to zero -- must lie outside it.  (What the bounds do
not resolve, by construction: a clamp 64 higher -- half an fp16 spacing of the low part there is 16 -- and, below 6e-5, the loss
of the last one or two bits of 2^-24.)"""
import numpy as np
import pytest

from oracle import ntm_oracle_torch as OT
import test_vgg_stem_shapes_gpu as T


def test_rtz_fp16_on_every_fp16_value_and_between():
    h = np.arange(0, 0x7C00, dtype=np.uint16).view(np.float16).astype(np.float64)         # every finite fp16 >= 0, ascending
    assert np.array_equal(T._rtz_fp16(h), h)
    up = np.append(h[1:], 2.0 ** 16)
    for t in (0.25, 0.5, 0.75, 1 - 2.0 ** -20):
        assert np.array_equal(T._rtz_fp16(h + t * (up - h)), h), t
    assert np.array_equal(T._rtz_fp16(np.array([65504.0, 65520.0, 1e5, 131008.0])), np.full(4, 65504.0))


def _conv1_2(y1, lo=None):
    """float64 conv1_2 of a model of its input map (the weights of the range cases); lo: minus the dropped lo x wl product"""
    _w1, _b1, w2, b2 = T._weights(0.0)
    if lo is None:
        return OT.conv3x3_same_relu(y1, w2, b2)
    return OT.conv3x3_same_relu(np.concatenate((y1, lo), axis=3), np.concatenate((w2.astype(np.float64), -T._w2_low_part(w2)), axis=2), b2)


def _split(y1):
    v = np.clip(y1.astype(np.float32).astype(np.float64), 0, T.S3_MAX)
    hi = T._rtz_fp16(v)
    return hi, (v - hi).astype(np.float16).astype(np.float64)


def _inside(case, y2):
    return bool((np.abs(y2 - case["ref"][False]) <= case["bound"][False]).all())


@pytest.mark.parametrize("frames,H,W", T.RANGE_SHAPES)
def test_range_bounds_admit_the_split_arithmetic_and_no_other(frames, H, W):
    sat, floor = T._range_case(frames, H, W, T.SATURATION_FACTOR), T._range_case(frames, H, W, T.FLOOR_FACTOR)
    for case in (sat, floor):
        hi, lo = _split(case["y1"])
        assert _inside(case, _conv1_2(hi + lo, lo))                                        # what the kernel is meant to compute
    y1 = sat["y1"]
    assert not _inside(sat, _conv1_2(_split(y1)[0]))                                       # the low part lost (below 6e-5 it is < 2^-24)
    assert not _inside(sat, _conv1_2(np.minimum(y1, T.FP16_MAX)))                          # saturating with nothing carried
    assert not _inside(sat, _conv1_2(y1))                                                  # no clamp at 131008
    y1 = floor["y1"]
    assert not _inside(floor, _conv1_2(np.where(y1 < 2.0 ** -14, 0.0, y1)))                # subnormal parts flushed to zero


@pytest.mark.parametrize("bias1", [0.0, 0.5])
def test_split_layer_bound_sees_conv1_1_evaluated_outside_the_frame(bias1):
    """the model that pads the FRAME by two pixels and conv1_1's map not at all: wrong on the frame's border only"""
    w1, b1, w2, b2 = T._weights(bias1)
    for H, W in ((8, 8), (16, 32)):
        x = T._frames(1, H, W)
        ref = OT.conv3x3_same_relu(OT.conv3x3_same_relu(x, w1, b1), w2, b2)
        y1p = OT.conv3x3_same_relu(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))), w1, b1)
        err = np.abs(OT.conv3x3_same_relu(y1p, w2, b2)[:, 1:-1, 1:-1] - ref)
        assert err[:, 1:-1, 1:-1].max() == 0
        border = np.ones((H, W), bool)
        border[1:-1, 1:-1] = False
        assert (err[0][border].max(axis=1) / ref.max() > 1000 * T.SPLIT_LAYER_BOUND).all()  # every border pixel, by three orders
