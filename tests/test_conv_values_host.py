"""No device: the oracle side of tests/test_conv_values_gpu.py.  For every value regime (tests/conv_value_util.py R0 .. R5) on every
layer shape the split form is run on there, before a kernel is looked at:

  * the MODEL of the split form's arithmetic (fp16 parts as the kernels make them, three products, float64 sums) stays within the
    derived bound D at EVERY output element: the bound the GPU test holds the kernel to, D + c_acc A, can be met by correct
    arithmetic (measured: at most 0.69 of D -- R2 on (5, 20, 28, 16, 64); 0.63 in the saturation regime);
  * the two MUTANTS (fp16 subnormal parts flushed to zero: the weights' or the activations') miss D + c_acc A, at some element, by
    at least 4 x in the regime that exists for them: the weights' in R1 (output-channel gains down to 2^-16 put the low parts of
    the small channels' weights below 2^-14; measured 30 x .. 75 x), the activations' in R2 and R4 (activations down to 2^-12 of
    the suite's; measured 168 x .. 967 x and 81 x .. 270 x).  The GPU bound cannot be met by the failure it exists for.
    Where a regime has nothing for a mutant to flush there is nothing to see, and that is what is asserted for the other two
    combinations of R1 and R2 (the weights' mutant in R2 and the activations' in R1 stay BELOW 4 x); elsewhere it is printed: the
    weights' mutant is the model itself on one layer scale (R0, R3, R4, R5: 0.0 .. 0.6 of the bound; R2 spreads the weights over
    twelve bits, and low parts become subnormal from seventeen: 0.5 .. 1.5), the activations' mutant at the suite's magnitudes
    loses the low parts of the 1.6 % of activations below 2^-3 (R0, R1, R5: 0.7 .. 3.4) and in R3 nothing at all;
  * the regime is the regime: R1 and R2 scale exactly and keep the layer's weight scale (R1) or every fp32 product (R2), every
    64-column block sees every R1 exponent and channel 0 gain 1; R3 has at least 1 % of its activations in each of (0, 65504],
    (65504, 131008] and beyond, and 1 % of its outputs beyond 131008; R4 is all below 2^-3 with a quarter above fp16's smallest
    subnormal; R5 has a third of its channels below -(D + c_acc A) everywhere and a third above +(D + c_acc A) everywhere;
  * c_ref, the accumulation unit (torch-CPU float32 against float64, per A), is what one fp32 summation costs: between 2^-24 / 4
    and 2^-21 (measured 0.98e-7 .. 3.3e-7).
`python tests/test_conv_values_host.py` prints every figure."""
import functools
import sys

import numpy as np
import pytest

import conv_value_util as U

SHAPES = tuple(sorted({row[:5] for row in U.SPLIT_SHAPES}))
MUTANT_FACTOR = 4.0


@functools.lru_cache(maxsize=None)
def figures(regime, shape):
    c = U.case(regime, shape)
    err = lambda pre: np.abs(pre - c.pre)
    f = dict(case=c, c_ref=c.c_ref,
             model=float((err(U.split_model(c.x, c.w, c.b)) / np.maximum(c.D, np.finfo(np.float64).tiny)).max()),
             mut_w=float((err(U.split_model(c.x, c.w, c.b, flush_w=True)) / c.bound).max()),
             mut_x=float((err(U.split_model(c.x, c.w, c.b, flush_x=True)) / c.bound).max()))
    return f


def _line(regime, shape, f):
    return ("%s %-22s c_ref %.2e  model / D %.3f  weights' mutant / bound %6.1f  activations' mutant / bound %6.1f"
            % (regime, shape, f["c_ref"], f["model"], f["mut_w"], f["mut_x"]))


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("regime", U.REGIMES)
def test_model_within_bound_and_mutants_outside(regime, shape):
    f = figures(regime, shape)
    print(_line(regime, shape, f))
    assert 2.0 ** -26 <= f["c_ref"] <= 2.0 ** -21, f["c_ref"]
    assert f["model"] < 1.0, f["model"]
    if regime == "R1":
        assert f["mut_w"] >= MUTANT_FACTOR, f["mut_w"]
        assert f["mut_x"] < MUTANT_FACTOR, f["mut_x"]           # R0's activations: this mutant has next to nothing to flush here
    if regime in ("R2", "R4"):
        assert f["mut_x"] >= MUTANT_FACTOR, f["mut_x"]
    if regime == "R2":
        assert f["mut_w"] < MUTANT_FACTOR, f["mut_w"]           # twelve bits of spread: no low part of a weight is subnormal yet


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_regimes_are_what_they_say(shape):
    cin, cout = shape[3], shape[4]
    r0 = figures("R0", shape)["case"]
    # R1: exact gains, channel 0 and the layer's weight scale untouched, the whole spread in every 64-column block
    r1, k1 = figures("R1", shape)["case"], U.r1_exponents(cout)
    assert k1[0] == 0 and all(sorted(set(k1[i:i + 64])) == list(range(U.R1_BITS + 1)) for i in range(0, cout, 64))
    assert np.array_equal(r1.w.astype(np.float64) * 2.0 ** k1, r0.w) and np.array_equal(r1.b.astype(np.float64) * 2.0 ** k1, r0.b)
    assert U.w_scale(r1.w) == U.w_scale(r0.w) and np.array_equal(r1.x, r0.x)
    # R2: exact gains both ways, so every fp32 product x w has R0's bits
    r2, k2 = figures("R2", shape)["case"], U.r2_exponents(cin)
    assert k2.min() == 0 and k2.max() == U.R2_BITS
    assert np.array_equal(r2.x.astype(np.float64) * 2.0 ** k2, r0.x) and np.array_equal(r2.w.astype(np.float64) * 2.0 ** -k2[:, None], r0.w)
    prod = lambda c: c.x[0, 0, 0, :, None] * c.w[1, 1]
    assert np.array_equal(prod(r2), prod(r0))
    # R3: the three bands of the activations, and outputs beyond the split map's range
    r3 = figures("R3", shape)["case"]
    x = r3.x.astype(np.float64)
    bands = [float(np.mean((x > lo) & (x <= hi))) for lo, hi in ((0.0, U.FP16_MAX), (U.FP16_MAX, U.S3_MAX), (U.S3_MAX, np.inf))]
    beyond = float(np.mean(r3.pre > U.S3_MAX))
    print("R3 %s: %.1f %% / %.1f %% / %.1f %% of the activations in (0, 65504] / (65504, 131008] / beyond; %.1f %% of the outputs beyond"
          % ((shape,) + tuple(100 * v for v in bands + [beyond])))
    assert min(bands) >= 0.01 and beyond >= 0.01, (bands, beyond)
    # R4: all below 2^-3 (every low part an fp16 subnormal), not all below the smallest subnormal
    r4 = figures("R4", shape)["case"]
    assert 0 < r4.x.max() < 2.0 ** -3 and float(np.mean(r4.x > 2.0 ** -24)) > 0.25
    # R5: a third of the channels dead, a third alive, by more than the bound, everywhere
    r5 = figures("R5", shape)["case"]
    n = np.arange(cout)
    dead, alive = n % 3 == 0, n % 3 == 1
    assert dead.sum() >= cout // 3 and alive.sum() >= cout // 3
    assert (r5.pre[..., dead] < -r5.bound[..., dead]).all() and (r5.pre[..., alive] > r5.bound[..., alive]).all()
    rest = r5.pre[..., ~(dead | alive)]
    assert 0.2 < float(np.mean(rest > 0)) < 0.8


def test_part_models_at_their_edges():
    """the part models on hand-picked values: saturation, the clamp, the floor, the rounding directions"""
    v = np.array([0.0, 1.0, 1.0 + 2.0 ** -10 - 2.0 ** -20, 65504.0, 65519.9, 70000.0, 131008.0, 1e9, 2.0 ** -3, 3e-5, 2.0 ** -26])
    xh, xl = U.x_parts(v)
    assert list(xh[:8]) == [0.0, 1.0, 1.0, 65504.0, 65504.0, 65504.0, 65504.0, 65504.0]          # toward zero, saturating
    assert xl[2] == np.float64(np.float16(2.0 ** -10 - 2.0 ** -20)) and xl[6] == 65504.0 and xl[7] == 65504.0
    assert (np.abs(np.minimum(v, U.S3_MAX) - xh - xl) <= U.dx(np.minimum(v, U.S3_MAX))).all()
    assert U.dx(np.array([0.0]))[0] == 0 and U.dx(np.array([2.0 ** -4]))[0] == 2.0 ** -25 and U.dx(np.array([1.0]))[0] == 2.0 ** -22
    assert U.dx(np.array([65504.0 + 4096.0]))[0] == 2.0 and U.dx(np.array([131008.0]))[0] == 16.0
    xhf, xlf = U.x_parts(v, flush=True)
    assert xhf[9] == 0 and xlf[8] == 0 and xhf[8] == 2.0 ** -3
    w = np.array([0.75, -0.75 * 2.0 ** -17 * (1 + 2.0 ** -12), 3e-9, 0.0], np.float32).reshape(1, 1, 4, 1)
    wh, wl, scale = U.w_parts(w)
    assert scale == 2.0 ** 14 and wh.ravel()[0] == 0.75 * 2.0 ** 14
    assert (np.abs(w.astype(np.float64) - (wh + wl) / scale) <= U.dw(w)).all()
    assert U.w_parts(w, flush=True)[1].ravel()[1] == 0 and wl.ravel()[1] != 0                     # 2^-17 of the largest: a subnormal low part


def test_winograd_restatement_matches_float64():
    """the fp32 restatement of the Winograd kernels' arithmetic (moved here from scripts/dev_wino43_numerics.py) computes the
    convolution: within the project's per-form bounds (1e-5 for F(2x2), 3e-5 for F(4x4)) of float64 on a layer-like input"""
    rng = np.random.default_rng(0)
    x = np.maximum(rng.standard_normal((8, 8, 32)), 0).astype(np.float32) * 2
    w = (rng.standard_normal((3, 3, 32, 16)) * np.sqrt(2.0 / (9 * 32))).astype(np.float32)
    ref = U.direct64(x, w)
    assert np.allclose(ref, U.conv_pre(x[None], w)[0], rtol=0, atol=1e-12)
    s = np.abs(ref).max()
    assert np.abs(U.wino23(x, w) - ref).max() / s < 1e-5 and np.abs(U.wino43(x, w) - ref).max() / s < 3e-5


if __name__ == "__main__":
    for shape in SHAPES:
        for regime in U.REGIMES:
            print(_line(regime, shape, figures(regime, shape)), flush=True)
    sys.exit(0)
