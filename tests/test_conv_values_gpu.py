"""GPU: the trunk's conv forms where their VALUES change -- per output channel, per input channel and at the edges of fp16's range.

Every other conv test draws relu(N(0,1)) 3 activations and He-scaled weights of one magnitude and measures max |got - ref| / max |ref|
over the whole map: one number that hides every channel smaller than the largest.  Here the operands go through the value regimes of
tests/conv_value_util.py (R0 the suite's operands, R1 output-channel gains down to 2^-16, R2 input-channel gains down to 2^-12 with
the weights scaled back, R3 activations beyond 65504 and 131008, R4 activations below 2^-3, R5 a third of the channels dead and a
third always alive), all built with powers of two, and every comparison is made at EVERY output element.
tests/test_conv_values_host.py holds the oracle side without a device: the bounds used here can be met by correct split arithmetic
and cannot be met by arithmetic that flushes fp16 subnormal parts.

SPLIT form (csrc/conv_bf16p.hip X3), one shape per instantiation (conv_value_util.SPLIT_SHAPES), every regime:
  * |got - float64| <= D + c_acc A at every element, fp32 and split-map output (the split map against min(y, 131008): its epilogue
    clamps; the fp32 epilogue does not), a pooled output against the 2x2 maximum of the bound.  The fp32 output meets it in every
    regime.  The split map meets it except where its own format's error dx(y) is the larger one (all of R1, one case of R3:
    strict expected failures, figures at _SPLIT_MAP_BEYOND_FORMAT); it meets D + c_acc A + dx(y) everywhere, and is within dx of
    the fp32 map of the same launch;
  * the split map == to_split(the fp32 map clamped at 131008); an fp32 input gives the bits of its to_split() map; a second launch
    gives the same bits;
  * R1: the channels with gain 1 carry R0's bits;
  * the sign: got > 0 exactly where the float64 pre-activation is positive, outside the band |pre-activation| <= bound; R5: dead
    channels are +0.0 bit for bit (both parts of a split map), alive channels > 0 everywhere.
D is derived from the parts' formats, A = sum |x| |w| + |b|, and c_acc = 4 c_ref with c_ref = max |torch-CPU float32 conv - float64| / A
of the same operands: nothing in a bound comes from a kernel's output.
The OTHER forms (direct, wino, wino43 on eight and four waves and on blocked maps, bf16, bf16p) on (3, 8, 8, 32 -> 64) and
(3, 20, 28, 64 -> 64), pooled and un-pooled, wherever their predicates accept:
  * R1 and R2 are EXACT: scaling by a power of two commutes with every fp32 and bf16 rounding and with the (linear) Winograd
    transforms, so channel n of R1 is g_n x R0's channel bit for bit and R2's map is R0's map bit for bit -- a mismatch is a hidden
    clamp, a flush, a narrower intermediate or leakage between channels;
  * direct and the bf16 forms with an fp32 output, R0 and R5: |got - float64| <= c_acc A at every element (bf16 forms: against
    bf16-rounded operands);
  * R5 as above; the band of the Winograd forms is the project's per-form bound (1e-5 / 3e-5) of the channel's max |ref|.
Every figure is printed on a line that starts with "conv_values"; profiles/conv_values.txt holds a run's."""
import functools

import numpy as np
import pytest
import torch

import conv_value_util as U

pytestmark = pytest.mark.gpu

TINY = np.finfo(np.float64).tiny


def _t(a, cuda):
    return torch.from_numpy(np.ascontiguousarray(a)).to(cuda)


def _np64(t):
    return t.float().cpu().numpy().astype(np.float64)


def _pointwise(tag, got, ref, bound, D, cA):
    """|got - ref| <= bound at every element; prints the worst err / bound and the accumulation factor max (err - D)+ / (c_ref A)"""
    assert got.shape == ref.shape, (tag, got.shape, ref.shape)
    assert np.isfinite(got).all(), tag
    err = np.abs(got - ref)
    ratio = float((err / np.maximum(bound, TINY)).max())
    factor = float((np.maximum(err - D, 0) / np.maximum(cA, TINY)).max())
    print("conv_values %s: err / bound %.3f, err / (c_ref A) %.2f, accumulation factor (err - D)+ / (c_ref A) %.2f (allowed %.0f), err / max |ref| %.2e"
          % (tag, ratio, float((err / np.maximum(cA, TINY)).max()), factor, U.Case.ACC_MARGIN, err.max() / max(np.abs(ref).max(), TINY)))
    bad = err > bound
    assert not bad.any(), "%s: %d elements beyond the bound, worst %.3f x, in channels %s" % (
        tag, int(bad.sum()), ratio, sorted(set(np.nonzero(bad)[-1].tolist()))[:16])


def _sign(tag, got, pre, band):
    """got > 0 exactly where the float64 pre-activation is positive, outside the band"""
    out = np.abs(pre) > band
    wrong = out & ((got > 0) != (pre > 0))
    assert not wrong.any(), "%s: %d signs differ outside the band, channels %s" % (tag, int(wrong.sum()), sorted(set(np.nonzero(wrong)[-1].tolist()))[:16])


def _split_parts(ys):
    """split map [F,H,W,C/16,2,16] -> the bit patterns of its high and low parts, [F,H,W,C] each"""
    F, H, W, G = ys.shape[:4]
    bits = ys.view(torch.int16)
    return bits[:, :, :, :, 0].reshape(F, H, W, G * 16), bits[:, :, :, :, 1].reshape(F, H, W, G * 16)


def _r5_channels(cout, cuda):
    n = torch.arange(cout, device=cuda)
    return n % 3 == 0, n % 3 == 1


def _run_split(cuda, c, H, W, pool, in_f32, out_f32):
    from ntmtrack import vgg
    cin, cout = c.shape[3], c.shape[4]
    xt, bt = _t(c.x, cuda), _t(c.b, cuda)
    wp = vgg.pack_weights_split3(_t(c.w, cuda), H, W)
    return vgg.conv3x3_relu_split3(xt if in_f32 else vgg.to_split(xt), wp, bt, cin, cout, fuse_pool=pool, out_f32=out_f32)


def _split_case(regime, row):
    F, H, W, cin, cout, pool, in_f32, out_f32 = U.SPLIT_SHAPES[row]
    c = U.case(regime, (F, H, W, cin, cout))
    tag = "split3 %s %s pool=%d in_f32=%d" % (regime, (F, H, W, cin, cout), pool, in_f32)
    return c, tag, c.pooled(c.bound, pool), c.pooled(c.D, pool), c.c_ref * c.pooled(c.A, pool), c.pooled(c.pre, pool)


_ROW_ID = lambda i: "-".join(str(int(v)) for v in U.SPLIT_SHAPES[i])
# The split MAP as an output carries every value with its own format's error dx(y) (conv_value_util.dx): an absolute 2^-25 below 2^-3,
# up to 16 just under 131008.  The layer's bound D + c_acc A has no term for it, and the format cannot meet it where a channel's
# outputs are small against 2^-25 or a layer's bound is small against 16 -- measured on an MI355X, worst err / bound per case:
#   R1 (channels of gain 2^-16: outputs of 1e-5 carried to 3e-8, 2^-9 relative), the thirteen rows in order:
#      28.1, 50.6, 23.6, 106.2, 46.8, 18.9, 44.2, 21.3, 37.3, 41.2, 118.8, 37.0, 43.0
#   R3, (5, 20, 28, 16, 64) only (144 terms: the smallest bound of the thirteen): 1.108 at ONE element
# The kernel's arithmetic is right in both (the fp32 output of the same launch meets the bound, and the split map is to_split() of it
# bit for bit): the floor is the map format's, and only a per-channel activation scale would lift it.  Those cases are strict
# expected failures; test_split_form_pointwise holds every split map to D + c_acc A + dx(y), which they all meet (worst 0.984).
_SPLIT_MAP_BEYOND_FORMAT = {("R1", row) for row in U.SPLIT_SHAPES} | {("R3", (5, 20, 28, 16, 64, False, False, False))}
assert all(row in U.SPLIT_SHAPES for _regime, row in _SPLIT_MAP_BEYOND_FORMAT)


@pytest.mark.parametrize("regime,row", [
    pytest.param(regime, row, id="%s-%s" % (regime, _ROW_ID(row)),
                 marks=[pytest.mark.xfail(strict=True, reason="the split map's own format error dx(y) exceeds D + c_acc A here")]
                 if (regime, U.SPLIT_SHAPES[row]) in _SPLIT_MAP_BEYOND_FORMAT else [])
    for regime in U.REGIMES for row in range(len(U.SPLIT_SHAPES))])
def test_split_map_output_within_the_layer_bound(cuda, regime, row):
    """|split map - min(float64, 131008)| <= D + c_acc A at every element, and its sign outside that band"""
    from ntmtrack import vgg
    F, H, W, cin, cout, pool, in_f32, out_f32 = U.SPLIT_SHAPES[row]
    c, tag, bound, D, cA, pre = _split_case(regime, row)
    gs = _np64(vgg.from_split(_run_split(cuda, c, H, W, pool, in_f32, False)))
    _pointwise(tag + " split out", gs, c.ref(pool, clamp_out=True), bound, D, cA)
    _sign(tag + " split out", gs, pre, bound)


@pytest.mark.parametrize("row", range(len(U.SPLIT_SHAPES)), ids=_ROW_ID)
@pytest.mark.parametrize("regime", U.REGIMES)
def test_split_form_pointwise(cuda, regime, row):
    from ntmtrack import vgg
    F, H, W, cin, cout, pool, in_f32, out_f32 = U.SPLIT_SHAPES[row]
    assert vgg.split3_supported(H, W, cin, cout, pool)
    c, tag, bound, D, cA, pre = _split_case(regime, row)
    y32 = _run_split(cuda, c, H, W, pool, in_f32, True)
    ys = _run_split(cuda, c, H, W, pool, in_f32, False)
    torch.cuda.synchronize()
    g32, gs = _np64(y32), _np64(vgg.from_split(ys))
    _pointwise(tag + " fp32 out", g32, c.ref(pool), bound, D, cA)
    _sign(tag + " fp32 out", g32, pre, bound)
    # the split map: the layer's bound + the error of its own format at that value (dx is monotone: at ref + bound, from the
    # reference side alone); against the fp32 map of the same launch, the format's error alone
    refc = c.ref(pool, clamp_out=True)
    top = np.minimum(refc + bound, U.S3_MAX)
    fmt = np.maximum(U.dx(top), 2.0 ** -22 * np.minimum(top, U.FP16_MAX))        # dx drops at 65504: its monotone envelope
    _pointwise(tag + " split out, bound + dx(y)", gs, refc, bound + fmt, D + fmt, cA)
    _sign(tag + " split out, bound + dx(y)", gs, pre, bound + fmt)
    g32c = np.minimum(g32, U.S3_MAX)
    assert (np.abs(gs - g32c) <= U.dx(g32c)).all(), tag + ": the split map is further from its fp32 map than the format's dx"
    if regime == "R3":                                        # pinned: the fp32 epilogue does not clamp, the split epilogue does
        assert float(y32.max()) > U.S3_MAX and float(vgg.from_split(ys).max()) == U.S3_MAX
    assert torch.equal(ys, vgg.to_split(y32.clamp(max=U.S3_MAX))), tag + ": split map != to_split(fp32 map)"
    assert torch.equal(ys, _run_split(cuda, c, H, W, pool, in_f32, False)), tag + ": a second launch differs"
    if in_f32:
        assert torch.equal(ys, _run_split(cuda, c, H, W, pool, False, False)), tag + ": fp32 input != its to_split() map"
        assert torch.equal(y32, _run_split(cuda, c, H, W, pool, False, True)), tag + ": fp32 input != its to_split() map (fp32 out)"
    if regime == "R1":
        k = U.r1_exponents(cout)
        c0 = U.case("R0", (F, H, W, cin, cout))
        one = torch.from_numpy(k == 0).to(cuda)
        assert int(one.sum()) >= 2 * (cout // 64)
        assert torch.equal(y32[..., one], _run_split(cuda, c0, H, W, pool, in_f32, True)[..., one]), tag + ": gain-1 channels differ from R0"
        small = k == U.R1_BITS
        ref, err = c.ref(pool)[..., small], np.abs(g32 - c.ref(pool))[..., small]
        print("conv_values %s: channels of gain 2^-%d: worst err / max |ref_n| %.2e (whole map: %.2e)"
              % (tag, U.R1_BITS, float((err.max(axis=(0, 1, 2)) / np.maximum(ref.max(axis=(0, 1, 2)), TINY)).max()),
                 np.abs(g32 - c.ref(pool)).max() / c.ref(pool).max()))
    if regime == "R5":
        dead, alive = _r5_channels(cout, cuda)
        hi, lo = _split_parts(ys)
        assert bool((y32[..., dead].view(torch.int32) == 0).all()), tag + ": a dead channel is not +0.0 (fp32 map)"
        assert bool((hi[..., dead] == 0).all()) and bool((lo[..., dead] == 0).all()), tag + ": a dead channel is not +0.0 (split map)"
        assert bool((y32[..., alive] > 0).all()) and bool((vgg.from_split(ys)[..., alive] > 0).all()), tag + ": an alive channel is not > 0"


# ---------------------------------------------------------------------------------------------------------------------------------
OTHER_FORMS = ("direct", "wino", "wino43", "bf16", "bf16p")
WINO_BAND = {"wino": 1e-5, "wino43": 3e-5}          # the per-form bounds of tests/test_vgg_gpu.py, of max |ref|


@functools.lru_cache(maxsize=None)
def _other_case(regime, shape, bf16):
    return U.Case(regime, *shape, split=False, bf16=bf16)


def _variants(form, cuda, c, H, W, pool):
    """{variant: output tensor} of every variant of `form` on the case's operands"""
    from ntmtrack import vgg
    cin, cout = c.shape[3], c.shape[4]
    xt, wt, bt = _t(c.x, cuda), _t(c.w, cuda), _t(c.b, cuda)
    if form == "direct":
        return {"fp32": vgg.conv3x3_relu(xt, vgg.pack_weights(wt), bt, cin, cout, fuse_pool=pool)}
    if form == "wino":
        return {"fp32": vgg.conv3x3_relu_wino(xt, vgg.pack_weights_wino(wt), bt, cin, cout, fuse_pool=pool)}
    if form == "wino43":
        u = vgg.pack_weights_wino43(wt)
        yb = vgg.conv3x3_relu_wino43_blocked(vgg.nhwc_to_blocked(xt), u, bt, cin, cout, fuse_pool=pool, out_blocked=True)
        return {"eight waves": vgg.conv3x3_relu_wino43(xt, u, bt, cin, cout, fuse_pool=pool, waves=8),
                "four waves": vgg.conv3x3_relu_wino43(xt, u, bt, cin, cout, fuse_pool=pool, waves=4),
                "blocked maps": vgg.blocked_to_nhwc(yb)}
    xb = xt.to(torch.bfloat16)
    assert torch.equal(xb.float(), xt)                        # the case's activations are bf16 numbers
    wp, conv = ((vgg.pack_weights_bf16p(wt, H, W), vgg.conv3x3_relu_bf16p) if form == "bf16p" else
                (vgg.pack_weights_bf16(wt), vgg.conv3x3_relu_bf16))
    return {"bf16 out": conv(xb, wp, bt, cin, cout, fuse_pool=pool), "fp32 out": conv(xb, wp, bt, cin, cout, fuse_pool=pool, out_f32=True)}


def _mismatch(a, b):
    """where two maps differ: how many elements, which channels, and how (for the report of a failed exactness check)"""
    a, b = a.float(), b.float()
    ne = a != b
    ch = torch.nonzero(ne.reshape(-1, ne.shape[-1]).any(dim=0)).view(-1).tolist()
    zero = int(((a == 0) != (b == 0))[ne].sum())
    rel = float(((a - b).abs()[ne] / b.abs()[ne].clamp(min=1e-45)).max())
    return "%d elements in channels %s differ, %d of them zero on one side only, worst relative difference %.2e" % (int(ne.sum()), ch[:24], zero, rel)


@pytest.mark.parametrize("form", OTHER_FORMS)
def test_other_forms_scale_exactly_and_hold_their_signs(cuda, form):
    bf16 = form in ("bf16", "bf16p")
    ran = 0
    for shape in U.OTHER_SHAPES:
        F, H, W, cin, cout = shape
        for pool in (False, True):
            if not U.accepts(form, F, H, W, cin, cout, pool):
                continue
            ran += 1
            cases = {r: _other_case(r, shape, bf16) for r in ("R0", "R1", "R2", "R5")}
            out = {r: _variants(form, cuda, c, H, W, pool) for r, c in cases.items()}
            torch.cuda.synchronize()
            g1 = torch.from_numpy((2.0 ** -U.r1_exponents(cout)).astype(np.float32)).to(cuda)
            for v in out["R0"]:
                tag = "%s %s %s pool=%d" % (form, v, shape, pool)
                y0 = out["R0"][v].float()
                assert bool((y0 > 0).any())
                # exact homogeneity
                assert torch.equal(out["R1"][v].float(), y0 * g1), "%s R1: channel n is not g_n x R0's: %s" % (tag, _mismatch(out["R1"][v], y0 * g1))
                assert torch.equal(out["R2"][v].float(), y0), "%s R2: not R0's bits: %s" % (tag, _mismatch(out["R2"][v], y0))
                print("conv_values %s R1, R2: exact" % tag)
                for r in ("R0", "R5"):
                    c, got = cases[r], _np64(out[r][v])
                    pre, A = c.pooled(c.pre, pool), c.pooled(c.A, pool)
                    ref = c.ref(pool)
                    if form in WINO_BAND:
                        band = WINO_BAND[form] * ref.max(axis=(0, 1, 2))
                        err = np.abs(got - ref)
                        print("conv_values %s %s: err / max |ref| %.2e (the form's bound %.0e), accumulation factor %.2f (of c_ref; not bounded)"
                              % (tag, r, err.max() / ref.max(), WINO_BAND[form], float((err / (c.c_ref * A)).max())))
                    else:
                        band = c.c_acc * A
                        if out[r][v].dtype == torch.float32:
                            _pointwise("%s %s" % (tag, r), got, ref, band, 0.0, c.c_ref * A)
                    _sign("%s %s" % (tag, r), got, pre, band)
                dead, alive = _r5_channels(cout, cuda)
                y5 = out["R5"][v]
                bits = y5.view(torch.int32 if y5.dtype == torch.float32 else torch.int16)
                assert bool((bits[..., dead] == 0).all()), tag + " R5: a dead channel is not +0.0"
                assert bool((y5[..., alive] > 0).all()), tag + " R5: an alive channel is not > 0"
    assert ran >= (1 if form == "bf16" else 2), (form, ran)
