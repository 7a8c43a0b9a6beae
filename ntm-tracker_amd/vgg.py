"""VGG-16 conv1_1 .. conv4_3 feature extractor on the HIP MFMA conv kernel.

Replaces the frozen-GraphDef import of the reference
(direct_offset_output.py:417-422; layer spec vgg.py:155-161): ten
[conv3x3 SAME + bias + ReLU] layers with 2x2/2 max-pools after conv1_2,
conv2_2 and conv3_3 (fused into the producing conv's epilogue), NHWC fp32,
TF HWIO weights.  The extractor is frozen (constants in the reference), so it
is inference-only.
"""
import math
import os
from collections import namedtuple

import torch

from . import _lib

# (name, Cin, Cout, pool_after) -- vgg.py:155-160
VGG_LAYERS = [
    ("conv1_1", 3, 64, False), ("conv1_2", 64, 64, True),
    ("conv2_1", 64, 128, False), ("conv2_2", 128, 128, True),
    ("conv3_1", 128, 256, False), ("conv3_2", 256, 256, False), ("conv3_3", 256, 256, True),
    ("conv4_1", 256, 512, False), ("conv4_2", 512, 512, False), ("conv4_3", 512, 512, False),
]

# algorithmic MACs per 224x224 frame: sum H*W*9*Cin*Cout
def conv_flops_per_frame(h=224, w=224):
    total = 0
    for _name, cin, cout, pool in VGG_LAYERS:
        total += 2 * h * w * 9 * cin * cout
        if pool:
            h //= 2
            w //= 2
    return total


# activation maps by layout: fp32 "nhwc" [F,H,W,C], fp32 channel-"blocked" [F,H,C/8,W,8], fp16 "split" [F,H,W,C/16,2,16] (hi | lo parts),
# "bf16" [F,H,W,C]
_MAP_DTYPE = {"nhwc": torch.float32, "blocked": torch.float32, "split": torch.float16, "bf16": torch.bfloat16}


def _map_shape(layout, F, H, W, C):
    if layout == "blocked":
        return (F, H, C // 8, W, 8)
    if layout == "split":
        return (F, H, W, C // 16, 2, 16)
    return (F, H, W, C)


def _conv(entry, x, src, dst, w_packed, bias, cin, cout, fuse_pool, out, tail, err, *err_args):
    """What the conv3x3_relu* wrappers share: `x` must be a `src` map of cin channels (else NtkError(err % err_args)); the output
    map, in the `dst` layout, is allocated unless given; one checked call of the library's `entry` with the common arguments and
    `tail`.  fuse_pool None: the entry has no pool argument."""
    F, H, W = (x.shape[0], x.shape[1], x.shape[3 if src == "blocked" else 2]) if x.dim() >= 4 else (0, 0, 0)
    if x.dtype != _MAP_DTYPE[src] or tuple(x.shape) != _map_shape(src, F, H, W, cin):
        raise _lib.NtkError(err % err_args)
    if out is None:
        oh, ow = (H // 2, W // 2) if fuse_pool else (H, W)
        out = torch.empty(_map_shape(dst, F, oh, ow, cout), device=x.device, dtype=_MAP_DTYPE[dst])
    pool = () if fuse_pool is None else (1 if fuse_pool else 0,)
    _lib.check(getattr(_lib.lib(), entry)(_lib.ptr(x), _lib.ptr(w_packed), _lib.ptr(bias), _lib.ptr(out), F, H, W, cin, cout,
                                          *pool, *tail, _lib.stream()), entry)
    return out


def _channels(x):
    return x.shape[3] if x.dim() == 4 else -1


def conv3x3_relu(x, w_packed, bias, cin, cout, fuse_pool=False, out=None):
    """x [F,H,W,Cin] fp32 NHWC device tensor -> relu(conv3x3_same(x)+b), optionally 2x2 max-pooled."""
    return _conv("ntk_vgg_conv3x3_relu_f32", x, "nhwc", "nhwc", w_packed, bias, cin, cout, fuse_pool, out, (),
                 "conv3x3_relu: input has %d channels, layer expects %d", _channels(x), cin)


def conv3x3_relu_f32_to_bf16(x, w_packed, bias, cin, cout, out=None):
    """conv3x3_relu of fp32 NHWC frames written as a bf16 map (where the bf16 trunk starts: conv1_1)."""
    return _conv("ntk_vgg_conv3x3_relu_f32_to_bf16", x, "nhwc", "bf16", w_packed, bias, cin, cout, None, out, (),
                 "conv3x3_relu_f32_to_bf16: input has %d channels, layer expects %d", _channels(x), cin)


def pack_weights(w_hwio):
    """[3,3,Cin,Cout] (TF HWIO) device tensor -> kernel layout [Cout][Kp]."""
    kh, kw, cin, cout = w_hwio.shape
    assert kh == 3 and kw == 3
    L = _lib.lib()
    kp = L.ntk_vgg_packed_k(cin)
    wp = torch.empty((cout, kp), device=w_hwio.device, dtype=torch.float32)
    _lib.check(L.ntk_vgg_pack_weights(_lib.ptr(w_hwio.contiguous()), _lib.ptr(wp), cin, cout, _lib.stream()),
               "ntk_vgg_pack_weights")
    return wp


def wino_supported(cin, cout, H, W, frames=1):
    """Shapes the fused Winograd kernel takes (otherwise the direct kernel runs): the entry's own answer (csrc/conv_wino.hip, wino_form)."""
    return bool(_lib.lib().ntk_vgg_wino_supported(frames, H, W, cin, cout))


def pack_weights_wino(w_hwio):
    """[3,3,Cin,Cout] (TF HWIO) -> Winograd-domain weights U = G g G^T packed for the MFMA B operand."""
    kh, kw, cin, cout = w_hwio.shape
    assert kh == 3 and kw == 3
    L = _lib.lib()
    u = torch.empty(L.ntk_vgg_wino_packed_floats(cin, cout), device=w_hwio.device, dtype=torch.float32)
    w = w_hwio.contiguous()
    _lib.check(L.ntk_vgg_pack_weights_wino(_lib.ptr(w), _lib.ptr(u), cin, cout, _lib.stream()), "ntk_vgg_pack_weights_wino")
    return u


def conv3x3_relu_wino(x, u_packed, bias, cin, cout, fuse_pool=False, out=None):
    """Same operator as conv3x3_relu by fused Winograd F(2x2,3x3) (csrc/conv_wino.hip)."""
    return _conv("ntk_vgg_conv3x3_relu_wino_f32", x, "nhwc", "nhwc", u_packed, bias, cin, cout, fuse_pool, out, (),
                 "conv3x3_relu_wino: input has %d channels, layer expects %d", _channels(x), cin)


def wino43_supported(cin, cout, H, W, frames=1):
    """Shapes the fused Winograd F(4x4,3x3) kernel takes: the launcher's own answer (csrc/conv_wino43.hip, wino43_form)."""
    return bool(_lib.lib().ntk_vgg_wino43_supported(frames, H, W, cin, cout))


def pack_weights_wino43(w_hwio):
    """[3,3,Cin,Cout] (TF HWIO) -> the 36 Winograd-domain planes U = G g G^T of F(4x4,3x3), packed for the MFMA B operand."""
    kh, kw, cin, cout = w_hwio.shape
    assert kh == 3 and kw == 3
    L = _lib.lib()
    u = torch.empty(L.ntk_vgg_wino43_packed_floats(cin, cout), device=w_hwio.device, dtype=torch.float32)
    w = w_hwio.contiguous()
    _lib.check(L.ntk_vgg_pack_weights_wino43(_lib.ptr(w), _lib.ptr(u), cin, cout, _lib.stream()), "ntk_vgg_pack_weights_wino43")
    return u


def conv3x3_relu_wino43(x, u_packed, bias, cin, cout, fuse_pool=False, out=None, window=None, waves=None):
    """Same operator as conv3x3_relu by fused Winograd F(4x4,3x3) (csrc/conv_wino43.hip).
    window = (y0, x0, y1, x1), multiples of 4: compute only that part of the un-pooled output (the rest of `out` is not touched).
    waves = 4 / 8: the one- / two-waves-per-SIMD form of the kernel (default: 8; same bits)."""
    win = tuple(int(v) for v in window) if window is not None else None
    if waves is not None:
        entry, tail = "ntk_vgg_conv3x3_relu_wino43_form_f32", (win or (0, 0, x.shape[1], x.shape[2])) + (int(waves),)
    elif win is not None:
        entry, tail = "ntk_vgg_conv3x3_relu_wino43_window_f32", win
    else:
        entry, tail = "ntk_vgg_conv3x3_relu_wino43_f32", ()
    return _conv(entry, x, "nhwc", "nhwc", u_packed, bias, cin, cout, fuse_pool, out, tail,
                 "conv3x3_relu_wino43: input has %d channels, layer expects %d", _channels(x), cin)


def blocked_trunk_supported(frames, H, W):
    """Can conv1_2 .. conv4_3 of a [frames,H,W,3] batch hand channel-blocked maps [H][C/8][W][8] to each other?  Every one of them
    must be a shape of the eight-wave F(4x4) kernel (ntk_vgg_wino43_blocked_supported), which holds only for H and W that are multiples of 32."""
    L = _lib.lib()
    h, w = H, W
    for _name, cin, cout, pool in VGG_LAYERS[1:]:
        if not L.ntk_vgg_wino43_blocked_supported(frames, h, w, cin, cout):
            return False
        if pool:
            h //= 2
            w //= 2
    return True


def conv3x3_relu_wino43_blocked(x, u_packed, bias, cin, cout, fuse_pool=False, out_blocked=True, out=None):
    """conv3x3_relu_wino43 with channel-blocked maps: the input is blocked [F,H,cin/8,W,8] (5-D) or NHWC [F,H,W,cin] (4-D); the
    output blocked [F,Ho,cout/8,Wo,8] or NHWC [F,Ho,Wo,cout].  Same arithmetic and bits as the NHWC call (csrc/conv_wino43.hip)."""
    in_blocked = x.dim() == 5
    err = (("conv3x3_relu_wino43_blocked: input is %s, layer expects %d channels in blocks of 8", tuple(x.shape), cin) if in_blocked
           else ("conv3x3_relu_wino43_blocked: input has %d channels, layer expects %d", _channels(x), cin))
    return _conv("ntk_vgg_conv3x3_relu_wino43_layout_f32", x, "blocked" if in_blocked else "nhwc", "blocked" if out_blocked else "nhwc",
                 u_packed, bias, cin, cout, fuse_pool, out, (1 if in_blocked else 0, 1 if out_blocked else 0), *err)


def nhwc_to_blocked(x):
    """[F,H,W,C] -> [F,H,C/8,W,8] (host-side helper for tests and step-wise callers)."""
    F, H, W, C = x.shape
    return x.view(F, H, W, C // 8, 8).permute(0, 1, 3, 2, 4).contiguous()


def blocked_to_nhwc(x):
    F, H, CB, W, E = x.shape
    return x.permute(0, 1, 3, 2, 4).reshape(F, H, W, CB * E).contiguous()


def conv3x3_relu_bf16(x, w_packed, bias, cin, cout, fuse_pool=False, out_f32=False, out=None):
    """bf16 NHWC activations [F,H,W,Cin] -> relu(conv3x3_same(x)+b) in bf16 (or fp32 when out_f32)."""
    return _conv("ntk_vgg_conv3x3_relu_bf16", x, "bf16", "nhwc" if out_f32 else "bf16", w_packed, bias, cin, cout, fuse_pool, out,
                 (1 if out_f32 else 0,), "conv3x3_relu_bf16: expected bf16 input with %d channels", cin)


def conv3x3_relu_bf16p(x, w_packed, bias, cin, cout, fuse_pool=False, out_f32=False, out=None):
    """conv3x3_relu_bf16 in patch form (csrc/conv_bf16p.hip); w_packed from pack_weights_bf16p for THIS frame shape."""
    return _conv("ntk_vgg_conv3x3_relu_bf16p", x, "bf16", "nhwc" if out_f32 else "bf16", w_packed, bias, cin, cout, fuse_pool, out,
                 (1 if out_f32 else 0,), "conv3x3_relu_bf16p: expected bf16 input with %d channels", cin)


def pack_weights_bf16p(w_hwio, H, W):
    kh, kw, cin, cout = w_hwio.shape
    wp = torch.empty(_lib.lib().ntk_vgg_bf16p_packed_elems(cin, cout), device=w_hwio.device, dtype=torch.bfloat16)
    _lib.check(_lib.lib().ntk_vgg_pack_weights_bf16p(_lib.ptr(w_hwio.contiguous()), _lib.ptr(wp), cin, cout, H, W, _lib.stream()),
               "ntk_vgg_pack_weights_bf16p")
    return wp


# ---- the SPLIT form of the fp32 trunk (csrc/conv_bf16p.hip, template flag X3): every fp32 value travels as two fp16 numbers
def to_split(x):
    """fp32 NHWC [F,H,W,C] (C a multiple of 16) -> split map [F,H,W,C/16,2,16] fp16, as the kernels' epilogues write it
    (csrc/conv_bf16p.hip s3_split4): hi = fp16(x) rounded toward zero (saturating at 65504), lo = fp16(x - hi)."""
    F, H, W, C = x.shape
    t = x.clamp(-65504.0, 65504.0)
    hi = t.to(torch.float16)                                  # round to nearest ...
    over = hi.to(torch.float32).abs() > t.abs()               # ... stepped back where that rounded away from zero
    hi_i = hi.view(torch.int16)
    hi = torch.where(over, hi_i - 1, hi_i).view(torch.float16)    # (sign-magnitude: one ulp toward zero is bits - 1)
    lo = (x - hi.to(torch.float32)).clamp(-65504.0, 65504.0).to(torch.float16)
    return torch.stack((hi.view(F, H, W, C // 16, 16), lo.view(F, H, W, C // 16, 16)), dim=4).contiguous()


def from_split(s):
    """split map -> fp32 NHWC (hi + lo)."""
    F, H, W, G = s.shape[:4]
    return (s[:, :, :, :, 0].to(torch.float32) + s[:, :, :, :, 1].to(torch.float32)).reshape(F, H, W, G * 16)


def split3_supported(H, W, cin, cout, fuse_pool=False):
    return bool(_lib.lib().ntk_vgg_split3_supported(H, W, cin, cout, 1 if fuse_pool else 0))


def pack_weights_split3(w_hwio, H, W):
    kh, kw, cin, cout = w_hwio.shape
    wp = torch.empty(_lib.lib().ntk_vgg_split3_packed_elems(cin, cout), device=w_hwio.device, dtype=torch.float16)
    _lib.check(_lib.lib().ntk_vgg_pack_weights_split3(_lib.ptr(w_hwio.contiguous()), _lib.ptr(wp), cin, cout, H, W, _lib.stream()),
               "ntk_vgg_pack_weights_split3")
    return wp


def split3_stem_supported(H, W, fuse_pool=False):
    """Frame shapes on which conv1_1 can be computed inside conv1_2's staging (conv3x3_relu_split3(..., stem=...))."""
    return bool(_lib.lib().ntk_vgg_split3_stem_supported(H, W, 1 if fuse_pool else 0))


def conv3x3_relu_split3(x, w_packed, bias, cin, cout, fuse_pool=False, out_f32=False, out=None, stem=None):
    """split map [F,H,W,Cin/16,2,16] (or an fp32 NHWC map [F,H,W,Cin]: the kernel's staging splits it; cin <= 64 and cout == 64 only)
    -> relu(conv3x3_same(x) + b) as a split map (or fp32 NHWC when out_f32): the fp32 product x w accumulated as
    xh wh + xh wl + xl wh on the 16-bit matrix pipe (fp16 parts, fp32 accumulators).
    stem = (w1_packed, bias1), conv1_1's weights from pack_weights: x is then the fp32 FRAMES [F,H,W,3] and the layer (conv1_2,
    64 -> 64) computes conv1_1's map on the fly in its staging (csrc/conv_bf16p.hip STEM); that map never reaches memory."""
    if stem is not None:
        if x.dim() != 4 or x.dtype != torch.float32 or x.shape[3] != 3 or (cin, cout) != (64, 64):
            raise _lib.NtkError("conv3x3_relu_split3: the fused stem reads fp32 frames [F,H,W,3] and runs a 64 -> 64 layer")
        F, H, W = x.shape[:3]
        dst = "nhwc" if out_f32 else "split"
        if out is None:
            oh, ow = (H // 2, W // 2) if fuse_pool else (H, W)
            out = torch.empty(_map_shape(dst, F, oh, ow, cout), device=x.device, dtype=_MAP_DTYPE[dst])
        _lib.check(_lib.lib().ntk_vgg_conv3x3_relu_split3_stem(_lib.ptr(x), _lib.ptr(stem[0]), _lib.ptr(stem[1]), _lib.ptr(w_packed),
                                                               _lib.ptr(bias), _lib.ptr(out), F, H, W, 1 if fuse_pool else 0,
                                                               1 if out_f32 else 0, _lib.stream()), "ntk_vgg_conv3x3_relu_split3_stem")
        return out
    in_f32 = x.dtype == torch.float32
    return _conv("ntk_vgg_conv3x3_relu_split3", x, "nhwc" if in_f32 else "split", "nhwc" if out_f32 else "split", w_packed, bias,
                 cin, cout, fuse_pool, out, (1 if in_f32 else 0, 1 if out_f32 else 0),
                 "conv3x3_relu_split3: expected %s of %d channels", "an fp32 NHWC map" if in_f32 else "a split map", cin)


def pack_weights_bf16(w_hwio):
    kh, kw, cin, cout = w_hwio.shape
    wp = torch.empty((cout, 9 * cin), device=w_hwio.device, dtype=torch.bfloat16)
    _lib.check(_lib.lib().ntk_vgg_pack_weights_bf16(_lib.ptr(w_hwio.contiguous()), _lib.ptr(wp), cin, cout, _lib.stream()),
               "ntk_vgg_pack_weights_bf16")
    return wp


# ---- which kernel runs which layer in which activation layout: decided once per frame shape
TrunkStep = namedtuple("TrunkStep", "layer kernel src dst pool window waves")
# TrunkStep.kernel -> the module-level function that launches it (looked up by name when a step runs)
_STEP_FN = {"direct": "conv3x3_relu", "direct_to_bf16": "conv3x3_relu_f32_to_bf16", "wino": "conv3x3_relu_wino",
            "wino43": "conv3x3_relu_wino43", "wino43_blocked": "conv3x3_relu_wino43_blocked", "split3": "conv3x3_relu_split3",
            "bf16": "conv3x3_relu_bf16", "bf16p": "conv3x3_relu_bf16p"}


def trunk_plan(frames_shape, dtype, form, upto="conv4_3", *, layout, wino_waves, features_window, split3_upto, bf16_form,
               stem="separate"):
    """The layers conv1_1 .. `upto` of a [F,H,W,3] chunk as TrunkSteps.  A pure host function: it asks the library's shape
    predicates and touches no device and no weights.  dtype "bf16": the patch form where it takes the layer (bf16_form "patch"), the
    tile form otherwise.  dtype "f32", by `form`:
      "split3"    where the whole trunk can (the eight-wave F(4x4) kernel takes every layer, no window, conv1_2 fits the split form):
                  conv1_1 direct, conv1_2 .. split3_upto in the split form for as long as it takes the layer, the rest on the F(4x4)
                  kernel with channel-blocked maps; elsewhere as "winograd";
      "winograd"  with layout "blocked" where the whole trunk can: F(4x4) with channel-blocked maps between the layers; elsewhere
                  NHWC maps and per layer F(4x4) (carrying wino_waves; features_window on a final conv4_3), F(2x2), direct;
      "winograd2" NHWC, per layer F(2x2), direct;  "direct": NHWC, direct.
    The last step writes fp32 NHWC and is un-pooled when `upto` comes before conv4_3.
    stem "fused": where conv1_2 runs in the split form on conv1_1's fp32 map and the library can compute conv1_1 inside conv1_2's
    staging (ntk_vgg_split3_stem_supported), step 0 writes the marker layout "stem" -- a map that is never materialised: nothing is
    launched for it -- and step 1 reads it: one launch for both layers."""
    F, H, W = frames_shape[:3]
    names = [l[0] for l in VGG_LAYERS]
    layers = VGG_LAYERS[:names.index(upto) + 1]
    steps = []
    if dtype == "bf16":
        if upto != "conv4_3":
            raise _lib.NtkError("bf16 trunk runs to conv4_3 only")
        h, w = H, W
        for name, cin, cout, pool in layers:
            if not steps:
                kernel, src = "direct_to_bf16", "nhwc"
            else:
                patch = bf16_form == "patch" and _lib.lib().ntk_vgg_bf16p_supported(h, w, cin, cout, 1 if pool else 0)
                kernel, src = "bf16p" if patch else "bf16", "bf16"
            steps.append(TrunkStep(name, kernel, src, "nhwc" if name == upto else "bf16", pool, None, None))
            h, w = (h // 2, w // 2) if pool else (h, w)
        return tuple(steps)
    # the whole-trunk routes first: maps between the layers in the workspaces' own layouts, no NHWC layer after conv1_1's output
    whole = upto == "conv4_3" and wino_waves in (None, 8) and features_window is None and blocked_trunk_supported(F, H, W)
    n_split = None                                   # layers after conv1_1 that may run in the split form; None: the NHWC fall-back
    if form == "split3":
        if whole and split3_supported(H, W, 64, 64, True):
            n_split = names.index(split3_upto) if split3_upto in names else 0
        form = "winograd"                            # everything else as the Winograd trunk
    if n_split is None and whole and form == "winograd" and layout == "blocked":
        n_split = 0
    h, w = H, W
    for li, (name, cin, cout, pool) in enumerate(layers):
        last = name == upto
        src = steps[-1].dst if steps else "nhwc"
        pool = pool and not last
        oh, ow = (h // 2, w // 2) if pool else (h, w)
        dst, window, waves = "nhwc", None, None
        if li == 0:
            kernel = "direct"                        # conv1_1: three input channels
        elif n_split is not None:
            if (li <= n_split and src != "blocked" and split3_supported(h, w, cin, cout, pool)
                    and (src == "split" or (cin <= 64 and cout == 64))):     # an fp32 map is read by the four-wave form only (conv1_2)
                kernel = "split3"                    # writes fp32 NHWC when the next layer cannot read a split map
                nxt = None if last else VGG_LAYERS[li + 1]
                if nxt is not None and li + 1 <= n_split and split3_supported(oh, ow, nxt[1], nxt[2], nxt[3]):
                    dst = "split"
            else:
                kernel, dst = "wino43_blocked", "nhwc" if last else "blocked"
        elif form == "winograd" and wino43_supported(cin, cout, h, w, F):
            kernel, waves, window = "wino43", wino_waves, features_window if name == "conv4_3" else None
        elif form in ("winograd", "winograd2") and wino_supported(cin, cout, h, w, F):
            kernel = "wino"
        else:
            kernel = "direct"
        steps.append(TrunkStep(name, kernel, src, dst, pool, window, waves))
        h, w = oh, ow
    if (stem == "fused" and len(steps) > 1 and steps[0].kernel == "direct" and steps[1].kernel == "split3" and steps[1].src == "nhwc"
            and split3_stem_supported(H, W, steps[1].pool)):
        steps[0] = steps[0]._replace(dst="stem")
        steps[1] = steps[1]._replace(src="stem")
    return tuple(steps)


class VGG16Conv43(object):
    """Frozen VGG-16 trunk up to conv4_3/Relu.

    weights: {layer_name: (w_hwio [3,3,Cin,Cout], b [Cout])} as numpy arrays or tensors.
    dtype "f32" (BASELINE configs 2-4: fp32 values and accumulators; `algo` picks the form -- None / "split3": conv1_2 .. conv4_3
    as three fp16 MFMA products per fp32 product of hi / lo parts (DESIGN.md 4.0''; error at or below the Winograd form's;
    an activation is carried to 2^-22 relative from 2^-3 up to 65504, to an absolute 2^-25 below 2^-3 and at fp16's spacing from
    65504 to the clamp at 131008, a weight to 2^-22 relative down to 2^-17 of its layer's largest; conv4_3's fp32 output is not
    clamped: include/ntmtrack.h, tests/test_conv_values_gpu.py),
    "winograd" / "winograd2": fused Winograd on the fp32 MFMA pipe, "direct": the implicit-GEMM kernel; NTK_TRUNK_ALGO overrides
    the default) or "bf16" (config 5: bf16 operands, fp32 accumulate; conv1_1 reads the fp32 frames, conv4_3 writes fp32 for the
    memory cell).
    """

    def __init__(self, weights, device="cuda", chunk_frames=1024, dtype="f32", algo=None):
        self.device = torch.device(device)
        self.chunk_frames = int(chunk_frames)
        if dtype not in ("f32", "bf16"):
            raise _lib.NtkError("VGG16Conv43: dtype must be 'f32' or 'bf16'")
        if algo is None:                                        # the fp32 trunk's default form (NTK_TRUNK_ALGO overrides)
            algo = os.environ.get("NTK_TRUNK_ALGO", "split3")
        if algo not in ("split3", "winograd", "winograd2", "direct"):
            raise _lib.NtkError("VGG16Conv43: algo must be 'split3', 'winograd', 'winograd2' or 'direct'")
        self.dtype = dtype
        # (y0, x0, y1, x1) in conv4_3 output pixels, multiples of 4, or None: compute conv4_3 only there (F(4x4) fp32 trunk).  The
        # tracker's extract_features reads 64 fixed points of the 28x28 map (rows / columns 6..20): window (4, 4, 24, 24) = 25
        # of its 49 tiles.  Positions outside the window keep whatever the buffer held (pass a zeroed `out`).  Off by default:
        # the benchmark computes the whole map, as the reference graph does.
        self.features_window = None
        # parts / streams of a trunk pass (see __call__): two for the default F(4x4) fp32 trunk; measured a loss for the direct
        # kernels (149 -> 173 ms per step) and for round 2's bf16 tile kernel (59.5 -> 59.9), no change for F(2x2); the bf16 patch-form
        # kernel (one workgroup per CU, like the F(4x4) kernel) gains 2 % (640 frames: 18.07 -> 17.67 ms)
        self.split_streams = int(os.environ.get("NTK_TRUNK_SPLIT", "2" if ((dtype == "f32" and algo in ("winograd", "split3")) or dtype == "bf16") else "1"))
        self._side = []
        # fp32 trunk: "winograd" = fused Winograd F(4x4,3x3) wherever the layer shape allows (conv1_2 .. conv4_3 on
        # 224x224 frames; 4x fewer multiplies than the direct form, error ~1e-5 of the activation scale per layer),
        # "winograd2" = fused Winograd F(2x2,3x3) (2.25x fewer multiplies, error ~3e-7 per layer); the direct
        # implicit-GEMM kernel runs where neither applies (conv1_1, odd frame sizes) and everywhere with "direct"
        # "split3" = the SPLIT form (csrc/conv_bf16p.hip X3: every fp32 product as three fp16 MFMA products of hi / lo parts, fp32
        # accumulators) on conv1_2 .. split3_upto,
        # the F(4x4) Winograd kernel on the layers after it (on the 28 x 28 maps of conv4_x the two are within 2 %).  conv1_1 is computed
        # inside conv1_2's staging (self.stem below; as its own fp32 kernel, whose map conv1_2's staging splits, with "separate"), the
        # last split layer writes fp32 NHWC for the Winograd layers.
        self.split3 = (algo == "split3" and dtype == "f32")
        self.split3_upto = os.environ.get("NTK_SPLIT3_UPTO", "conv4_3")
        # "fused": conv1_1 is computed inside conv1_2's staging wherever the split trunk runs (no 12.8 MB / frame stem map, one launch
        # less); "separate": conv1_1 as its own fp32 kernel (the form before; for A/B runs: NTK_TRUNK_STEM=separate)
        self.stem = os.environ.get("NTK_TRUNK_STEM", "fused")
        if self.stem not in ("fused", "separate"):
            raise _lib.NtkError("VGG16Conv43: NTK_TRUNK_STEM must be 'fused' or 'separate'")
        # __call__(..., latency=True) runs a call of fewer frames than this in the Winograd form: with a handful of frames a layer is
        # a few workgroups per CU at most and the pass is bound by one workgroup's critical path, which is shorter in the F(4x4)
        # kernel (224 x 224, one MI355X: 1 frame 0.78 against 0.96 ms, 8 frames 1.00 against 1.09, 12 frames 1.39 against 1.27,
        # 16 frames 1.57 against 1.44 -- scripts/r04/small_batch_trunk.py).  What the online tracker asks for (one frame per call).
        # Without the flag every call runs the same form, so a frame's features do not depend on the size of the batch it is in
        # (bit for bit: tests/test_fullsize_gpu.py).
        self.split3_latency_frames = 12
        self._packed_split3 = {}
        self._plans = {}
        self.last_plan = None                                   # the plan of the chunk that ran last
        if self.split3:
            algo = "winograd"                                # everything else (weights packed, layouts, fallbacks) as the Winograd trunk
        self.algo = algo
        # form of the F(4x4) kernel: None = the library's default (eight waves per workgroup); 4 = round 2's one-wave-per-SIMD kernel
        self.wino_waves = None
        # activation layout BETWEEN the layers of the F(4x4) fp32 trunk: "blocked" = [H][C/8][W][8] (a K step's eight channels
        # contiguous per pixel, blocks interleaved per image row: the patch staging reads whole cache lines), "nhwc" = round 3's.
        # Blocked is the default wherever the eight-wave kernel takes every layer (blocked_trunk_supported); frames, conv1_1's
        # output and conv4_3's output are NHWC either way; same bits.
        self.layout = os.environ.get("NTK_TRUNK_LAYOUT", "blocked")
        self._blocked_ws = {}
        self.packed = {}
        self._w_hwio = {}
        self._packed_bf16p = {}
        # bf16 trunk: "patch" = csrc/conv_bf16p.hip wherever it takes the layer shape (round 4), "tile" = round 2's kernel
        self.bf16_form = os.environ.get("NTK_BF16_FORM", "patch")
        self.packed_wino = {}
        self.packed_wino43 = {}
        for name, cin, cout, _pool in VGG_LAYERS:
            w, b = weights[name]
            w = torch.as_tensor(w, dtype=torch.float32).to(self.device)
            b = torch.as_tensor(b, dtype=torch.float32).to(self.device).contiguous()
            if tuple(w.shape) != (3, 3, cin, cout):
                raise _lib.NtkError("%s: weight shape %s != (3,3,%d,%d)" % (name, tuple(w.shape), cin, cout))
            if self.split3 and dtype == "f32" and cin % 16 == 0:
                self._w_hwio[name] = w                     # packed per frame shape on first use
            if dtype == "bf16" and cin % 64 == 0:
                self.packed[name] = (pack_weights_bf16(w), b)
                self._w_hwio[name] = w                     # the patch-form kernel packs per frame shape, on first use
            else:
                self.packed[name] = (pack_weights(w), b)
                if dtype == "f32" and algo in ("winograd", "winograd2") and cin % 16 == 0:
                    self.packed_wino[name] = pack_weights_wino(w)
                    if algo == "winograd":
                        self.packed_wino43[name] = pack_weights_wino43(w)

    def _trunk_ws(self, frames, plan):
        """Where every step of `plan` but the last writes: two ping-pong workspaces per (stream, chunk shape) for the maps between the
        layers, allocated once -- a training loop then makes no allocator calls in its trunk passes -- and viewed once per plan in each
        step's layout.  The largest map, conv1_1's, is 12.8 MB per frame; a split or bf16 map has at most the bytes of its layer's
        fp32 map."""
        F, H, W, _ = frames.shape
        fused = plan[0].dst == "stem"                             # no stem map: the largest map left is conv2_1's, half its bytes
        key = (torch.cuda.current_stream(frames.device).cuda_stream, F, H, W, fused)
        if key not in self._blocked_ws:
            if len(self._blocked_ws) >= 8:                        # shapes come and go (tests, online tracking): keep the table small
                self._blocked_ws.clear()
            ws = (torch.empty(F * H * W * (32 if fused else 64), device=frames.device),
                  torch.empty(F * (H // 2) * (W // 2) * 64, device=frames.device))
            self._blocked_ws[key] = (ws, {})
        ws, views = self._blocked_ws[key]
        if plan not in views:
            if len(views) >= 8:
                views.clear()
            dsts, h, w = [], H, W
            for i, (step, (_name, _cin, cout, _pool)) in enumerate(zip(plan[:-1], VGG_LAYERS)):
                h, w = (h // 2, w // 2) if step.pool else (h, w)
                if step.dst == "stem":
                    dsts.append(None)
                    continue
                shape = _map_shape(step.dst, F, h, w, cout)
                dsts.append(ws[i & 1].view(_MAP_DTYPE[step.dst])[:math.prod(shape)].view(shape))
            views[plan] = dsts
        return views[plan]

    def split3_trunk_supported(self, frames_shape):
        F, H, W = frames_shape[:3]
        return (self.wino_waves in (None, 8) and self.features_window is None and blocked_trunk_supported(F, H, W)
                and split3_supported(H, W, 64, 64, True))

    def plan(self, frames_shape, upto="conv4_3", form=None):
        """trunk_plan of this trunk as it is configured NOW (layout, wino_waves, features_window, ... may be assigned at any time), cached
        per argument set.  form: None = the trunk's own ("split3" while self.split3, else self.algo); a split trunk also runs "winograd"."""
        own = "split3" if self.split3 else self.algo
        if form is None:
            form = own
        elif form != own and not (form == "winograd" and self.algo == "winograd"):
            raise _lib.NtkError("VGG16Conv43: this %s trunk has no weights packed for form=%r" % (own, form))
        win = self.features_window
        key = (tuple(frames_shape[:3]), self.dtype, form, upto, self.layout, self.wino_waves, None if win is None else tuple(win),
               self.split3_upto, self.bf16_form, self.stem)
        plan = self._plans.get(key)
        if plan is None:
            if len(self._plans) >= 8:
                self._plans.clear()
            plan = self._plans[key] = trunk_plan(key[0], *key[1:4], layout=key[4], wino_waves=key[5], features_window=key[6],
                                                 split3_upto=key[7], bf16_form=key[8], stem=key[9])
        return plan

    def _step_weights(self, step, h, w, device):
        name = step.layer
        if step.kernel in ("split3", "bf16p"):                   # packed per frame shape, on first use
            cache, pack, key = ((self._packed_split3, pack_weights_split3, (name, h, w)) if step.kernel == "split3"
                                else (self._packed_bf16p, pack_weights_bf16p, (name, h % 8 == 0 and w % 8 == 0)))
            if key not in cache:
                cache[key] = pack(self._w_hwio[name], h, w)
                torch.cuda.current_stream(device).synchronize()    # packed once, read from every stream a pass runs on
            return cache[key]
        if step.kernel in ("wino43", "wino43_blocked"):
            return self.packed_wino43[name]
        return self.packed_wino[name] if step.kernel == "wino" else self.packed[name][0]

    def forward_chunk(self, frames, upto="conv4_3", out=None, form=None):
        """Plan and run one chunk: one loop for every form.  The last step writes `out` (allocated when None: zeroed under a window,
        which leaves the rest untouched); every other map lives in one of the two ping-pong workspaces, viewed in the step's layout."""
        frames = frames.contiguous()
        F, h, w, _ = frames.shape
        plan = self.last_plan = self.plan(frames.shape, upto, form)
        launch = globals()                         # the conv functions by name at call time: tests count launches by patching them
        dsts = self._trunk_ws(frames, plan) if len(plan) > 1 else []
        x = frames
        for i, (step, (name, cin, cout, _pool)) in enumerate(zip(plan, VGG_LAYERS)):
            if i < len(dsts):
                dst = dsts[i]
            elif out is None and step.window is not None:
                dst = torch.zeros((F, h, w, cout), device=frames.device, dtype=torch.float32)
            else:
                dst = out
            if step.dst == "stem":                                # conv1_1 runs inside the next step's launch
                continue
            kw = {} if step.kernel == "direct_to_bf16" else {"fuse_pool": step.pool}
            if step.src == "stem":
                kw["stem"] = self.packed["conv1_1"]
            if step.kernel == "wino43":
                kw.update(window=step.window, waves=step.waves)
            elif step.kernel == "wino43_blocked":
                kw["out_blocked"] = step.dst == "blocked"
            elif step.kernel in ("split3", "bf16", "bf16p"):
                kw["out_f32"] = step.dst == "nhwc"
            x = launch[_STEP_FN[step.kernel]](x, self._step_weights(step, h, w, frames.device), self.packed[name][1], cin, cout,
                                              out=dst, **kw)
            h, w = (h // 2, w // 2) if step.pool else (h, w)
        return x

    def __call__(self, frames, out=None, latency=False, form=None):
        """frames [F,H,W,3] mean-subtracted fp32 NHWC, H and W multiples of 32 (the reference's frames: 224 x 224) -> [F,H/8,W/8,512].
        Frames with other sides are refused before anything is launched: conv4_x runs on H/8 x W/8 maps, and every conv form needs
        sides that are multiples of 4.  form: run THIS call in that form instead of the trunk's own (see plan()).  latency=True: a call
        of a few frames may run the form with the shorter critical path (split3_latency_frames) -- same operator, results equal to fp32
        rounding, not bit for bit."""
        if frames.dim() != 4 or frames.shape[3] != 3:
            raise _lib.NtkError("frames must be [F,H,W,3] NHWC")
        F, H, W, _ = frames.shape
        if H < 32 or W < 32 or H % 32 or W % 32:
            raise _lib.NtkError("frames of %d x %d: H and W must be multiples of 32 (conv4_x runs on H/8 x W/8 maps, whose sides "
                                "every conv form needs to be multiples of 4)" % (H, W))
        if out is None:
            # with a features_window the window kernel leaves everything outside the window untouched: the map a caller
            # gets back must be zero there, not uninitialised memory
            alloc = torch.zeros if getattr(self, "features_window", None) is not None else torch.empty
            out = alloc((F, H // 8, W // 8, 512), device=frames.device, dtype=torch.float32)
        if form is None and latency and F < self.split3_latency_frames and self.split3:
            form = "winograd"
        return self._run_chunks(frames, out, form)

    def _run_chunks(self, frames, out, form=None):
        F = frames.shape[0]
        for f0 in range(0, F, self.chunk_frames):
            f1 = min(F, f0 + self.chunk_frames)
            n = self.split_streams if (f1 - f0) >= 32 * self.split_streams else 1
            if n <= 1:
                self.forward_chunk(frames[f0:f1], out=out[f0:f1], form=form)
                continue
            # the chunk in n parts on n streams: the kernels of the parts fill each other's launch tails (a layer's last
            # workgroups leave CUs idle until the next launch; frames are independent, the layers of one frame are not).
            # Measured, 640 frames: one stream 55.4 ms, two 54.5, three 54.4; whole step 64.45 -> 63.65 ms with two.
            cur = torch.cuda.current_stream(frames.device)
            while len(self._side) < n - 1:
                self._side.append(torch.cuda.Stream(device=frames.device, priority=cur.priority))
            cuts = [f0 + (f1 - f0) * i // n for i in range(n + 1)]
            for i in range(1, n):
                self._side[i - 1].wait_stream(cur)
                with torch.cuda.stream(self._side[i - 1]):
                    self.forward_chunk(frames[cuts[i]:cuts[i + 1]], out=out[cuts[i]:cuts[i + 1]], form=form)
            self.forward_chunk(frames[cuts[0]:cuts[1]], out=out[cuts[0]:cuts[1]], form=form)
            for i in range(1, n):
                cur.wait_stream(self._side[i - 1])
        return out
