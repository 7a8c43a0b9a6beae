"""CPU: every conv form's shape predicate agrees with its launcher, over a grid of layer shapes.

The trunk picks a conv kernel per layer by asking a predicate (ntk_vgg_split3_supported, ntk_vgg_split3_stem_supported, ntk_vgg_bf16p_supported, and through
vgg.wino_supported / vgg.wino43_supported ntk_vgg_wino_supported / ntk_vgg_wino43_supported; ntk_vgg_wino43_blocked_supported for
channel-blocked maps); the entry then picks an instantiation by its own logic.  Here every entry is called with fake pointers
(non-null, 16-byte aligned, never dereferenced): a shape its predicate accepts must pass every host-side check and reach the launch,
which fails without a device (NTK_ERR_HIP); a shape the predicate refuses must be refused before that (NTK_ERR_BAD_SHAPE /
NTK_ERR_UNSUPPORTED).  With a device present a wrongly accepted shape would launch against the fake pointers, so the file runs only
where there is none.  tests/test_conv_shapes_gpu.py runs the accepted shapes on the GPU."""
import ctypes
import itertools

import pytest
import torch

pytestmark = pytest.mark.skipif(torch.cuda.is_available(), reason="fake pointers: runs only where no device is visible")

NTK_ERR_BAD_SHAPE, NTK_ERR_BAD_PTR, NTK_ERR_UNSUPPORTED, NTK_ERR_HIP = -1, -2, -3, -4
FRAMES = 2
SIDES = (4, 8, 12, 16, 20, 24, 28, 32, 40, 56)
# out of range: sides that are not multiples of 4, zero sides, 28-wide maps too short for runs of rows (H < 20 is also in SIDES)
ODD = ((6, 8), (8, 6), (10, 28), (18, 28), (28, 26), (0, 8), (8, 0), (0, 28), (0, 0))
GEOMETRY = [(h, w) for h in SIDES for w in SIDES] + list(ODD)
CHANNELS = ((16, 64), (32, 64), (48, 64), (64, 64), (32, 128), (64, 128), (128, 256), (256, 512), (512, 512),
            (64, 192), (64, 1024), (1040, 64),
            (0, 64), (64, 0))               # no channels (cout = 0 once divided by zero in the split and patch forms' predicates)
P = ctypes.c_void_p(1 << 20)


def _lib():
    from ntmtrack import _lib
    return _lib.lib()


def _layers():
    return itertools.product(GEOMETRY, CHANNELS, (0, 1))


class _Sweep(object):
    """Collects every disagreement between a predicate and an entry; the failure lists them all."""

    def __init__(self, entry):
        self.entry, self.n, self.bad = entry, 0, []

    def check(self, accepted, rc, **shape):
        self.n += 1
        what = " ".join("%s=%d" % kv for kv in shape.items())
        if accepted and rc != NTK_ERR_HIP:
            msg = _lib().ntk_last_error()
            self.bad.append("%s: the predicate accepts it, the entry returned %d (%s)" % (what, rc, msg.decode() if msg else ""))
        elif not accepted and rc not in (NTK_ERR_BAD_SHAPE, NTK_ERR_UNSUPPORTED):
            self.bad.append("%s: the predicate refuses it, the entry returned %d" % (what, rc))

    def verdict(self):
        assert self.n > 0
        assert not self.bad, "%s: %d of %d calls disagree with the predicate:\n  %s" % (self.entry, len(self.bad), self.n,
                                                                                         "\n  ".join(self.bad))


def test_split3_entries_agree_with_their_predicate():
    """ntk_vgg_conv3x3_relu_split3 in every in / out variant and ntk_vgg_pack_weights_split3 take exactly the shapes
    ntk_vgg_split3_supported accepts (an fp32 input map: those of the four-wave form only, cin <= 64, cout = 64, H and W multiples
    of 8)."""
    from ntmtrack import vgg
    L = _lib()
    conv, pack = _Sweep("ntk_vgg_conv3x3_relu_split3"), _Sweep("ntk_vgg_pack_weights_split3")
    for (H, W), (cin, cout), pool in _layers():
        ok = vgg.split3_supported(H, W, cin, cout, pool)
        four_waves = ok and cin <= 64 and cout == 64 and H % 8 == 0 and W % 8 == 0
        for in_f32, out_f32 in ((0, 0), (0, 1), (1, 0), (1, 1)):
            rc = L.ntk_vgg_conv3x3_relu_split3(P, P, P, P, FRAMES, H, W, cin, cout, pool, in_f32, out_f32, None)
            conv.check(four_waves if in_f32 else ok, rc, H=H, W=W, cin=cin, cout=cout, pool=pool, in_f32=in_f32, out_f32=out_f32)
        if not pool:
            pack.check(ok, L.ntk_vgg_pack_weights_split3(P, P, cin, cout, H, W, None), H=H, W=W, cin=cin, cout=cout)
    conv.verdict()
    pack.verdict()


def test_split3_stem_entry_agrees_with_its_predicate():
    """The fused stem (ntk_vgg_conv3x3_relu_split3_stem: conv1_1 inside conv1_2's staging) takes exactly the frame shapes
    ntk_vgg_split3_stem_supported accepts -- those of the four-wave split form at 64 -> 64 channels: H and W multiples of 8 -- with
    either output; its pixel offsets are 32-bit, its 16-byte accesses (packed conv1_2 weights, output) need aligned pointers, and the
    frames, which it reads float by float, do not."""
    from ntmtrack import vgg
    L = _lib()
    conv, accepted = _Sweep("ntk_vgg_conv3x3_relu_split3_stem"), 0
    for H, W in GEOMETRY:
        for pool in (0, 1):
            ok = bool(L.ntk_vgg_split3_stem_supported(H, W, pool))
            assert ok == (vgg.split3_supported(H, W, 64, 64, pool) and H % 8 == 0 and W % 8 == 0), (H, W, pool)
            assert ok == vgg.split3_stem_supported(H, W, bool(pool)), (H, W, pool)
            accepted += ok
            for out_f32 in (0, 1):
                rc = L.ntk_vgg_conv3x3_relu_split3_stem(P, P, P, P, P, P, FRAMES, H, W, pool, out_f32, None)
                conv.check(ok, rc, H=H, W=W, pool=pool, out_f32=out_f32)
    conv.verdict()
    assert accepted == 72, accepted                  # the 36 maps whose sides are multiples of 8, pooled or not
    stem = lambda frames=FRAMES, x=P, w2=P, out=P: L.ntk_vgg_conv3x3_relu_split3_stem(x, P, P, w2, P, out, frames, 8, 8, 0, 1, None)
    assert stem() == NTK_ERR_HIP
    assert stem(frames=1 << 25) == NTK_ERR_UNSUPPORTED          # 2^31 pixels: one more than a 32-bit pixel offset reaches
    assert stem(frames=(1 << 25) - 1) == NTK_ERR_HIP
    assert stem(frames=0) in (NTK_ERR_BAD_SHAPE, NTK_ERR_UNSUPPORTED) and stem(frames=-1) in (NTK_ERR_BAD_SHAPE, NTK_ERR_UNSUPPORTED)
    at8 = ctypes.c_void_p(P.value + 8)               # 8-byte aligned, not 16
    assert stem(w2=at8) == NTK_ERR_BAD_PTR and stem(out=at8) == NTK_ERR_BAD_PTR
    assert stem(x=ctypes.c_void_p(P.value + 4)) == NTK_ERR_HIP  # the frames: 4-byte alignment is enough
    assert stem(x=ctypes.c_void_p(P.value + 2)) == NTK_ERR_BAD_PTR and stem(x=None) == NTK_ERR_BAD_PTR


def test_bf16p_entries_agree_with_their_predicate():
    L = _lib()
    conv, pack = _Sweep("ntk_vgg_conv3x3_relu_bf16p"), _Sweep("ntk_vgg_pack_weights_bf16p")
    for (H, W), (cin, cout), pool in _layers():
        ok = bool(L.ntk_vgg_bf16p_supported(H, W, cin, cout, pool))
        for out_f32 in (0, 1):
            rc = L.ntk_vgg_conv3x3_relu_bf16p(P, P, P, P, FRAMES, H, W, cin, cout, pool, out_f32, None)
            conv.check(ok, rc, H=H, W=W, cin=cin, cout=cout, pool=pool, out_f32=out_f32)
        if not pool:
            pack.check(ok, L.ntk_vgg_pack_weights_bf16p(P, P, cin, cout, H, W, None), H=H, W=W, cin=cin, cout=cout)
    conv.verdict()
    pack.verdict()


def test_winograd_f2_entry_agrees_with_its_predicate():
    from ntmtrack import vgg
    L = _lib()
    conv = _Sweep("ntk_vgg_conv3x3_relu_wino_f32")
    for (H, W), (cin, cout), pool in _layers():
        rc = L.ntk_vgg_conv3x3_relu_wino_f32(P, P, P, P, FRAMES, H, W, cin, cout, pool, None)
        conv.check(vgg.wino_supported(cin, cout, H, W, FRAMES), rc, H=H, W=W, cin=cin, cout=cout, pool=pool)
    conv.verdict()


def test_winograd_f4_entries_agree_with_their_predicate():
    """ntk_vgg_conv3x3_relu_wino43_form_f32 on four and on eight waves over the whole frame, and the channel-blocked entry
    ntk_vgg_conv3x3_relu_wino43_layout_f32 (eight waves) against its own predicate ntk_vgg_wino43_blocked_supported.  Every layer
    of the grid is within the eight-wave kernel's reach (where it cuts a frame into single tiles, a block's input spans less than
    16 MB), so the blocked predicate and entry must take what the whole-frame predicate takes."""
    from ntmtrack import vgg
    L = _lib()
    form, layout = _Sweep("ntk_vgg_conv3x3_relu_wino43_form_f32"), _Sweep("ntk_vgg_conv3x3_relu_wino43_layout_f32")
    for (H, W), (cin, cout), pool in _layers():
        ok = vgg.wino43_supported(cin, cout, H, W, FRAMES)
        blocked = bool(L.ntk_vgg_wino43_blocked_supported(FRAMES, H, W, cin, cout))
        assert blocked == ok, (H, W, cin, cout)
        for waves in (4, 8):
            rc = L.ntk_vgg_conv3x3_relu_wino43_form_f32(P, P, P, P, FRAMES, H, W, cin, cout, pool, 0, 0, H, W, waves, None)
            form.check(ok, rc, H=H, W=W, cin=cin, cout=cout, pool=pool, waves=waves)
        for in_blocked, out_blocked in ((1, 1), (1, 0), (0, 1)):
            rc = L.ntk_vgg_conv3x3_relu_wino43_layout_f32(P, P, P, P, FRAMES, H, W, cin, cout, pool, in_blocked, out_blocked, None)
            layout.check(blocked, rc, H=H, W=W, cin=cin, cout=cout, pool=pool, in_blocked=in_blocked, out_blocked=out_blocked)
    form.verdict()
    layout.verdict()
    # beyond the grid: a frame the kernel cuts into single tiles whose blocks of 32 span more than 16 MB (conv4_2 of a 480 x 640 frame)
    assert L.ntk_vgg_wino43_supported(1, 60, 80, 512, 512) and not L.ntk_vgg_wino43_blocked_supported(1, 60, 80, 512, 512)
    for in_blocked, out_blocked, want in ((1, 1, NTK_ERR_UNSUPPORTED), (0, 1, NTK_ERR_UNSUPPORTED), (0, 0, NTK_ERR_HIP)):
        assert L.ntk_vgg_conv3x3_relu_wino43_layout_f32(P, P, P, P, 1, 60, 80, 512, 512, 0, in_blocked, out_blocked, None) == want


def test_packed_weight_sizes_are_pinned():
    """What a caller allocates for the packed weights.  The split form's image is followed by a 16-byte tail (8 fp16 elements) that
    ntk_vgg_pack_weights_split3 writes its power-of-two scales into: a buffer of 18 cin cout elements is 16 bytes short."""
    L = _lib()
    for cin, cout in CHANNELS + ((3, 64),):
        assert L.ntk_vgg_split3_packed_elems(cin, cout) == 18 * cin * cout + 8
        assert L.ntk_vgg_bf16p_packed_elems(cin, cout) == 9 * cin * cout
        assert L.ntk_vgg_wino_packed_floats(cin, cout) == 16 * cin * cout
        assert L.ntk_vgg_wino43_packed_floats(cin, cout) == 36 * cin * cout
