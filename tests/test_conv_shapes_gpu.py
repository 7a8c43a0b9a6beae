"""GPU: every conv form on every layer shape its predicate accepts, against a float64 convolution of the same operands.

tests/test_conv_shapes_cabi.py holds each form's predicate to its launcher without a device; here the shapes a predicate accepts run,
and no others.  The geometry grid takes H, W in SIDES with and without the fused pool on three frames (sub-blocks, tile blocks and
runs of rows then cross frame boundaries), on the cheap channel pairs that select each form's internal variants; the channel grid
takes every channel pair of the CPU sweep on an 8 x 8 pooled map and on the 20 / 24 / 28 x 28 maps of conv4_x.  The bounds are the
per-form bounds of tests/test_vgg_gpu.py.  A sweep lists every failing shape in one message."""
import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O
from oracle import ntm_oracle_torch as OT

pytestmark = pytest.mark.gpu

F = 3
SIDES = (4, 8, 12, 16, 20, 24, 28, 32, 40, 56)
CHANNELS = ((16, 64), (32, 64), (48, 64), (64, 64), (32, 128), (64, 128), (128, 256), (256, 512), (512, 512),
            (64, 192), (64, 1024), (1040, 64))
CHANNEL_MAPS = ((8, 8, True), (20, 28, False), (24, 28, False), (28, 28, False))
FORMS = ("split3", "bf16p", "bf16", "wino43", "wino", "direct")
# Geometry grid: the forms each cheap channel pair runs, and how many of the grid's 200 (H, W, pool) each one's predicate takes.
# split3: the 36 maps whose sides are multiples of 8, pooled or not, and the six 28-wide maps of at least 20 rows, un-pooled; the
# bf16 patch form: every map un-pooled and the 36 with the pool; the others: all 200.
GEOMETRY_FORMS = {
    (64, 64): {"split3": 78, "bf16p": 136, "bf16": 200},     # split form on four waves (fp32 input too), eight on 28-wide maps
    (32, 128): {"split3": 78, "bf16p": 136},                  # eight waves, 128 columns per block
    (32, 64): {"wino43": 200, "wino": 200, "direct": 200},
    (16, 128): {"wino43": 200},
    (3, 64): {"direct": 200},                                 # conv1_1: its row kernel where W % 32 == 0 without the pool
}


class _Weights(object):
    """A layer's He-scaled weights and nonzero biases on the device, and the packings that do not depend on the frame shape."""

    def __init__(self, cuda, cin, cout):
        rng = np.random.default_rng([cin, cout])
        self.cuda, self.cin, self.cout = cuda, cin, cout
        self.w = (rng.standard_normal((3, 3, cin, cout)) * np.sqrt(2.0 / (9 * cin))).astype(np.float32)
        self.b = (rng.standard_normal(cout) * 0.1).astype(np.float32)
        self.wt, self.bt = torch.from_numpy(self.w).to(cuda), torch.from_numpy(self.b).to(cuda)
        self._packed = {}

    def packed(self, form):
        from ntmtrack import vgg
        if form not in self._packed:
            pack = {"direct": vgg.pack_weights, "bf16": vgg.pack_weights_bf16, "wino": vgg.pack_weights_wino,
                    "wino43": vgg.pack_weights_wino43}[form]
            self._packed[form] = pack(self.wt)
        return self._packed[form]


class _Maps(object):
    """F frames of H x W input (post-ReLU-like; rounded to bf16 for the bf16 forms) and its float64 outputs, computed once and
    shared by every form that reads the same input (the pooled output is the 2x2 max of the un-pooled one)."""

    def __init__(self, wts, H, W):
        rng = np.random.default_rng([H, W, wts.cin, wts.cout])
        self.wts, self.H, self.W = wts, H, W
        self.x = (np.maximum(rng.standard_normal((F, H, W, wts.cin)), 0) * 3).astype(np.float32)
        self.xt = torch.from_numpy(self.x).to(wts.cuda)
        self.xb = torch.from_numpy(O.bf16_round(self.x)).to(wts.cuda).to(torch.bfloat16)       # exact: the values are bf16 already
        self._ref = {}

    def ref(self, pool, bf16=False):
        if bf16 not in self._ref:
            x, w = (O.bf16_round(self.x), O.bf16_round(self.wts.w)) if bf16 else (self.x, self.wts.w)
            self._ref[bf16] = OT.conv3x3_same_relu(x, w, self.wts.b)
        return O.maxpool2x2(self._ref[bf16]) if pool else self._ref[bf16]


class _Checks(object):
    def __init__(self):
        self.n, self.bad, self.worst = 0, [], {}

    def close(self, what, shape, got, ref, bound, bf16_out=False):
        """max |got - ref| / max |ref| below the bound; a bf16 output: |got - ref| / (|ref| + 1e-3 max |ref|) (one bf16 rounding)"""
        self.n += 1
        got = got.float().cpu().numpy()
        if got.shape != ref.shape:
            self.bad.append("%s %s: output %s, expected %s" % (what, shape, got.shape, ref.shape))
            return
        scale, d = float(np.max(np.abs(ref))), np.abs(got - ref)
        err = float(np.max(d / (np.abs(ref) + 1e-3 * scale))) if bf16_out else float(np.max(d)) / scale
        self.worst[what] = max(self.worst.get(what, 0.0), err)
        if not err < bound:
            self.bad.append("%s %s: error %.3e, bound %.1e" % (what, shape, err, bound))

    def same(self, what, shape, a, b):
        self.n += 1
        if not torch.equal(a, b):
            self.bad.append("%s %s: not bit for bit" % (what, shape))

    def verdict(self, name):
        print("%s: %d checks, worst errors %s" % (name, self.n, ", ".join("%s %.2e" % kv for kv in sorted(self.worst.items()))))
        assert self.n > 0, name
        assert not self.bad, "%s: %d of %d checks failed:\n  %s" % (name, len(self.bad), self.n, "\n  ".join(self.bad))


def _accepts(form, H, W, cin, cout, pool):
    """The predicate that decides whether `form` takes a layer (the bf16 tile and the direct kernel have none of their own: their
    shape rules in include/ntmtrack.h)."""
    from ntmtrack import vgg, _lib
    if form == "split3":
        return vgg.split3_supported(H, W, cin, cout, pool)
    if form == "bf16p":
        return bool(_lib.lib().ntk_vgg_bf16p_supported(H, W, cin, cout, 1 if pool else 0))
    if form == "wino43":
        return vgg.wino43_supported(cin, cout, H, W, F)
    if form == "wino":
        return vgg.wino_supported(cin, cout, H, W, F)
    if not (H % 4 == 0 and W % 4 == 0 and cout % 64 == 0):
        return False
    return cin % 64 == 0 if form == "bf16" else (cin == 3 or cin % 32 == 0)


def _run(form, c, m, pool):
    """Every variant of `form` on one layer, checked against the float64 output and against each other."""
    from ntmtrack import vgg
    wts, H, W = m.wts, m.H, m.W
    cin, cout, b = wts.cin, wts.cout, wts.bt
    shape = "F=%d H=%d W=%d cin=%d cout=%d pool=%d" % (F, H, W, cin, cout, pool)
    if form == "split3":
        wp = vgg.pack_weights_split3(wts.wt, H, W)
        xs = vgg.to_split(m.xt)
        ys = vgg.conv3x3_relu_split3(xs, wp, b, cin, cout, fuse_pool=pool)
        yf = vgg.conv3x3_relu_split3(xs, wp, b, cin, cout, fuse_pool=pool, out_f32=True)
        c.close("split3", shape, vgg.from_split(ys), m.ref(pool), 4e-6)
        c.close("split3 out_f32", shape, yf, m.ref(pool), 4e-6)
        c.same("split3 split map vs to_split(its fp32 map)", shape, ys, vgg.to_split(yf))
        if cin <= 64 and cout == 64 and H % 8 == 0 and W % 8 == 0:           # four waves: an fp32 input map, split by the staging
            c.same("split3 in_f32", shape, vgg.conv3x3_relu_split3(m.xt, wp, b, cin, cout, fuse_pool=pool), ys)
            c.same("split3 in_f32 out_f32", shape, vgg.conv3x3_relu_split3(m.xt, wp, b, cin, cout, fuse_pool=pool, out_f32=True), yf)
    elif form in ("bf16p", "bf16"):
        wp = vgg.pack_weights_bf16p(wts.wt, H, W) if form == "bf16p" else wts.packed("bf16")
        conv = vgg.conv3x3_relu_bf16p if form == "bf16p" else vgg.conv3x3_relu_bf16
        for out_f32 in (False, True):
            y = conv(m.xb, wp, b, cin, cout, fuse_pool=pool, out_f32=out_f32)
            c.close(form + (" out_f32" if out_f32 else ""), shape, y, m.ref(pool, bf16=True), 1e-5 if out_f32 else 2.0 ** -8,
                    bf16_out=not out_f32)
    elif form == "wino43":
        u = wts.packed("wino43")
        y = vgg.conv3x3_relu_wino43(m.xt, u, b, cin, cout, fuse_pool=pool, waves=8)
        c.close("wino43", shape, y, m.ref(pool), 3e-5)
        c.same("wino43 four waves", shape, vgg.conv3x3_relu_wino43(m.xt, u, b, cin, cout, fuse_pool=pool, waves=4), y)
        # channel-blocked maps (eight waves: every layer here is within its reach) change addresses only
        yb = vgg.conv3x3_relu_wino43_blocked(vgg.nhwc_to_blocked(m.xt), u, b, cin, cout, fuse_pool=pool, out_blocked=True)
        c.same("wino43 blocked", shape, vgg.blocked_to_nhwc(yb), y)
    elif form == "wino":
        c.close("wino", shape, vgg.conv3x3_relu_wino(m.xt, wts.packed("wino"), b, cin, cout, fuse_pool=pool), m.ref(pool), 1e-5)
    else:
        c.close("direct", shape, vgg.conv3x3_relu(m.xt, wts.packed("direct"), b, cin, cout, fuse_pool=pool), m.ref(pool), 1e-5)


def _run_checked(form, c, m, pool):
    from ntmtrack import _lib
    try:
        _run(form, c, m, pool)
    except _lib.NtkError as e:                   # a shape the predicate accepts that the entry refuses
        c.bad.append("%s F=%d H=%d W=%d cin=%d cout=%d pool=%d: %s" % (form, F, m.H, m.W, m.wts.cin, m.wts.cout, pool, e))


@pytest.mark.parametrize("cin,cout", sorted(GEOMETRY_FORMS))
def test_every_accepted_geometry_matches_float64(cuda, cin, cout):
    forms = GEOMETRY_FORMS[(cin, cout)]
    wts, c, ran = _Weights(cuda, cin, cout), _Checks(), dict.fromkeys(forms, 0)
    for H in SIDES:
        for W in SIDES:
            m = _Maps(wts, H, W)
            for pool in (False, True):
                for form in forms:
                    if _accepts(form, H, W, cin, cout, pool):
                        ran[form] += 1
                        _run_checked(form, c, m, pool)
    c.verdict("geometry grid, cin=%d cout=%d" % (cin, cout))
    assert ran == forms, ran


@pytest.mark.parametrize("cin,cout", CHANNELS)
def test_every_accepted_channel_pair_matches_float64(cuda, cin, cout):
    wts, c = _Weights(cuda, cin, cout), _Checks()
    for H, W, pool in CHANNEL_MAPS:
        m = _Maps(wts, H, W)
        for form in FORMS:
            if _accepts(form, H, W, cin, cout, pool):
                _run_checked(form, c, m, pool)
    c.verdict("channel grid, cin=%d cout=%d" % (cin, cout))


# Two instantiations of the direct conv (csrc/conv_direct.hip) that the grids above do not reach.

@pytest.mark.parametrize("H,W", ((4, 4), (8, 12), (12, 40), (4, 32), (8, 64)))
def test_conv1_1_to_bf16_called_on_its_own_matches_float64(cuda, H, W):
    """ntk_vgg_conv3x3_relu_f32_to_bf16 (fp32 frames in, bf16 map out; elsewhere reached only through the bf16 trunk): the tiny-Cin
    tile kernel with a bf16 output on the first three maps (rows no multiple of the tile's 128, crossing frame boundaries), the
    row kernel where W % 32 == 0.  Against the float64 convolution of the fp32 operands, within one bf16 rounding."""
    from ntmtrack import vgg
    wts, c = _Weights(cuda, 3, 64), _Checks()
    m = _Maps(wts, H, W)
    y = vgg.conv3x3_relu_f32_to_bf16(m.xt, wts.packed("direct"), wts.bt, 3, 64)
    c.close("direct to bf16", "F=%d H=%d W=%d cin=3 cout=64" % (F, H, W), y, m.ref(False), 2.0 ** -8, bf16_out=True)
    c.verdict("conv1_1 to bf16, H=%d W=%d" % (H, W))


@pytest.mark.parametrize("H,W", ((4, 4), (8, 12), (32, 32)))
def test_tiny_cin_with_128_column_tiles_matches_float64(cuda, H, W):
    """cin = 3, cout = 128: the tiny-Cin tile kernel on 128-column tiles, with and without the pool."""
    wts, c = _Weights(cuda, 3, 128), _Checks()
    m = _Maps(wts, H, W)
    for pool in (False, True):
        _run_checked("direct", c, m, pool)
    c.verdict("tiny Cin, 128 columns, H=%d W=%d" % (H, W))
