"""CPU: vgg.trunk_plan -- which conv kernel runs which layer of the trunk in which activation layout -- against known answers,
and over a sweep of frame shapes: every plan is a chain (a step reads the layout the step before wrote, frames in and features out
are fp32 NHWC) and names only launches the library's own shape predicates accept.  The library loads without a device, so the
predicates answer here."""
import itertools

import pytest

DEFAULT = dict(layout="blocked", wino_waves=None, features_window=None, split3_upto="conv4_3", bf16_form="patch")
WINDOW = (4, 4, 24, 24)


def _plan(shape, dtype="f32", form="split3", upto="conv4_3", **kw):
    from ntmtrack import vgg
    return vgg.trunk_plan(shape, dtype, form, upto, **dict(DEFAULT, **kw))


def _text(plan):
    return ["%s %s>%s" % (s.kernel, s.src, s.dst) for s in plan]


def _layers(plan):
    from ntmtrack import vgg
    assert [s.layer for s in plan] == [l[0] for l in vgg.VGG_LAYERS[:len(plan)]]
    return plan


ALL_SPLIT = ["direct nhwc>nhwc", "split3 nhwc>split"] + ["split3 split>split"] * 7 + ["split3 split>nhwc"]
MIXED = (["direct nhwc>nhwc", "split3 nhwc>split"] + ["split3 split>split"] * 4 + ["split3 split>nhwc"]
         + ["wino43_blocked nhwc>blocked", "wino43_blocked blocked>blocked", "wino43_blocked blocked>nhwc"])
BLOCKED = ["direct nhwc>nhwc", "wino43_blocked nhwc>blocked"] + ["wino43_blocked blocked>blocked"] * 7 + ["wino43_blocked blocked>nhwc"]
NHWC43 = ["direct nhwc>nhwc"] + ["wino43 nhwc>nhwc"] * 9
POOLS = [False, True, False, True, False, False, True, False, False, False]


@pytest.mark.parametrize("shape", [(2, 224, 224), (640, 224, 224), (2, 64, 64), (2, 192, 224), (2, 256, 224), (2, 160, 224)])
def test_default_trunk_runs_the_split_form_through_conv4_3(shape):
    plan = _layers(_plan(shape))
    assert _text(plan) == ALL_SPLIT
    assert [s.pool for s in plan] == POOLS and all(s.window is None and s.waves is None for s in plan)


@pytest.mark.parametrize("shape", [(1, 128, 224), (1, 224, 192), (2, 64, 96), (2, 32, 32)])
def test_default_trunk_hands_over_to_the_blocked_winograd_kernel_after_conv3_3(shape):
    """conv4_x maps that are neither multiples of 8 nor 28 wide with at least 20 rows: conv3_3 writes fp32 NHWC for the F(4x4) kernel"""
    plan = _layers(_plan(shape))
    assert _text(plan) == MIXED and [s.pool for s in plan] == POOLS


def test_split3_upto_ends_the_split_form_early():
    assert _text(_plan((2, 224, 224), split3_upto="conv3_3")) == MIXED


@pytest.mark.parametrize("frames", [1, 2])
def test_frames_whose_conv4_blocks_span_more_than_16_mb_fall_back_to_nhwc(frames):
    """480 x 640: conv4_x cuts its 60 x 80 maps into single tiles and a block of 32 spans more than 16 MB of input, so the eight-wave
    kernel (and with it every whole-trunk route) is out"""
    from ntmtrack import vgg
    assert not vgg.blocked_trunk_supported(frames, 480, 640)
    plan = _layers(_plan((frames, 480, 640)))
    assert _text(plan) == NHWC43 and [s.pool for s in plan] == POOLS


def test_winograd_forms():
    at = (2, 224, 224)
    assert _text(_plan(at, form="winograd")) == BLOCKED
    for kw in (dict(layout="nhwc"), dict(wino_waves=4), dict(features_window=WINDOW)):
        for form in ("winograd", "split3"):                 # a window or four waves take the split trunk to this route too
            if form == "split3" and "layout" in kw:
                continue                                    # (the split route does not ask for the layout)
            plan = _layers(_plan(at, form=form, **kw))
            assert _text(plan) == NHWC43, (form, kw)
            assert [s.waves for s in plan] == [None] + [kw.get("wino_waves")] * 9
            assert [s.window for s in plan] == [None] * 9 + [kw.get("features_window")]
    assert _text(_plan(at, form="winograd2")) == ["direct nhwc>nhwc"] + ["wino nhwc>nhwc"] * 9
    assert _text(_plan(at, form="direct")) == ["direct nhwc>nhwc"] * 10
    assert _text(_plan(at, form="winograd", wino_waves=8)) == BLOCKED


@pytest.mark.parametrize("form", ["split3", "winograd", "winograd2", "direct"])
def test_a_trunk_cut_short_ends_unpooled_on_nhwc_maps(form):
    plan = _layers(_plan((2, 224, 224), form=form, upto="conv1_2"))
    kernel = {"split3": "wino43", "winograd": "wino43", "winograd2": "wino", "direct": "direct"}[form]
    assert _text(plan) == ["direct nhwc>nhwc", "%s nhwc>nhwc" % kernel]
    assert [s.pool for s in plan] == [False, False]
    # a window is for conv4_3 only
    assert all(s.window is None for s in _plan((2, 224, 224), form="winograd", upto="conv3_3", features_window=WINDOW))
    plan = _plan((2, 224, 224), form=form, upto="conv3_3")
    assert len(plan) == 7 and [s.pool for s in plan] == POOLS[:6] + [False] and {s.src for s in plan} == {"nhwc"}


def test_bf16_trunk():
    from ntmtrack import _lib
    plan = _layers(_plan((2, 224, 224), dtype="bf16"))
    assert _text(plan) == ["direct_to_bf16 nhwc>bf16"] + ["bf16p bf16>bf16"] * 8 + ["bf16p bf16>nhwc"]
    assert [s.pool for s in plan] == POOLS
    assert _text(_plan((2, 224, 224), dtype="bf16", bf16_form="tile")) == ["direct_to_bf16 nhwc>bf16"] + ["bf16 bf16>bf16"] * 8 + ["bf16 bf16>nhwc"]
    with pytest.raises(_lib.NtkError):
        _plan((2, 224, 224), dtype="bf16", upto="conv3_3")


CONFIGS = [dict(), dict(split3_upto="conv3_3"), dict(form="winograd"), dict(form="winograd", layout="nhwc"),
           dict(form="winograd", wino_waves=4), dict(form="winograd", features_window=WINDOW), dict(features_window=WINDOW),
           dict(form="winograd2"), dict(form="direct"), dict(upto="conv1_2"), dict(form="winograd", upto="conv3_3"),
           dict(dtype="bf16"), dict(dtype="bf16", bf16_form="tile")]


def _accepts(L, vgg, step, F, h, w, cin, cout):
    """Does the step's kernel take the step's shape, by the kernel's own predicate?"""
    k, pool = step.kernel, 1 if step.pool else 0
    if k == "wino":
        return L.ntk_vgg_wino_supported(F, h, w, cin, cout)
    if k == "wino43":
        return L.ntk_vgg_wino43_supported(F, h, w, cin, cout)
    if k == "wino43_blocked":
        return L.ntk_vgg_wino43_blocked_supported(F, h, w, cin, cout)
    if k == "split3":               # an fp32 map is read by the four-wave form only
        return L.ntk_vgg_split3_supported(h, w, cin, cout, pool) and (step.src == "split" or (cin <= 64 and cout == 64 and h % 8 == 0 and w % 8 == 0))
    if k == "bf16p":
        return L.ntk_vgg_bf16p_supported(h, w, cin, cout, pool)
    if k == "bf16":                 # the tile kernel (csrc/conv_direct.hip): 64-channel multiples, sides multiples of 4
        return cin % 64 == 0 and cout % 64 == 0 and h % 4 == 0 and w % 4 == 0
    assert k in ("direct", "direct_to_bf16")
    return (cin == 3 or cin % 32 == 0) and cout % 64 == 0 and h % 4 == 0 and w % 4 == 0


def test_every_plan_is_a_chain_of_launches_the_library_accepts():
    from ntmtrack import _lib, vgg
    L = _lib.lib()
    sides = range(32, 257, 32)
    n = 0
    for F, H, W, cfg in itertools.product((1, 2), sides, sides, CONFIGS):
        plan = _layers(_plan((F, H, W), **cfg))
        what = (F, H, W, cfg)
        assert len(plan) == [l[0] for l in vgg.VGG_LAYERS].index(cfg.get("upto", "conv4_3")) + 1, what
        assert plan[0].src == "nhwc" and plan[-1].dst == "nhwc", what
        h, w = H, W
        for prev, step, (_name, cin, cout, _pool) in zip((None,) + plan, plan, vgg.VGG_LAYERS):
            assert prev is None or step.src == prev.dst, (what, step)
            assert _accepts(L, vgg, step, F, h, w, cin, cout), (what, step, h, w)
            assert step.window is None or (step.kernel == "wino43" and step is plan[-1] and step.layer == "conv4_3"), (what, step)
            assert step.waves is None or step.kernel == "wino43", (what, step)
            h, w = (h // 2, w // 2) if step.pool else (h, w)
            n += 1
    assert n > 10000
