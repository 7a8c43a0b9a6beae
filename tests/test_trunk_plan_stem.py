"""CPU: vgg.trunk_plan with stem="fused" -- conv1_1 computed inside conv1_2's launch (the marker layout "stem") -- is a chain, is
offered only where ntk_vgg_split3_stem_supported says yes, and leaves every default-argument plan as it was."""
import itertools

from test_trunk_plan import ALL_SPLIT, CONFIGS, MIXED, POOLS, _layers, _plan, _text


def test_fused_stem_plan_on_the_reference_frames():
    plan = _layers(_plan((2, 224, 224), stem="fused"))
    assert _text(plan) == ["direct nhwc>stem", "split3 stem>split"] + ALL_SPLIT[2:]
    assert [s.pool for s in plan] == POOLS
    assert _text(_plan((2, 64, 96), stem="fused")) == ["direct nhwc>stem", "split3 stem>split"] + MIXED[2:]


def test_default_arguments_keep_the_separate_stem():
    for shape in ((2, 224, 224), (640, 224, 224), (2, 64, 64), (1, 128, 224)):
        assert _plan(shape) == _plan(shape, stem="separate")
        assert _text(_plan(shape))[:2] == ["direct nhwc>nhwc", "split3 nhwc>split"]


def test_fused_stem_plans_are_chains_offered_where_the_library_says_yes():
    from ntmtrack import _lib, vgg
    L = _lib.lib()
    sides = range(32, 257, 32)
    fused = 0
    for F, H, W, cfg in itertools.product((1, 2), sides, sides, CONFIGS):
        plan, base = _layers(_plan((F, H, W), stem="fused", **cfg)), _plan((F, H, W), **cfg)
        what = (F, H, W, cfg)
        assert len(plan) == len(base) and plan[0].src == "nhwc" and plan[-1].dst == "nhwc", what
        for prev, step in zip((None,) + plan, plan):
            assert prev is None or step.src == prev.dst, (what, step)
        marked = [i for i, s in enumerate(plan) if s.dst == "stem"]
        can = (len(base) > 1 and base[1].kernel == "split3" and base[1].src == "nhwc"
               and bool(L.ntk_vgg_split3_stem_supported(H, W, 1 if base[1].pool else 0)))
        if can:
            assert marked == [0] and plan[1].src == "stem" and plan[1].kernel == "split3" and plan[0].kernel == "direct", what
            assert plan[2:] == base[2:] and plan[1]._replace(src="nhwc") == base[1], what
            fused += 1
        else:
            assert plan == base, what
    assert fused > 100
    # the predicate itself: the four-wave split form's shapes (sides multiples of 8), nothing else
    for H, W in itertools.product(range(4, 72, 4), repeat=2):
        for pool in (0, 1):
            assert bool(L.ntk_vgg_split3_stem_supported(H, W, pool)) == (H % 8 == 0 and W % 8 == 0), (H, W, pool)
    assert not L.ntk_vgg_split3_stem_supported(28, 28, 0) and not L.ntk_vgg_split3_stem_supported(0, 8, 0)
