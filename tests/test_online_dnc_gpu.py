"""GPU: the online DNC trackers -- DNC.serving_state / serve_projected, ntk_dnc_state_keep, online.BatchDNCTracker and
online.DNCTracker -- against the path this feature leaves as it was: DNC.run_projected / run_sequence, online.crop_and_resize,
the trunk, ntk_gather_serialize_online and the host box geometry.

One core per kernel family, the smallest the existing tables have: the one-workgroup kernels on tests/test_dnc_gpu.py's
"word_size_5_zero_state" (word size 5, padded to 8), the LDS-resident and the memory-partitioned cluster kernels on
CLUSTER_CASES' "small_64x16"; every core takes the trunk's 514 inputs and gives 2 outputs.  Frames are 96 x 128 uint8, B = 3
objects in two clips, clips of 4 frames.

ntk_dnc_state_keep takes a row size that is no multiple of 4 (and a base that is not 16-byte aligned): such rows move one float
at a time."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import dnc_oracle as D
from oracle import ntm_oracle as O

from dnc_util import _random_state, conditioned_params, convert_state, to_device
from test_dnc_gpu import CASES, CLUSTER_CASES

pytestmark = pytest.mark.gpu

OFFSET_ATOL, REGION_ATOL = 1e-4, 1e-2          # the bounds tests/test_online_batch_gpu.py holds the NTM batch tracker to
H, W, T = 96, 128, 4
REGIONS = [(40.0, 30.0, 36.0, 27.0), (62.0, 20.0, 30.0, 40.0), (25.0, 41.0, 44.0, 33.0)]     # x, y, w, h: two in clip 0, one in clip 1
FRAME_OF = [0, 0, 1]

_SEQ = next(c for c in CASES if c[0] == "word_size_5_zero_state")
_CL = next(c for c in CLUSTER_CASES if c[0] == "small_64x16")
#: family -> (memory_size, word_size, num_reads, hidden_size, clip_value, cluster_form)
FAMILIES = {"seq": (_SEQ[3], _SEQ[4], _SEQ[5], _SEQ[7], _SEQ[8], None),
            "lds": (_CL[1], _CL[2], _CL[3], _CL[4], 20.0, "lds"),
            "mp": (_CL[1], _CL[2], _CL[3], _CL[4], 20.0, "mp")}
assert _SEQ[4] % 4 != 0 and _SEQ[6] == 1


def same_bits(a, b):
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


@pytest.fixture(scope="module")
def world(cuda):
    """Trunk weights and five frames of two clips (frame 0 starts the trackers)."""
    from ntmtrack.vgg import VGG16Conv43
    rng = np.random.default_rng(5)
    ws = O.init_vgg_weights(rng)
    frames = rng.integers(0, 256, size=(T + 1, 2, H, W, 3), dtype=np.uint8)
    return {"ws": ws, "vgg": VGG16Conv43(ws, device=cuda), "frames": frames, "dframes": torch.from_numpy(frames).to(cuda)}


def family_params(family):
    N, Wd, R, hid, clip, _form = FAMILIES[family]
    cfg = D.DNCConfig(514, 2, memory_size=N, word_size=Wd, num_reads=R, num_writes=1, hidden_size=hid, clip_value=clip)
    p = conditioned_params(cfg, np.random.default_rng(17), 2)
    p["lstm/w_gates"] = (p["lstm/w_gates"] * 0.05).astype(np.float32)      # trunk features are O(10): keep the gates off saturation
    return cfg, p


def make_core(family, cuda, params=None):
    """A fresh core of the family (its own cluster plan and workspace)."""
    from ntmtrack.dnc import DNC
    N, Wd, R, hid, clip, form = FAMILIES[family]
    core = DNC({"memory_size": N, "word_size": Wd, "num_reads": R, "num_writes": 1}, {"hidden_size": hid}, 2, clip, device=cuda)
    core.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in (params or family_params(family)[1]).items()})
    if form is None:
        core.cluster_k = 0
    else:
        core.cluster_form = form
    return core


def assert_family(core, family):
    form = FAMILIES[family][5]
    if form is None:
        assert core.last_cluster_form is None and core.last_cluster_k == 1
    else:
        assert core.last_cluster_form == form and core.last_cluster_k > 1, (core.last_cluster_form, core.last_cluster_k)
        core.check_cluster()


def make(world, cuda, family, regions=REGIONS, frame_of=FRAME_OF, core=None):
    from ntmtrack import online
    return online.BatchDNCTracker(world["dframes"][0], regions, core or make_core(family, cuda), world["vgg"], frame_of=frame_of,
                                  device=cuda)


def snapshot(trk):
    s = {"state/" + n: t.clone() for n, t in zip(trk.state.NAMES, trk.state.tensors())}
    s.update(box_state=trk.box_state.clone(), cropbox32=trk.cropbox32.clone(), frame=trk.frame.clone(),
             regions=trk.regions.clone(), offsets=trk.offsets.clone())
    return s


def leaves(st):
    a = st.access_state
    return {"reads": st.access_output, "memory": a.memory, "rw": a.read_weights, "ww": a.write_weights, "link": a.linkage.link,
            "prec": a.linkage.precedence_weights, "usage": a.usage, "h": st.controller_state.hidden, "c": st.controller_state.cell}


def single_loop(core, vgg, first_image, region, images, cuda):
    """One object tracked with what the parent commit offers: online.crop_and_resize, the trunk, ntk_gather_serialize_online,
    DNC.run_sequence(X, prev_state) and the host box arithmetic of online.NTMTracker.  -> (offsets [T,2], regions [T,4])."""
    from ntmtrack import _lib, geometry as G, online
    P = _lib.ptr
    Hh, Ww = first_image.shape[:2]

    def boxes(region):
        x1, y1, w, h = region
        bbox = (y1, x1, y1 + h, x1 + w)
        nb = list(bbox) if (x1 < 1 and y1 < 1 and w < 1 and h < 1) else G.normalize_bbox((Ww, Hh), bbox)
        cb = G.calculate_cropbox(nb, 8, 6)
        return nb, cb, G.calculate_transformation(cb)

    def frame(img, nb, cb, tr, first, state):
        crop = online.crop_and_resize(img.to(torch.float32), cb)
        fmap = vgg(crop.unsqueeze(0), latency=True)
        gts0 = None
        if first:
            gt = G.generate_gt(G.apply_transformation(nb, tr), 8, 6)
            gts0 = torch.as_tensor(gt.reshape(1, -1), dtype=torch.float32).to(cuda).contiguous()
        X = torch.empty((1, 65, core.ldx), device=cuda)
        _lib.check(_lib.lib().ntk_gather_serialize_online(P(fmap), None if gts0 is None else P(gts0), P(X), 1, 1, 28, 28, 512,
                                                          core.ldx, 6, 2, 8, _lib.stream()), "ntk_gather_serialize_online")
        out, state = core.run_sequence(X[:, :, :core.D].transpose(0, 1).contiguous(), state)
        return out[-1, 0], state

    nb, cb, tr = boxes(region)
    _, state = frame(first_image, nb, cb, tr, True, None)
    init = [.5 - .375, .5 - .375, .5 + .375, .5 + .375]
    offsets, regions = [], []
    for img in images:
        logits, state = frame(img, nb, cb, tr, False, state)
        off = torch.tanh(logits).cpu().numpy()
        y1, x1, y2, x2 = G.apply_transformation(G.offset_bbox(init, off), np.linalg.inv(tr))
        region = (x1 * Ww, y1 * Hh, (x2 - x1) * Ww, (y2 - y1) * Hh)
        offsets.append(off)
        regions.append(region)
        nb, cb, tr = boxes(region)
    return np.array(offsets), np.array(regions)


# ------------------------------------------------------------------------------------------------------- 1. the state path
@pytest.mark.parametrize("S", [1, 65])
@pytest.mark.parametrize("family", list(FAMILIES))
def test_serve_projected_equals_run_projected(cuda, family, S):
    """Same kernel, same plan (equal B on one core), same inputs: outputs and every state tensor have the same bits; nothing of
    the serving state is cloned on the way (the buffers keep their addresses)."""
    from ntmtrack import dnc as G
    B = 3
    cfg, p = family_params(family)
    core = make_core(family, cuda, p)
    rng = np.random.default_rng(100 + S)
    st0 = convert_state(_random_state(cfg, B, rng), G, to_device(cuda))
    xproj = torch.from_numpy(rng.standard_normal((B * S, 4 * core.hid)).astype(np.float32)).to(cuda)

    ref_out_tm, ref_st = core.run_projected(xproj, B, S, st0, record=False)
    ref_plan = (core.last_cluster_form, core.last_cluster_k)
    assert_family(core, family)

    ss = core.serving_state(B).load(st0)
    for k, v in leaves(ss.to_state()).items():
        assert same_bits(v, leaves(st0)[k]), "load / to_state round trip: " + k
    addresses = [t.data_ptr() for t in ss.tensors()]
    out = core.serve_projected(xproj, B, S, ss)
    assert (core.last_cluster_form, core.last_cluster_k) == ref_plan
    assert_family(core, family)
    torch.cuda.synchronize()
    assert [t.data_ptr() for t in ss.tensors()] == addresses
    assert out.shape == (B, S, 2)
    got, want = leaves(ss.to_state()), leaves(ref_st)
    err = max([float((out - ref_out_tm.transpose(0, 1)).abs().max())] + [float((got[k] - want[k]).abs().max()) for k in want])
    print("%s S=%d: max |serve_projected - run_projected| over outputs and state %.3g" % (family, S, err))
    assert err <= 5e-5
    assert same_bits(out, ref_out_tm.transpose(0, 1).contiguous()), "outputs"
    for k in want:
        assert same_bits(got[k], want[k]), k
    if core.word_size != core.W:
        assert not ss.mem[..., core.word_size:].any() and not ss.reads[..., core.word_size:].any()
    # a second call goes on from the state the first one left, as chained run_projected calls do
    out2 = core.serve_projected(xproj, B, S, ss)
    ref2_tm, _ = core.run_projected(xproj, B, S, ref_st, record=False)
    assert same_bits(out2, ref2_tm.transpose(0, 1).contiguous())


# ---------------------------------------------------------------------------------------------------- 2. ntk_dnc_state_keep
@pytest.mark.parametrize("pattern", ["none", "all", "alternating"])
@pytest.mark.parametrize("keep_where", [0, 1])
def test_state_keep_copies_selected_rows_only(cuda, pattern, keep_where):
    from ntmtrack import online
    B = 5
    rows = [4, 20, 64 * 64, 1027, 8]           # 1027: no multiple of 4, crosses a chunk; the 8 sits on a base that is not 16-byte aligned
    g = torch.Generator().manual_seed(2)
    srcs = [torch.randn((B, n), generator=g).to(cuda) for n in rows[:4]]
    dsts = [torch.full((B, n), float("nan"), device=cuda) for n in rows[:4]]
    odd_src, odd_dst = torch.randn((B * 8 + 1,), generator=g).to(cuda), torch.full((B * 8 + 1,), float("nan"), device=cuda)
    srcs.append(odd_src[1:].view(B, 8))
    dsts.append(odd_dst[1:].view(B, 8))
    assert srcs[-1].data_ptr() % 16 == 4
    mask = {"none": [0] * B, "all": [1] * B, "alternating": [1, 0, 1, 0, 1]}[pattern]
    dmask = torch.tensor(mask, device=cuda, dtype=torch.uint8)
    table = lambda ts: torch.tensor([t.data_ptr() for t in ts], device=cuda, dtype=torch.int64)
    online.state_keep(dmask, keep_where, B, table(srcs), table(dsts), (ctypes.c_longlong * len(rows))(*rows))
    torch.cuda.synchronize()
    poison = torch.full((1,), float("nan"))
    for n, s, d in zip(rows, srcs, dsts):
        for b in range(B):
            if mask[b] == keep_where:
                assert same_bits(d[b], s[b]), "row %d of the tensor with %d floats per row was not copied" % (b, n)
            else:
                assert same_bits(d[b], poison.expand(n).contiguous()), "row %d of the tensor with %d floats per row was touched" % (b, n)
    assert same_bits(odd_dst[:1], poison)


# ----------------------------------------------------------------------------------------------- 3. tracker against the loop
@pytest.fixture(scope="module")
def clip_runs(world, cuda):
    """family -> the batch tracker's clip and the three single-object loops over the parent's API, computed once."""
    cache = {}

    def get(family):
        if family not in cache:
            trk = make(world, cuda, family)
            regions = trk.track_clip(world["dframes"][1:])
            offsets = trk.offsets.clone()
            form = (trk.core.last_cluster_form, trk.core.last_cluster_k)
            trk.check()
            loops = [single_loop(make_core(family, cuda), world["vgg"], world["dframes"][0, f], r,
                                 [world["dframes"][t, f] for t in range(1, T + 1)], cuda) for r, f in zip(REGIONS, FRAME_OF)]
            cache[family] = {"trk": trk, "regions": regions, "offsets": offsets, "form": form, "loops": loops}
        return cache[family]
    return get


@pytest.mark.parametrize("family", list(FAMILIES))
def test_batch_tracker_matches_single_object_loops(world, cuda, clip_runs, family):
    run = clip_runs(family)
    trk, regions = run["trk"], run["regions"]
    assert regions.is_cuda and regions.dtype == torch.float64 and regions.shape == (T, 3, 4)
    form, k = run["form"]
    want_form = FAMILIES[family][5]
    assert form == want_form and (k > 1) == (want_form is not None)
    assert trk.frame.tolist() == [T] * 3
    got = regions.cpu().numpy()
    ref_regions = np.stack([l[1] for l in run["loops"]], axis=1)             # [T,3,4]
    ref_last_offsets = np.stack([l[0][-1] for l in run["loops"]])            # [3,2]
    er = np.abs(got - ref_regions).max()
    eo = np.abs(run["offsets"].cpu().numpy() - ref_last_offsets).max()
    print("%s (k %d): batch of 3 against three loops over %d frames: max |offset err| %.3g, max |region err| %.3g px"
          % (family, k, T, eo, er))
    assert np.isfinite(got).all() and np.abs(ref_last_offsets).max() > 1e-3      # the clip moves the boxes: not a comparison of zeros
    assert eo <= OFFSET_ATOL
    assert er <= REGION_ATOL
    # the state is the serving state; its logical form has the caller's word size
    st = trk.state.to_state()
    assert st.access_state.memory.shape == (3, FAMILIES[family][0], FAMILIES[family][1])
    # track() frame by frame issues the same launches as track_clip: same bits
    again = make(world, cuda, family)
    frames = [again.track(world["dframes"][t]) for t in range(1, T + 1)]
    assert same_bits(torch.stack(frames), regions)


# ------------------------------------------------------------------------------------------------------------------ 4. mask
@pytest.mark.parametrize("family", list(FAMILIES))
def test_inactive_trackers_keep_everything_and_active_ones_do_not_notice(world, cuda, family):
    d = world["dframes"]
    trk, full_a, full_b = make(world, cuda, family), make(world, cuda, family), make(world, cuda, family)
    for t_ in (trk, full_a, full_b):
        t_.track(d[1])
    # frame 2 with slots 0 and 2, frame 3 with slot 1 only
    before = snapshot(trk)
    r = trk.track(d[2], active=[1, 0, 1])
    mid = snapshot(trk)
    r_a = full_a.track(d[2])
    a = snapshot(full_a)
    assert trk.frame.tolist() == [2, 1, 2]
    for k in before:
        assert same_bits(mid[k][1], before[k][1]), "inactive tracker changed: " + k
        for b in (0, 2):
            assert same_bits(mid[k][b], a[k][b]), "active tracker %d differs from the unmasked run: %s" % (b, k)
    assert same_bits(r[1], before["regions"][1]) and same_bits(r[0], r_a[0]) and same_bits(r[2], r_a[2])
    trk.track(d[3], active=torch.tensor([0, 1, 0], device=cuda, dtype=torch.uint8))
    full_b.track(d[3])
    end, b_ = snapshot(trk), snapshot(full_b)
    assert trk.frame.tolist() == [2, 2, 2]
    for k in end:
        assert same_bits(end[k][1], b_[k][1]), "slot 1 (frames 1, 3) differs from an unmasked run of frames 1, 3: " + k
        for b in (0, 2):
            assert same_bits(end[k][b], mid[k][b]), "inactive tracker %d changed: %s" % (b, k)
    assert not torch.isnan(trk.regions).any()
    trk.check()
    assert trk.core.last_cluster_form == FAMILIES[family][5]


# ----------------------------------------------------------------------------------------------------------------- 5. reset
@pytest.mark.parametrize("family", list(FAMILIES))
def test_reset_starts_one_slot_anew_and_leaves_the_others(world, cuda, family):
    from ntmtrack import online
    d = world["dframes"]
    trk, plain = make(world, cuda, family), make(world, cuda, family)
    trk.track(d[1]); plain.track(d[1])
    region, image = (55.0, 22.0, 32.0, 45.0), d[2, 1]
    trk.reset([1], image, [region])
    assert trk.frame.tolist() == [1, 0, 1]
    fresh = online.BatchDNCTracker(image, [region], make_core(family, cuda), world["vgg"], device=cuda)
    eo = er = 0.0
    for t in (3, 4):
        got = trk.track(d[t], frame_of=[0, 1, 1])
        want = plain.track(d[t])
        one = fresh.track(d[t, 1])
        eo = max(eo, float((trk.offsets[1] - fresh.offsets[0]).abs().max()))
        er = max(er, float((got[1] - one[0]).abs().max()))
        for b in (0, 2):
            assert same_bits(got[b], want[b]), "reset disturbed slot %d at frame %d" % (b, t)
    s, p_ = snapshot(trk), snapshot(plain)
    for k in s:
        for b in (0, 2):
            assert same_bits(s[k][b], p_[k][b]), "reset disturbed slot %d: %s" % (b, k)
    print("%s: the reset slot against a fresh tracker at B = 1 over 2 frames: max |offset err| %.3g, max |region err| %.3g px"
          % (family, eo, er))
    assert eo <= OFFSET_ATOL and er <= REGION_ATOL
    assert trk.frame.tolist() == [3, 2, 3]
    trk.check()


# ---------------------------------------------------------------------------------------------------------- 6. from_tracker
def test_from_tracker_serves_a_checkpointed_offset_tracker(world, cuda, tmp_path):
    """DNCOffsetTracker.infer serialises the training way (delimiter row last, the delimiter step read) and starts every call from
    zero state, so its output is not what an online frame computes.  The documented equivalent is used instead: the first tracked
    frame's offsets equal tanh of the last step of DNC.run_sequence over the same crops serialised the online way, state
    chained from the first frame -- single_loop above -- on a separate core that holds the SAVED tracker's parameters."""
    from ntmtrack import online, tracker
    from ntmtrack.dnc import DNC
    N, Wd, R, hid = FAMILIES["lds"][:4]
    kw = dict(mem_size=N, mem_dim=Wd, hidden_size=hid, read_head_size=R, write_head_size=1, clip_value=20, device=cuda)
    saved = tracker.DNCOffsetTracker(1, 2, vgg_weights=None, seed=7, **kw)
    saved.core.params.view("WxT").mul_(0.05)                    # as family_params: keep the gates off saturation
    path = saved.save_checkpoint(str(tmp_path / "dnc.ckpt"))
    loaded = tracker.DNCOffsetTracker(1, 2, vgg_weights=None, seed=8, **kw)
    assert not torch.equal(loaded.core.params.flat, saved.core.params.flat)
    loaded.load_checkpoint(path)
    loaded.vgg = world["vgg"]
    d = world["dframes"]
    trk = online.BatchDNCTracker.from_tracker(loaded, d[0], REGIONS, frame_of=FRAME_OF, device=cuda)
    assert trk.core is loaded.core and trk.vgg is world["vgg"]
    trk.track(d[1])
    trk.check()
    ref_core = DNC({"memory_size": N, "word_size": Wd, "num_reads": R, "num_writes": 1}, {"hidden_size": hid}, 2, 20, device=cuda)
    ref_core.load_state_dict(saved.state_dict())
    eo = er = 0.0
    for b, (r, f) in enumerate(zip(REGIONS, FRAME_OF)):
        offs, regs = single_loop(ref_core, world["vgg"], d[0, f], r, [d[1, f]], cuda)
        eo = max(eo, np.abs(trk.offsets[b].cpu().numpy() - offs[0]).max())
        er = max(er, np.abs(trk.regions[b].cpu().numpy() - regs[0]).max())
    print("from_tracker: first tracked frame against the loop on the saved parameters: max |offset err| %.3g, |region err| %.3g px"
          % (eo, er))
    assert float(trk.offsets.abs().max()) > 1e-3
    assert eo <= OFFSET_ATOL and er <= REGION_ATOL
    # the same through the explicit trunk argument, and a head is refused
    loaded.vgg = None
    again = online.BatchDNCTracker.from_tracker(loaded, d[0], REGIONS, vgg=world["vgg"], frame_of=FRAME_OF, device=cuda)
    again.track(d[1])
    assert same_bits(again.offsets, trk.offsets)
    from ntmtrack._lib import NtkError
    with pytest.raises(NtkError, match="head"):
        online.BatchDNCTracker(d[0], REGIONS, loaded.core, world["vgg"], head=object(), frame_of=FRAME_OF, device=cuda)


# ------------------------------------------------------------------------------------------ 7. allocation and synchronisation
@pytest.mark.parametrize("family", list(FAMILIES))
def test_unmasked_frames_allocate_nothing_and_do_not_wait_for_the_device(world, cuda, family):
    """Caching-allocator requests ("allocation.all.allocated") over ten frames after a warm one.  The per-frame path (crop,
    trunk, serialise, projection, core, boxes) makes none: track_clip of ten frames makes exactly ONE request, its [T,B,4]
    result, and ten track() calls make exactly ten, the [B,4] tensor each returns (BatchNTMTracker's contract: the caller
    owns what track returns)."""
    d = world["dframes"]
    ten = d[1:].repeat(3, 1, 1, 1, 1)[:10].contiguous()
    trk = make(world, cuda, family)
    trk.track(d[1])                                             # warm: plan, workspace, trunk buffers, feature map
    torch.cuda.synchronize()
    count = lambda: torch.cuda.memory_stats(cuda)["allocation.all.allocated"]
    n0 = count()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        clip = trk.track_clip(ten)
        n1 = count()
        outs = [trk.track(ten[t]) for t in range(10)]
        n2 = count()
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    print("%s: allocator requests over ten frames: track_clip %d, ten track() calls %d" % (family, n1 - n0, n2 - n1))
    assert n1 - n0 == 1
    assert n2 - n1 == 10
    # track() returns while the device is still working: the event recorded after the call has not completed, at least once in ten
    pending = 0
    for t in range(10):
        e0, e1 = torch.cuda.Event(), torch.cuda.Event()
        e0.record()
        trk.track(ten[t])
        e1.record()
        pending += 0 if e1.query() else 1
    torch.cuda.synchronize()
    print("%s: track() returned before the device had finished in %d of 10 frames" % (family, pending))
    assert pending >= 1
    assert torch.isfinite(clip).all() and all(torch.isfinite(o).all() for o in outs)
    assert trk.frame.tolist() == [31] * 3
    trk.check()


# --------------------------------------------------------------------------------------------------- 8. single-object tracker
@pytest.mark.parametrize("family", list(FAMILIES))
def test_single_tracker_returns_row_zero_of_a_batch_of_one(world, cuda, family):
    from ntmtrack import online
    frames = world["frames"]                                    # host uint8 arrays, as a caller of the single tracker has them
    one = online.DNCTracker(frames[0, 0], REGIONS[0], make_core(family, cuda), world["vgg"], device=cuda)
    batch = make(world, cuda, family, [REGIONS[0]], [0])
    for t in (1, 2):
        r = one.track(frames[t, 0])
        want = batch.track(world["dframes"][t]).cpu().numpy()[0]
        assert isinstance(r, online.Rectangle)
        assert tuple(r) == tuple(want.tolist())
        assert one.offsets.dtype == np.float32 and np.array_equal(one.offsets, batch.offsets.cpu().numpy()[0])
    assert one.frame == 2


def test_single_tracker_matches_the_numpy_restatement(world, cuda):
    """One object, the first tracked frame, the one-workgroup core, against tests/dnc_online_util.py (crop and trunk in float64,
    core in float32).  Bounds: those tests/test_online_gpu.py:86-87 holds the NTM online tracker to against the same chain."""
    from dnc_online_util import online_dnc_loop
    from ntmtrack import online
    cfg, p = family_params("seq")
    frames = world["frames"]
    offs, regs, _st = online_dnc_loop(cfg, p, world["ws"], frames[0, 0], REGIONS[0], [frames[1, 0]])
    one = online.DNCTracker(frames[0, 0], REGIONS[0], make_core("seq", cuda, p), world["vgg"], device=cuda)
    got = one.track(frames[1, 0])
    eo, er = np.abs(one.offsets - offs[0]).max(), np.abs(np.array(got) - regs[0]).max()
    print("single tracker against the numpy restatement: |offset err| %.3g, |region err| %.3g px (offsets %s)" % (eo, er, offs[0]))
    assert eo <= OFFSET_ATOL and er <= REGION_ATOL
