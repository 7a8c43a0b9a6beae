"""GPU: the batched online tracker -- ntk_crop_and_resize_batch, ntk_track_boxes_update, ntk_select_rows and
online.BatchNTMTracker -- against the single-object path (online.crop_and_resize, geometry.py, online.NTMTracker), which this
feature leaves as it was."""
import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O

pytestmark = pytest.mark.gpu

OFFSET_ATOL, REGION_ATOL = 1e-4, 1e-2          # the project's own bounds for this path (tests/test_online_gpu.py:86-87)


def same_bits(a, b):
    a, b = a.detach().cpu().reshape(-1), b.detach().cpu().reshape(-1)
    return a.shape == b.shape and a.dtype == b.dtype and bool((a.view(torch.uint8) == b.view(torch.uint8)).all())


# ---------------------------------------------------------------------------------------------------------------- 1. crop
def test_batched_crop_is_bit_equal_to_the_one_box_entry(cuda):
    from ntmtrack import online
    rng = np.random.default_rng(0)
    images = torch.from_numpy(rng.uniform(0, 255, size=(2, 37, 53, 3)).astype(np.float32)).to(cuda)
    boxes = [[0.1, 0.2, 0.8, 0.9], [-0.2, -0.1, 0.6, 1.3], [0.25, 0.25, 0.75, 0.75],     # tests/test_online_gpu.py:16
             [0.5, 0.4, 1.2, 0.9],                                                        # leaves the image
             [-0.5, -0.5, -0.1, -0.1]]                                                    # entirely outside it
    frame_of = [1, 0, 0, 1, 0]
    mean = torch.tensor(online.VGG_MEAN, device=cuda, dtype=torch.float32)
    dbox = torch.tensor(boxes, device=cuda, dtype=torch.float32)
    dfo = torch.tensor(frame_of, device=cuda, dtype=torch.int32)
    got = online.crop_and_resize_batch(images, dfo, dbox, crop=24, mean=mean)
    assert got.shape == (5, 24, 24, 3)
    for b, (f, box) in enumerate(zip(frame_of, boxes)):
        ref = online.crop_and_resize(images[f], box, crop=24)
        assert same_bits(got[b], ref), "box %d" % b
    assert got[:4].abs().sum() > 0 and not got[4].any()

    # uint8 frames: converted exactly, so the same values give the same bits
    u8 = images.round().to(torch.uint8)
    got_u8 = online.crop_and_resize_batch(u8, dfo, dbox, crop=24, mean=mean)
    got_f32 = online.crop_and_resize_batch(u8.to(torch.float32), dfo, dbox, crop=24, mean=mean)
    assert same_bits(got_u8, got_f32)

    # a frame index outside [0, F) is not dereferenced: that tracker's crop is the extrapolation value, the call returns
    for bad in (7, -1):
        fo = torch.tensor([1, bad, 0, 1, 0], device=cuda, dtype=torch.int32)
        for imgs in (images, u8):
            out = online.crop_and_resize_batch(imgs, fo, dbox, crop=24, mean=mean)
            torch.cuda.synchronize()
            assert not out[1].any()
            assert same_bits(out[0], (got if imgs is images else got_u8)[0])


# ---------------------------------------------------------------------------------------------------------- 2. box update
def test_box_update_matches_the_host_geometry(cuda):
    """Expectation: NTMTracker.track's bookkeeping (offset_bbox, _decode_bbox, _update_bbox) with geometry.py in float64, from
    the fp32 tanh of the same logits, as that tracker reads it back from the device.  Two checks: the emitted fp32 offsets
    against np.tanh within 2e-7 (a host tanh and the device's fp32 tanh may differ in the last bit; one fp32 ulp of offset is
    up to 3e-4 px of region on these image sizes, so it cannot be folded into the 1e-6 px bound), and the geometry from
    exactly those fp32 offsets (the shifted box an fp32 sum, as geometry.offset_bbox gives it for fp32 offsets; float64 after
    it) within 1e-6 px / 1e-9."""
    from ntmtrack import _lib, geometry as G
    rng = np.random.default_rng(11)
    B, S, CG, BG = 7, 3, 8, 6
    QUIRK, IDLE = 2, 4
    sizes = rng.integers(64, 4000, size=(B, 2)).astype(np.float64)                 # (w, h)
    logits = rng.uniform(-2, 2, size=(B, S, 2)).astype(np.float32)
    state = np.empty((B, 10), dtype=np.float64)
    for b in range(B):
        c, half = rng.uniform(0.2, 0.8, size=2), rng.uniform(0.02, 0.2, size=2)
        nb = [c[0] - half[0], c[1] - half[1], c[0] + half[0], c[1] + half[1]]
        if b == QUIRK:                      # a box so small that the decoded region is < 1 px in all four numbers
            nb = [1e-4, 2e-4, 9e-4, 1.2e-3]
            sizes[b] = (300, 200)
        state[b] = list(sizes[b]) + nb + G.calculate_cropbox(nb, CG, BG)
    active = np.ones(B, dtype=np.uint8)
    active[IDLE] = 0

    # ---- device
    SENT = -12345.5
    d_state = torch.from_numpy(state).to(cuda)
    d_state[IDLE, 2:] = SENT
    d_cb32 = torch.full((B, 4), SENT, device=cuda, dtype=torch.float32)
    d_reg = torch.full((B, 4), SENT, device=cuda, dtype=torch.float64)
    d_off = torch.full((B, 2), SENT, device=cuda, dtype=torch.float32)
    d_frame = torch.full((B,), 41, device=cuda, dtype=torch.int32)
    P = _lib.ptr
    _lib.check(_lib.lib().ntk_track_boxes_update(P(torch.from_numpy(logits).to(cuda)), B, S, float(CG), float(BG),
                                                 P(torch.from_numpy(active).to(cuda)), P(d_state), P(d_cb32), P(d_reg), P(d_off),
                                                 P(d_frame), _lib.stream()), "ntk_track_boxes_update")
    torch.cuda.synchronize()
    g_state, g_cb32, g_reg, g_off = d_state.cpu().numpy(), d_cb32.cpu().numpy(), d_reg.cpu().numpy(), d_off.cpu().numpy()
    # ---- host expectation, from the emitted fp32 offsets
    exp_regions, exp_state, exp_off = np.zeros((B, 4)), state.copy(), np.zeros((B, 2))
    width = BG / float(CG)
    init = [.5 - width / 2, .5 - width / 2, .5 + width / 2, .5 + width / 2]
    quirk_taken = []
    for b in range(B):
        w, h = state[b, :2]
        off = g_off[b]                     # the fp32 offsets the device emitted (np.float32, as the tracker holds them); checked below
        tr = G.calculate_transformation(state[b, 6:10])
        y1, x1, y2, x2 = G.apply_transformation(G.offset_bbox(init, off), np.linalg.inv(tr))
        y1, x1, y2, x2 = y1 * h, x1 * w, y2 * h, x2 * w
        rx, ry, rw, rh = x1, y1, x2 - x1, y2 - y1
        normalized = rx < 1 and ry < 1 and rw < 1 and rh < 1
        quirk_taken.append(normalized)
        bbox = (ry, rx, ry + rh, rx + rw)
        nb = list(bbox) if normalized else G.normalize_bbox((w, h), bbox)
        exp_regions[b], exp_off[b] = (rx, ry, rw, rh), np.tanh(logits[b, -1].astype(np.float64))
        exp_state[b, 2:6], exp_state[b, 6:10] = nb, G.calculate_cropbox(nb, CG, BG)
    assert quirk_taken == [b == QUIRK for b in range(B)]

    on = active.astype(bool)
    errs = {"regions": np.abs(g_reg - exp_regions)[on].max(), "state": np.abs(g_state - exp_state)[on].max(),
            "offsets": np.abs(g_off.astype(np.float64) - exp_off)[on].max()}
    e32 = exp_state[:, 6:10].astype(np.float32)
    ulps = (np.abs(g_cb32.astype(np.float64) - e32.astype(np.float64)) / np.spacing(np.abs(e32)).astype(np.float64))[on].max()
    print("box update: max |region err| %.3g px, max |state err| %.3g, max |offset err| %.3g, crop box fp32 %.3g ulp"
          % (errs["regions"], errs["state"], errs["offsets"], ulps))
    assert errs["regions"] <= 1e-6
    assert errs["state"] <= 1e-9
    assert ulps <= 1.0
    assert errs["offsets"] <= 2e-7
    assert (d_frame.cpu().numpy() == np.where(on, 42, 41)).all()
    # the inactive tracker: nothing of it was written
    assert (g_state[IDLE, :2] == state[IDLE, :2]).all() and (g_state[IDLE, 2:] == SENT).all()
    assert (g_cb32[IDLE] == SENT).all() and (g_reg[IDLE] == SENT).all() and (g_off[IDLE] == SENT).all()


def test_select_rows_keeps_the_masked_rows(cuda):
    from ntmtrack import online
    g = torch.Generator().manual_seed(3)
    a, b = torch.randn((5, 37), generator=g).to(cuda), torch.randn((5, 37), generator=g).to(cuda)
    mask = torch.tensor([1, 0, 0, 1, 1], device=cuda, dtype=torch.uint8)
    ref = torch.where(mask.bool()[:, None], a, b)
    assert same_bits(online.select_rows(mask, a, b), ref)
    a2 = a.clone()
    online.select_rows(mask, a2, b, out=a2)                    # in place, as the tracker uses it
    assert same_bits(a2, ref)


# ------------------------------------------------------------------------------------------------- 3-5. the tracker class
H, W = 90, 120
REGIONS = [(40.0, 30.0, 36.0, 27.0), (62.0, 20.0, 30.0, 40.0), (25.0, 41.0, 44.0, 33.0)]     # x, y, w, h: two in clip A, one in B
FRAME_OF = [0, 0, 1]
EXTRA_REGIONS, EXTRA_FRAME_OF = [(10.0, 12.0, 50.0, 40.0), (70.0, 35.0, 28.0, 36.0)], [1, 0]


@pytest.fixture(scope="module")
def model(cuda):
    """Cell, trunk weights, seed and frame size of test_online_tracker_two_frames_match_oracle; four frames of two clips."""
    from ntmtrack.ntm import NTMCell
    from ntmtrack.vgg import VGG16Conv43
    rng = np.random.default_rng(5)
    ws = O.init_vgg_weights(rng)
    cfg = O.NTMConfig(514, 2, mem_size=128, mem_dim=20, shift_range=1, controller_hidden_size=200, controller_num_layers=1,
                      write_head_size=1, read_head_size=4)
    params = O.init_params(cfg, rng, scale=0.05)
    frames = rng.uniform(0, 255, size=(4, 2, H, W, 3)).astype(np.float32)          # [t, clip, H, W, 3]
    cell = NTMCell(2, mem_size=128, mem_dim=20, controller_hidden_size=200, controller_num_layers=1, write_head_size=1,
                   read_head_size=4, device=cuda)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, input_dim=514)
    return {"cell": cell, "vgg": VGG16Conv43(ws, device=cuda), "frames": frames, "dframes": torch.from_numpy(frames).to(cuda)}


def make(model, cuda, regions=REGIONS, frame_of=FRAME_OF, cell=None):
    from ntmtrack import online
    return online.BatchNTMTracker(model["dframes"][0], regions, cell or model["cell"], model["vgg"], frame_of=frame_of, device=cuda)


def test_batch_matches_three_single_trackers(model, cuda):
    from ntmtrack import online
    frames, dframes = model["frames"], model["dframes"]
    # the reference: three independent single-object trackers, code this feature does not touch
    singles = [online.NTMTracker(frames[0, f], r, model["cell"], model["vgg"], device=cuda) for r, f in zip(REGIONS, FRAME_OF)]
    ref_regions, ref_offsets = [], []
    for t in (1, 2, 3):
        ref_regions.append([tuple(s.track(frames[t, f])) for s, f in zip(singles, FRAME_OF)])
        ref_offsets.append([s.offsets.copy() for s in singles])
    trk = make(model, cuda)
    assert trk.state["M"].shape[0] == 3
    got_regions, got_offsets = [], []
    for t in (1, 2, 3):
        r = trk.track(dframes[t])
        assert r.is_cuda and r.dtype == torch.float64 and r.shape == (3, 4)
        got_regions.append(r)
        got_offsets.append(trk.offsets.clone())
    torch.cuda.synchronize()
    assert trk.frame.tolist() == [3, 3, 3]
    eo = max(np.abs(g.cpu().numpy() - np.array(r)).max() for g, r in zip(got_offsets, ref_offsets))
    er = max(np.abs(g.cpu().numpy() - np.array(r)).max() for g, r in zip(got_regions, ref_regions))
    print("batch of 3 against three single trackers over 3 frames: max |offset err| %.3g, max |region err| %.3g px" % (eo, er))
    for t in range(3):
        np.testing.assert_allclose(got_offsets[t].cpu().numpy(), np.array(ref_offsets[t]), rtol=0, atol=OFFSET_ATOL)
        np.testing.assert_allclose(got_regions[t].cpu().numpy(), np.array(ref_regions[t]), rtol=0, atol=REGION_ATOL)

    # track_clip on the same three frames: the same launches, so the same bits
    clip = make(model, cuda).track_clip(dframes[1:4])
    assert clip.is_cuda and clip.shape == (3, 3, 4)
    assert same_bits(clip, torch.stack(got_regions))

    # the same three trackers inside a batch of five (both sizes run the same trunk form): a tracker's results do not
    # depend on who else is in the batch
    assert 5 < model["vgg"].split3_latency_frames
    five = make(model, cuda, REGIONS + EXTRA_REGIONS, FRAME_OF + EXTRA_FRAME_OF)
    clip5 = five.track_clip(dframes[1:4])
    assert same_bits(clip5[:, :3].contiguous(), clip)
    assert same_bits(five.offsets[:3].contiguous(), got_offsets[-1])
    for k in trk.state:
        assert same_bits(five.state[k][:3].contiguous(), trk.state[k]), k


def test_track_clip_makes_no_host_round_trip(model, cuda):
    trk = make(model, cuda)
    dframes = model["dframes"]
    u8 = model["frames"][2:4].round().astype(np.uint8)          # a host array: uploaded through pinned memory, no sync either
    active = torch.tensor([[1, 1, 1], [1, 0, 1]], device=cuda, dtype=torch.uint8)
    trk.track(dframes[1])                                       # warm-up: plans, workspaces and packed weights exist after it
    trk.track_clip(u8[:1])
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        out = trk.track_clip(dframes[2:4])
        out_masked = trk.track_clip(dframes[2:4], active=active)
        out_host = trk.track_clip(u8)
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    for o in (out, out_masked, out_host):
        assert torch.is_tensor(o) and o.is_cuda and o.shape == (2, 3, 4)
    torch.cuda.synchronize()
    assert torch.isfinite(out).all() and torch.isfinite(out_host).all()


def snapshot(trk):
    s = {"state/" + k: v.clone() for k, v in trk.state.items()}
    s.update(box_state=trk.box_state.clone(), cropbox32=trk.cropbox32.clone(), frame=trk.frame.clone(),
             regions=trk.regions.clone(), offsets=trk.offsets.clone())
    return s


def test_active_mask_and_reset(model, cuda):
    from ntmtrack import online
    dframes = model["dframes"]
    trk, full = make(model, cuda), make(model, cuda)
    trk.track(dframes[1]); full.track(dframes[1])
    before = snapshot(trk)
    r = trk.track(dframes[2], active=[1, 0, 1])
    r_full = full.track(dframes[2])
    after, after_full = snapshot(trk), snapshot(full)
    assert trk.frame.tolist() == [2, 1, 2]
    for k in before:
        assert same_bits(after[k][1], before[k][1]), "inactive tracker changed: " + k
        for b in (0, 2):
            assert same_bits(after[k][b], after_full[k][b]), "active tracker %d differs from the unmasked run: %s" % (b, k)
    assert same_bits(r[1], before["regions"][1]) and same_bits(r[0], r_full[0]) and same_bits(r[2], r_full[2])

    # reset slot 1 on a new image and region: equal to a freshly constructed single-object tracker, the others untouched
    region, image = (55.0, 22.0, 32.0, 45.0), dframes[3, 1]
    trk.reset([1], image, [region])
    fresh = online.BatchNTMTracker(image, [region], model["cell"], model["vgg"], device=cuda)
    got, want = snapshot(trk), snapshot(fresh)
    for k in got:
        assert same_bits(got[k][1], want[k][0]), "reset slot differs from a fresh tracker: " + k
        for b in (0, 2):
            assert same_bits(got[k][b], after[k][b]), "reset touched slot %d: %s" % (b, k)
    # and the slot goes on tracking like the fresh one
    a, f = trk.track(dframes[3], frame_of=[0, 1, 1]), fresh.track(dframes[3, 1])
    assert same_bits(a[1], f[0])


# ------------------------------------------------------------------------------------------------- 6. a deeper controller
def test_stacked_cell_batch_matches_batches_of_one(model, cuda):
    from ntmtrack.ntm import NTMCell, StackedNTMCell
    cell = NTMCell(2, mem_size=128, mem_dim=20, controller_hidden_size=200, controller_num_layers=2, write_head_size=1,
                   read_head_size=4, input_dim=514, device=cuda, init_scale=0.05, seed=9)
    assert isinstance(cell, StackedNTMCell)
    dframes = model["dframes"]
    regions, frame_of = REGIONS[1:], FRAME_OF[1:]
    two = make(model, cuda, regions, frame_of, cell=cell)
    ones = [make(model, cuda, [r], [f], cell=cell) for r, f in zip(regions, frame_of)]
    assert two.state["controller_state"].shape == (2, 2 * 200 * 2)
    eo = er = 0.0
    for t in (1, 2):
        r2 = two.track(dframes[t]).cpu().numpy()
        o2 = two.offsets.cpu().numpy()
        r1 = np.concatenate([o.track(dframes[t]).cpu().numpy() for o in ones])
        o1 = np.concatenate([o.offsets.cpu().numpy() for o in ones])
        eo, er = max(eo, np.abs(o2 - o1).max()), max(er, np.abs(r2 - r1).max())
        np.testing.assert_allclose(o2, o1, rtol=0, atol=OFFSET_ATOL)
        np.testing.assert_allclose(r2, r1, rtol=0, atol=REGION_ATOL)
    print("stacked cell, batch of 2 against two batches of 1: max |offset err| %.3g, max |region err| %.3g px" % (eo, er))


def test_output_dim_other_than_two_is_refused(model, cuda):
    from ntmtrack import online, _lib
    from ntmtrack.ntm import NTMCell
    cell = NTMCell(3, mem_size=128, mem_dim=20, controller_hidden_size=200, controller_num_layers=1, write_head_size=1,
                   read_head_size=4, input_dim=514, device=cuda, seed=1)
    with pytest.raises(_lib.NtkError):
        online.BatchNTMTracker(model["dframes"][0], REGIONS, cell, model["vgg"], frame_of=FRAME_OF, device=cuda)
