"""GPU: validation from image files decoded on the device -- ntk_track_decode_mask against the NumPy restatement of its rules
(tests/decode_mask_util.py), and evaluate.validate over file clips with decode="device" against decode="host" and against the
same frames handed over as uint8 arrays (the path that existed before), bit for bit.

Shapes: the validator tests' (tests/test_evaluate_gpu.py: 90 x 120 clips of lengths [2, 3, 6, 4, 5], 64 x 80 clips of lengths
[3, 2, 4], B = 2, T = 2, its NTM 128 x 20 cell and trunk, its smallest one-workgroup DNC core).  The files are written at test
time (tests/validate_files_util.py); every one is inside the decoder's bit-exact domain, asserted per file in the fixture."""
import numpy as np
import pytest
import torch

import decode_mask_util as M
import evaluate_util as U
import validate_files_util as F
from test_evaluate_gpu import (DIST_THR, IOU_THR, REGION_ATOL, assert_one_workgroup_family, assert_table, dnc_maker, ntm_maker,
                               same_bits, world)     # noqa: F401 -- world is a fixture

pytestmark = pytest.mark.gpu

B, T = 2, 2


# --------------------------------------------------------------------------------------------- 1. the kernel against the rules
KT, KB, KCLIPS, KSTATUS = 5, 70, 64, 400


def kernel_case():
    """T = 5, B = 70 (more than one wave).  Slots 0-59 hold clips 59..0, slots 60-69 none (clip_of -1, or a row past the table).
    -> status, cell_index [T,B], start_index [B], clip_of [B], dead [B], active [T,B]"""
    rng = np.random.default_rng(11)
    status = np.zeros(KSTATUS, dtype=np.int32)
    clip_of = np.concatenate([np.arange(59, -1, -1), [-1, KCLIPS, -5, KCLIPS + 3, -1, -1, 2 ** 30, -1, -1, -1]]).astype(np.int32)
    cell_index = rng.permutation(KSTATUS - 20)[:KT * KB].reshape(KT, KB).astype(np.int32)       # distinct files, none of the last 20
    active = (rng.uniform(size=(KT, KB)) < 0.8).astype(np.uint8)                                # inactive frames
    active[:, :12] = 1
    start_index = np.full(KB, -1, dtype=np.int32)
    start_index[0:40:3] = np.arange(KSTATUS - 20, KSTATUS - 20 + len(start_index[0:40:3]))      # these slots are reset this round
    dead = np.zeros(KB, dtype=np.uint8)
    dead[[1, 50]] = 1                                                                           # carried from an earlier round
    dead[3] = 1                                                                                 # cleared: slot 3 restarts on a good frame
    status[start_index[6]] = 2                                                                  # a failed starting frame
    status[start_index[9]] = 1
    status[cell_index[0, 2]] = 2                                                                # failures in the first,
    status[cell_index[2, 4]] = 1                                                                # a middle
    status[cell_index[4, 5]] = 5                                                                # and the last frame
    status[cell_index[1, 7]], status[cell_index[3, 7]] = 3, 2                                   # two in one clip: the first is kept
    cell_index[2, 8] = KSTATUS                                                                  # an index >= n_status: BAD_DESC
    cell_index[1, 10] = KSTATUS + 1000
    cell_index[:, 11] = -1                                                                      # no device file: status 0
    cell_index[3, 2] = -1
    status[cell_index[2, 62]], status[cell_index[0, 61]] = 2, 1                                 # failures in slots without a clip
    start_index[63] = KSTATUS - 1
    status[KSTATUS - 1] = 4
    active[:, 60:] = 1
    return status, cell_index, start_index, clip_of, dead, active


def run_mask(cuda, status, cell_index, start_index, clip_of, dead, active, table):
    """One launch on copies; -> (dead, active, table) as NumPy."""
    from ntmtrack import _lib
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(cuda)
    status, cell_index, start_index, clip_of, dead, active, table = [d(a) for a in (status, cell_index, start_index, clip_of, dead, active, table)]
    P = _lib.ptr
    t, b = active.shape
    _lib.check(_lib.lib().ntk_track_decode_mask(P(status), status.numel(), P(cell_index), P(start_index), P(clip_of), t, b,
                                                KCLIPS, P(dead), P(active), P(table), _lib.stream()), "ntk_track_decode_mask")
    torch.cuda.synchronize()
    return dead.cpu().numpy(), active.cpu().numpy(), table.cpu().numpy()


def test_decode_mask_matches_the_restatement(cuda):
    status, cell_index, start_index, clip_of, dead, active = kernel_case()
    SENT = -77
    table = M.new_table(KCLIPS + 1)                                  # one row more than the kernel is told of
    table[60:] = SENT                                                # rows no slot names, and the row past the table
    w_dead, w_active, w_table = dead.copy(), active.copy(), table.copy()
    M.decode_mask(status, cell_index, start_index, clip_of, KCLIPS, w_dead, w_active, w_table)
    # the cases are in the data as built: the restatement saw each of them
    row = lambda slot: w_table[clip_of[slot]]
    assert w_dead[6] == 1 and w_dead[9] == 1 and w_dead[3] == 0 and w_dead[1] == 1 and w_dead[0] == 0
    assert row(6)[M.START_STATUS] == 2 and row(6)[M.MASKED] == KT and row(6)[M.DECODED] == 0 and row(6)[M.FIRST_FAILED] == -1
    assert row(1)[M.MASKED] == KT and row(1)[M.START_STATUS] == 0                                # dead before this round
    assert row(2).tolist() == [KT - 1, 1, 0, 0, 2, 0] and row(4).tolist() == [KT - 1, 1, 0, 2, 1, 0]
    assert row(5).tolist() == [KT - 1, 1, 0, KT - 1, 5, 0] and row(7).tolist() == [KT - 2, 2, 0, 1, 3, 0]
    assert row(8)[M.FIRST_STATUS] == M.BAD_DESC and row(10)[M.FIRST_STATUS] == M.BAD_DESC and row(10)[M.FIRST_FAILED] == 1
    assert row(11).tolist() == [KT, 0, 0, -1, 0, 0]
    assert (w_active[:, 60:] == 1).all() and (w_dead[60:] == 0).all() and (w_table[60:] == SENT).all()
    assert 0 < w_active.sum() < active.sum() and (active == 0).sum() > 20
    g_dead, g_active, g_table = run_mask(cuda, status, cell_index, start_index, clip_of, dead, active, table)
    assert same_bits(g_dead, w_dead) and same_bits(g_active, w_active) and same_bits(g_table, w_table)
    # two calls over frames [0,2) and [2,5) leave the bits of one call: the second has no starting frames and carries dead
    none = np.full(KB, -1, dtype=np.int32)
    d1, a1, t1 = run_mask(cuda, status, cell_index[:2], start_index, clip_of, dead, active[:2], table)
    d2, a2, t2 = run_mask(cuda, status, cell_index[2:], none, clip_of, d1, active[2:], t1)
    assert same_bits(d2, w_dead) and same_bits(np.concatenate([a1, a2]), w_active) and same_bits(t2, w_table)


# ---------------------------------------------------------------------------------------------------------- the validator
@pytest.fixture(scope="module")
def files(tmp_path_factory):
    """The five 90 x 120 and three 64 x 80 clips as files, their bytes, and the same frames as uint8 arrays (Pillow's)."""
    folder = tmp_path_factory.mktemp("validate_files")
    clips, contents = F.write_clips(folder, F.LENGTHS, F.H, F.W, F.KINDS, 3, check_bits=True)
    clips[2].regions[4] = np.nan                                    # the object is absent in one frame: tracked, not scored
    small, small_contents = F.write_clips(folder, F.SMALL_LENGTHS, F.SMALL_H, F.SMALL_W, F.SMALL_KINDS, 4, check_bits=True)
    return {"folder": folder, "clips": clips, "contents": contents, "arrays": F.array_clips(clips, contents),
            "small": small, "small_contents": small_contents}


def run(maker, clips, cuda, **kw):
    """-> (result, regions per clip, the score table)"""
    from ntmtrack import evaluate as E
    v = E.Validation(maker, clips, B, T, return_regions=True, device=cuda, **kw).finish()
    res = v.scores.result()
    res["decode"] = v.decode_report
    return res, v.regions(), v.scores.table.cpu().numpy()


@pytest.fixture(scope="module")
def ntm_runs(world, cuda, files):                                   # noqa: F811
    """The NTM one-pass validation of the five 90 x 120 clips, computed once per form."""
    maker = ntm_maker(world, cuda)
    return {"device": run(maker, files["clips"], cuda, decode="device"), "host": run(maker, files["clips"], cuda, decode="host"),
            "arrays": run(maker, files["arrays"], cuda)}


def assert_same_run(a, b, what):
    for i, (x, y) in enumerate(zip(a[1], b[1])):
        assert same_bits(x, y), "%s: regions of clip %d differ by %.3g px" % (what, i, np.nanmax(np.abs(x - y)))
    assert same_bits(a[2], b[2]), what + ": score tables differ"


def test_ntm_device_decode_gives_the_bits_of_host_decode_and_of_arrays(ntm_runs, files):
    dev, host, arrays = ntm_runs["device"], ntm_runs["host"], ntm_runs["arrays"]
    assert all(r.shape == (n - 1, 4) and np.isfinite(r).all() for r, n in zip(dev[1], F.LENGTHS))
    assert_same_run(dev, host, "device against host")
    assert_same_run(dev, arrays, "device against uint8 arrays")
    assert arrays[0]["decode"] is None                              # a run without file clips has no decode report
    scored = [n - 1 for n in F.LENGTHS]
    total = sum(F.LENGTHS)
    for res, on_device in ((dev[0], total), (host[0], 0)):
        d = res["decode"]
        assert d["frames_on_device"] == on_device and d["frames_on_host"] == total - on_device
        assert d["clips"]["decoded"].tolist() == scored and d["decoded"] == sum(scored) and d["failed"] == d["masked"] == 0
        assert d["clips"]["first_failed"].tolist() == [-1] * 5 and d["clips"]["start_status"].tolist() == [0] * 5
        assert d["failed_files"] == [] and d["clips_affected"] == 0
    scored[2] -= 1
    assert dev[0]["clips"]["frames"].tolist() == scored and 0 < dev[0]["mean_overlap_frames"] < 1


def test_validate_adds_the_decode_report_only_to_runs_with_file_clips(world, cuda, files, ntm_runs):   # noqa: F811
    from ntmtrack import evaluate as E
    maker = ntm_maker(world, cuda)
    res, regions = E.validate(maker, files["clips"][:2], B, T, return_regions=True, device=cuda, decode="device")
    assert res["decode"]["frames_on_device"] == 5 and res["decode"]["clips"]["decoded"].tolist() == [1, 2]
    assert same_bits(regions[0], ntm_runs["device"][1][0]) and same_bits(regions[1], ntm_runs["device"][1][1])
    plain = E.validate(maker, files["arrays"][:2], B, T, device=cuda, decode="device")           # array clips: decode= changes nothing
    assert "decode" not in plain and sorted(plain) == sorted(k for k in res if k != "decode")
    for k in ("mean_overlap", "mean_centre_error"):
        assert same_bits(plain["clips"][k], res["clips"][k]), k


# ------------------------------------------------------------------------------- 3. supervised, polygon ground truth
SKIP, BURN_IN = 2, 1


def polygon_clips(clips):
    """The clips with 4-point polygon ground truth (a slightly sheared box); clip 2 carries a planted failure: its ground truth, a
    box about a tenth of the frame wide, jumps three box widths along x on frame 1 (tests/test_supervised_gpu.py's recipe: the
    box update cannot follow), so the slot fails there, sits SKIP frames out and is restarted on frame 3."""
    from ntmtrack.evaluate import Clip
    rng = np.random.default_rng(63)
    out = []
    for i, c in enumerate(clips):
        r = c.regions.copy()
        if i == 2:
            r = np.tile(np.array([14.0, 40.0, 12.0, 9.0]), (len(r), 1)) + np.cumsum(rng.uniform(-0.25, 0.25, size=(len(r), 4)), axis=0)
            r[1:, 0] += 36.0
        x, y, w, h = r[:, 0], r[:, 1], r[:, 2], r[:, 3]
        out.append(Clip(c.frames, np.stack([x, y, x + w, y + 1.5, x + w + 1.0, y + h, x + 1.0, y + h - 1.5], axis=1), None, c.size))
    return out


def test_supervised_polygons_device_decode_gives_the_bits_of_host_decode(world, cuda, files):     # noqa: F811
    from ntmtrack import evaluate as E
    clips = polygon_clips(files["clips"])
    maker = ntm_maker(world, cuda)
    kw = dict(return_regions=True, device=cuda, protocol="supervised", skip=SKIP, burn_in=BURN_IN)
    (d_res, d_reg, d_codes), (h_res, h_reg, h_codes) = [E.validate(maker, clips, B, T, decode=m, **kw) for m in ("device", "host")]
    assert d_res["failures"] >= 1 and d_res["restarts"] >= 1 and d_res["skipped"] >= 1 and d_res["valid"] >= 1   # skip and burn_in act
    assert d_codes[2][0] == E.SUP_CODE_FAILURE and d_codes[2][1] == E.SUP_CODE_SKIPPED and d_codes[2][2] == E.SUP_CODE_RESTART
    for i in range(len(clips)):
        assert same_bits(d_reg[i], h_reg[i]) and same_bits(d_codes[i], h_codes[i]), "clip %d" % i
    for k in ("accuracy", "valid", "failures", "restarts", "tracked", "skipped", "first_failure"):
        assert same_bits(d_res["clips"][k], h_res["clips"][k]), k
    assert d_res["decode"]["frames_on_device"] == sum(F.LENGTHS) and h_res["decode"]["frames_on_host"] == sum(F.LENGTHS)


# ------------------------------------------------------------------------------------------------------------- 4. DNC
def test_dnc_device_decode_matches_host_decode(world, cuda, files):                               # noqa: F811
    cores = []
    maker = dnc_maker(world, cuda, cores)
    dev, host = run(maker, files["clips"], cuda, decode="device"), run(maker, files["clips"], cuda, decode="host")
    assert len(cores) == 2
    assert_one_workgroup_family(cores)
    err = max(np.abs(g - w).max() for g, w in zip(dev[1], host[1]))
    print("DNC (seq family): decode=\"device\" against decode=\"host\": max |region err| %.3g px (the launches are the same: 0 expected)" % err)
    assert all(g.shape == w.shape and np.isfinite(g).all() for g, w in zip(dev[1], host[1])) and err <= REGION_ATOL
    assert_table(dev[2], U.score_clips(dev[1], [c.regions for c in files["clips"]], IOU_THR, DIST_THR),
                 "DNC validation table from files against the restatement")
    assert dev[0]["decode"]["frames_on_device"] == sum(F.LENGTHS)


# ----------------------------------------------------------------------------- 5. two frame sizes, files the host decodes
def test_two_frame_sizes_with_a_png_and_a_progressive_file(world, cuda, files, ntm_runs):          # noqa: F811
    from PIL import Image
    from ntmtrack.evaluate import Clip
    import jpeg_util as J
    big, small = [Clip(list(c.frames), c.regions) for c in files["clips"]], files["small"]
    folder = files["folder"]
    png, prog = str(folder / "frame.png"), str(folder / "progressive.jpg")
    Image.fromarray(J.pillow_decode(files["contents"][1][2])).save(png)                            # the same pixels, losslessly
    Image.fromarray(J.image(F.H, F.W, "smooth", 77)).save(prog, "JPEG", quality=90, progressive=True)
    big[1].frames[2] = png
    big[3].frames[0] = prog                                                                        # a starting frame
    mixed = [big[0], small[0], big[1], big[2], small[1], big[3], small[2], big[4]]
    where_big, where_small = [0, 2, 3, 5, 7], [1, 4, 6]
    maker = ntm_maker(world, cuda)
    dev, host = run(maker, mixed, cuda, decode="device"), run(maker, mixed, cuda, decode="host")
    assert_same_run(dev, host, "two sizes, device against host")
    d = dev[0]["decode"]
    total = sum(F.LENGTHS) + sum(F.SMALL_LENGTHS)
    assert d["frames_on_host"] == 2 and d["frames_on_device"] == total - 2 and d["failed"] == 0 and d["masked"] == 0
    assert d["clips"]["decoded"].tolist() == [1, 2, 2, 5, 1, 3, 3, 4]                              # in input order
    assert dev[0]["clips"]["frames"].tolist() == [1, 2, 2, 4, 1, 3, 3, 4]
    # the clips no file of which was replaced are the clips of the one-size run, row for row (the PNG holds the JPEG's pixels)
    for j, i in enumerate(where_big):
        if j != 3:
            assert same_bits(dev[1][i], ntm_runs["device"][1][j]) and same_bits(dev[2][i], ntm_runs["device"][2][j]), "90 x 120 clip %d" % j
    alone = run(maker, small, cuda, decode="device")
    for j, i in enumerate(where_small):
        assert same_bits(dev[1][i], alone[1][j]) and same_bits(dev[2][i], alone[2][j]), "64 x 80 clip %d" % j


# ------------------------------------------------------------------------------------- 6. prefetch and synchronisation
def test_prefetch_depth_does_not_change_the_bits(world, cuda, files, ntm_runs):                    # noqa: F811
    maker = ntm_maker(world, cuda)
    one = run(maker, files["clips"], cuda, decode="device", prefetch=1, workers=1)
    assert_same_run(one, ntm_runs["device"], "prefetch=1 against prefetch=2")


def test_device_decode_rounds_after_the_first_do_not_synchronise(world, cuda, files):              # noqa: F811
    """As tests/test_evaluate_gpu.py's test of the same name.  The one host wait of the path, the prefetcher's wait for the event
    behind the uploads from the pinned set it refills (Event.synchronize), is made inside these rounds and is not reported by the
    sync debug mode, which watches the synchronising calls of torch's own operators: nothing is exempted here."""
    from ntmtrack import evaluate as E
    v = E.Validation(ntm_maker(world, cuda), files["clips"], B, T, device=cuda, decode="device")
    assert v.step()                                                 # builds the tracker, its plans and workspaces
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    rounds = 0
    try:
        while v.step():
            rounds += 1
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert rounds == 4
    scored = [n - 1 for n in F.LENGTHS]
    scored[2] -= 1
    assert v.finish().scores.result()["clips"]["frames"].tolist() == scored
    assert v.decode_report["frames_on_device"] == sum(F.LENGTHS)


# ------------------------------------------------------------------------------------------------- 7. undecodable frames
def with_file(files, clip, frame, data, name):
    """The 90 x 120 file clips with `data` written as `name` in place of one frame."""
    from ntmtrack.evaluate import Clip
    path = str(files["folder"] / name)
    with open(path, "wb") as f:
        f.write(data)
    clips = [Clip(list(c.frames), c.regions) for c in files["clips"]]
    clips[clip].frames[frame] = path
    return clips, path


def test_a_truncated_tracked_frame_is_skipped_and_reported(world, cuda, files, ntm_runs):          # noqa: F811
    from ntmtrack import _lib, evaluate as E
    clips, path = with_file(files, 2, 3, F.truncated(F.H, F.W, 3), "cut_tracked.jpg")
    maker = ntm_maker(world, cuda)
    res, regions, table = run(maker, clips, cuda, decode="device", on_undecoded="skip")
    clean_res, clean_regions, clean_table = ntm_runs["device"]
    assert np.isnan(regions[2][2]).all() and np.isfinite(regions[2][[0, 1, 3, 4]]).all()           # frame 3 is tracked frame 2
    assert same_bits(regions[2][:2], clean_regions[2][:2])                                         # the clip's earlier frames
    for i in (0, 1, 3, 4):
        assert same_bits(regions[i], clean_regions[i]) and same_bits(table[i], clean_table[i]), "clip %d" % i
    want = clean_res["clips"]["frames"].copy()
    want[2] -= 1                                                                                   # its clip scores one frame fewer
    assert res["clips"]["frames"].tolist() == want.tolist() and res["frames"] == clean_res["frames"] - 1
    d = res["decode"]
    assert d["failed"] == 1 and d["masked"] == 0 and d["clips"]["failed"].tolist() == [0, 0, 1, 0, 0]
    assert d["clips"]["decoded"].tolist() == [1, 2, 4, 3, 4]
    assert d["clips"]["first_failed"].tolist() == [-1, -1, 2, -1, -1] and d["clips"]["first_status"].tolist() == [0, 0, 2, 0, 0]
    assert d["failed_files"] == [path] and d["clips_affected"] == 1
    # the default raises at finish(), naming the file and the status
    v = E.Validation(maker, clips, B, T, device=cuda, decode="device")
    with pytest.raises(_lib.NtkError) as e:
        v.finish()
    assert path in str(e.value) and "status 2" in str(e.value)


def test_a_truncated_starting_frame_masks_its_clip(world, cuda, files, ntm_runs):                  # noqa: F811
    clips, path = with_file(files, 2, 0, F.truncated(F.H, F.W, 4), "cut_start.jpg")
    res, regions, table = run(ntm_maker(world, cuda), clips, cuda, decode="device", on_undecoded="skip")
    _clean_res, clean_regions, clean_table = ntm_runs["device"]
    assert res["clips"]["frames"][2] == 0 and res["clips_without_frames"] == 1 and np.isnan(regions[2]).all()
    d = res["decode"]
    assert d["clips"]["masked"].tolist() == [0, 0, F.LENGTHS[2] - 1, 0, 0] and d["clips"]["start_status"].tolist() == [0, 0, 2, 0, 0]
    assert d["clips"]["decoded"][2] == 0 and d["failed"] == 0 and d["failed_files"] == [path]
    for i in (0, 1, 3, 4):
        assert same_bits(regions[i], clean_regions[i]) and same_bits(table[i], clean_table[i]), "clip %d" % i


# ----------------------------------------------------------------------------------------------------- 8. bad arguments
def test_bad_arguments(world, cuda, files):                                                        # noqa: F811
    from ntmtrack import evaluate as E
    from ntmtrack.evaluate import Clip
    maker = ntm_maker(world, cuda)
    floats = [Clip(c.frames.astype(np.float32), c.regions) for c in files["arrays"][:2]]
    for decode in ("device", "host"):
        with pytest.raises(ValueError, match="file clips"):
            E.Validation(maker, floats + files["clips"][2:3], B, T, device=cuda, decode=decode)
    # a file of another size raises at its round: round 1 (clips 0 and 1) runs, round 2 needs the file
    clips = [Clip(list(c.frames), c.regions, None, (F.H, F.W)) for c in files["clips"]]
    clips[2].frames[2] = files["small"][0].frames[0]
    for decode in ("device", "host"):
        v = E.Validation(maker, clips, B, T, device=cuda, decode=decode)
        assert v.step()
        with pytest.raises(ValueError) as e:
            v.step()
        assert clips[2].frames[2] in str(e.value) and "64x80" in str(e.value) and "90x120" in str(e.value)
        v.close()
