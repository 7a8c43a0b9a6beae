"""CPU: the host side of the mask ground truth -- evaluate.MaskRegions (encode, decode, the device layout of a slice of frames),
evaluate.mask_bounds against the raster restatement (tests/mask_util.py), data.parse_vot_mask and data.vot_clips on a mask
directory written here, and Validation's refusal of a mask clip beside another (raised before anything touches a device)."""
import os

import numpy as np
import pytest

import mask_util as M


def random_masks(rng, L, H, W):
    """Blobs, stripes and speckle; frame 2 (when there is one) all zero."""
    masks = np.zeros((L, H, W), dtype=bool)
    for i in range(L):
        kind = i % 3
        if kind == 0:
            masks[i] = rng.random((H, W)) < 0.3
        elif kind == 1:
            y, x = np.mgrid[:H, :W]
            cy, cx, ry, rx = rng.uniform(0.3, 0.7) * H, rng.uniform(0.3, 0.7) * W, rng.uniform(0.2, 0.45) * H + 0.5, rng.uniform(0.2, 0.45) * W + 0.5
            masks[i] = ((y + 0.5 - cy) / ry) ** 2 + ((x + 0.5 - cx) / rx) ** 2 <= 1
        else:
            masks[i, rng.integers(0, H // 2 + 1):, ::int(rng.integers(1, 4))] = True
    if L > 2:
        masks[2] = False
    return masks


def test_encode_and_decode_round_trip():
    from ntmtrack.evaluate import MaskRegions
    rng = np.random.default_rng(3)
    for H, W, L in ((64, 96, 7), (1, 9, 4), (11, 1, 4), (5, 5, 3)):
        masks = random_masks(rng, L, H, W)
        masks[0, 0, 0] = masks[0, H - 1, W - 1] = True            # the tight box is the frame: first count 0, no trailing zeros
        regions = MaskRegions.from_arrays(masks)
        assert len(regions) == L and regions.boxes.dtype == np.int32 and regions.counts.dtype == np.int32
        assert regions.offsets.tolist()[0] == 0 and regions.offsets[-1] == len(regions.counts)
        for i in range(L):
            assert (regions.dense(i, H, W) == masks[i]).all(), (H, W, i)
            x0, y0, w, h, counts = regions.frame(i)
            if masks[i].any():
                cols, rows = np.nonzero(masks[i].any(axis=0))[0], np.nonzero(masks[i].any(axis=1))[0]
                assert (x0, y0, w, h) == (cols[0], rows[0], cols[-1] + 1 - cols[0], rows[-1] + 1 - rows[0])     # a tight box
                assert (counts >= 0).all() and counts.sum() <= w * h and len(counts) % 2 == 0
            else:
                assert w == 0 and h == 0 and len(counts) == 0
        assert regions.frame(0)[4][0] == 0
        # the restatement decodes the same pixels from the device layout of any slice
        cells, counts = regions.cells(1, L)
        assert cells.shape == (L - 1, 6) and cells.dtype == np.int32 and cells[0, 4] == 0
        assert cells[-1, 4] + cells[-1, 5] == len(counts)
        for k in range(L - 1):
            m = M.decode(cells[k], counts)
            if masks[k + 1].any():
                x0, y0, img = m
                frame = np.zeros((H, W), dtype=bool)
                frame[y0:y0 + img.shape[0], x0:x0 + img.shape[1]] = img
                assert (frame == masks[k + 1]).all()
            else:
                assert m is None


def test_dense_follows_the_counts_rules():
    from ntmtrack.evaluate import MaskRegions, mask_bounds
    r = MaskRegions.from_lists([(1, 1, 4, 3, [5, 20]),              # counts that run past w h are dropped
                                (0, 0, 8, 6, [4, 5]),               # counts that stop short: the rest is zero
                                (3, 1, 6, 5, [2, 3, 0, 4, 5, 0, 0, 2]),      # zero-length runs
                                (2, 2, 3, 3, [1, 2, -1, 3]),        # a negative count: absent
                                (-2, -1, 4, 3, [0, 12]),            # partly outside the frame
                                None])
    want = np.zeros((6, 8, 10), dtype=bool)
    box = np.zeros(12, dtype=bool); box[5:] = True
    want[0, 1:4, 1:5] = box.reshape(3, 4)
    box = np.zeros(48, dtype=bool); box[4:9] = True
    want[1, 0:6, 0:8] = box.reshape(6, 8)
    box = np.zeros(30, dtype=bool); box[2:9] = True; box[14:16] = True
    want[2, 1:6, 3:9] = box.reshape(5, 6)
    want[4, 0:2, 0:2] = True
    for i in range(6):
        assert (r.dense(i, 8, 10) == want[i]).all(), i
    assert np.isnan(mask_bounds(r, 3)).all() and np.isnan(mask_bounds(r, 5)).all()


def test_mask_bounds_match_the_raster():
    from ntmtrack.evaluate import MaskRegions, mask_bounds
    rng = np.random.default_rng(8)
    masks = random_masks(rng, 9, 40, 56)
    regions = MaskRegions.from_arrays(masks)
    frames = [regions.frame(i) for i in range(len(regions))]
    frames += [(5, 3, 1, 7, [2, 3]), (4, 6, 9, 1, [3, 4]), (7, 8, 1, 1, [0, 1]), (2, 2, 5, 4, [0, 3, 4, 2]), (3, 3, 5, 5, [3, 10]),
               (1, 1, 4, 3, [5, 20]), (0, 0, 6, 4, [2, 4]), (-7, -9, 6, 4, [1, 1, 9, 2]), (3, 3, 4, 4, [16]), (3, 3, 4, 4, []),
               (3, 3, 4, 4, [2, 0, 5, 0]), (3, 3, 4, 4, [2, 3, -1, 4]), (3, 3, 0, 4, [0, 4]), (3, 3, 4, -1, [0, 4]),
               (0, 0, 65536, 32768, [0, 5])]
    regions = MaskRegions.from_lists(frames)
    got = mask_bounds(regions)
    assert got.shape == (len(frames), 4) and got.dtype == np.float64
    present = 0
    for i in range(len(regions)):
        cells, counts = regions.cells(i, i + 1)
        want = M.bounds(cells[0], counts)
        if want is None:
            assert np.isnan(got[i]).all(), i
        else:
            present += 1
            assert got[i].tobytes() == want[0].tobytes(), (i, got[i], want[0])
            assert (mask_bounds(regions, i) == got[i]).all()
    assert present == len(frames) - 1 - 7 and np.isnan(got[2]).all()         # frame 2 is all zero, the last seven are absent by rule


GOOD = [("m 3,4,5,6,0,7,2,1", (3, 4, 5, 6, [0, 7, 2, 1])), ("m-3,-4,5,6", (-3, -4, 5, 6, [])), ("m 1, 2, 3, 4, 5 ,6\n", (1, 2, 3, 4, [5, 6])),
        ("  m 0,0,32768,32768,9", (0, 0, 32768, 32768, [9])), ("m 1,1,0,5,3", (1, 1, 0, 5, [3]))]
BAD = [("m 1,2,3", "at least"), ("m", "at least"), ("m 1,2,3,4,5.5", "not an integer"), ("m 1,2,x,4", "not an integer"),
       ("m 1,2,3,4,,5", "not an integer"), ("m 1,2,3,4,5,-6", "negative count"), ("m 0,0,65536,32768,1", "at most"),
       ("1,2,3,4", "does not begin"), ("m 1,2,3,4,99999999999", "32 bits")]


@pytest.mark.parametrize("line,want", GOOD)
def test_parse_vot_mask_accepts(line, want):
    from ntmtrack.data import parse_vot_mask
    got = parse_vot_mask(line)
    assert tuple(got[:4]) == want[:4] and got[4].dtype == np.int32 and got[4].tolist() == want[4]


@pytest.mark.parametrize("line,reason", BAD)
def test_parse_vot_mask_refuses_with_the_reason(line, reason):
    from ntmtrack.data import parse_vot_mask
    with pytest.raises(ValueError, match=reason):
        parse_vot_mask(line)


def test_parse_vot_region_still_reads_a_mask_line_as_none():
    from ntmtrack.data import parse_vot_region
    assert parse_vot_region("m 3,4,5,6,0,7") is None and parse_vot_region("1,2,3,4") == [1.0, 2.0, 3.0, 4.0]


def write_mask_directory(root, name, regions, frames, sub="color", extra=None):
    """A VOT sequence folder: groundtruth.txt with one ``m`` line per frame (an empty line for an absent object, ``extra``
    {line index: text} in place of some) and the frames as JPEG files numbered from 1."""
    from PIL import Image
    os.makedirs(os.path.join(root, name, sub))
    lines = []
    for i in range(len(regions)):
        x0, y0, w, h, counts = regions.frame(i)
        lines.append("" if w == 0 else "m %s" % ",".join(str(int(v)) for v in [x0, y0, w, h] + list(counts)))
    for k, text in (extra or {}).items():
        lines[k] = text
    with open(os.path.join(root, name, "groundtruth.txt"), "w") as f:
        f.write("\n".join(lines) + "\n")
    for i, image in enumerate(frames):
        Image.fromarray(image).save(os.path.join(root, name, sub, "%08d.jpg" % (i + 1)))


def test_vot_clips_reads_a_mask_directory(tmp_path):
    from ntmtrack import data
    from ntmtrack.evaluate import MaskRegions
    rng = np.random.default_rng(5)
    H, W, L = 24, 40, 5
    masks = random_masks(rng, L, H, W)                               # frame 2 is absent
    regions = MaskRegions.from_arrays(masks)
    frames = rng.integers(0, 256, size=(L, H, W, 3), dtype=np.uint8)
    write_mask_directory(str(tmp_path), "a", regions, frames)
    write_mask_directory(str(tmp_path), "b", regions, frames, sub="", extra={3: "nonsense"})
    with open(os.path.join(str(tmp_path), "list.txt"), "w") as f:
        f.write("a\nb\n")
    for frames_as in ("arrays", "files"):
        clips = data.vot_clips(str(tmp_path), frames=frames_as)
        assert len(clips) == 2 and all(isinstance(c.regions, MaskRegions) and len(c.regions) == L and c.size == (H, W) for c in clips)
        for i in range(L):
            assert (clips[0].regions.dense(i, H, W) == masks[i]).all()
            assert (clips[1].regions.dense(i, H, W) == (masks[i] if i != 3 else False)).all()    # an unparseable line: absent
    assert clips[0].regions.counts.tolist() == regions.counts.tolist()                           # the counts as they are written
    # rectangle directories read as before
    write_mask_directory(str(tmp_path), "r2", regions, frames, extra={i: "1,2,3,4" for i in range(L)})
    assert data.vot_clips(str(tmp_path), names=["r2"])[0].regions.shape == (L, 4)


@pytest.mark.parametrize("text", ["10,12,30,20", "1,1,9,1,9,9,1,9"])
def test_a_rectangle_or_polygon_among_mask_lines_is_refused(tmp_path, text):
    from ntmtrack import data
    from ntmtrack.evaluate import MaskRegions
    rng = np.random.default_rng(6)
    regions = MaskRegions.from_arrays(random_masks(rng, 4, 16, 16))
    write_mask_directory(str(tmp_path), "s", regions, rng.integers(0, 256, size=(4, 16, 16, 3), dtype=np.uint8), extra={1: text})
    with pytest.raises(ValueError, match=r"groundtruth\.txt, line 2: a rectangle or polygon among mask lines"):
        data.vot_clips(str(tmp_path), names=["s"])
    # a bad mask line names its file and line too
    write_mask_directory(str(tmp_path), "t", regions, rng.integers(0, 256, size=(4, 16, 16, 3), dtype=np.uint8), extra={3: "m 1,2,3,4,-5"})
    with pytest.raises(ValueError, match=r"groundtruth\.txt, line 4: .*negative count"):
        data.vot_clips(str(tmp_path), names=["t"])


def test_a_mask_clip_beside_another_clip_is_refused_and_named():
    """Raised by Validation's constructor before a tracker is made or a device is touched."""
    from ntmtrack import evaluate as E
    rng = np.random.default_rng(7)
    masks = E.MaskRegions.from_arrays(random_masks(rng, 3, 16, 16))
    frames = np.zeros((3, 16, 16, 3), dtype=np.uint8)
    clips = [E.Clip(frames, np.tile([2.0, 2.0, 5.0, 5.0], (3, 1))), E.Clip(frames, masks), E.Clip(frames, masks)]
    with pytest.raises(ValueError, match=r"clips \[1, 2\] have mask regions and clips \[0\] have not"):
        E.Validation(lambda *a: None, clips, 2, 2, device="cpu")
