"""CPU: the host side of polygon ground truth -- data.vot_clips on a VOT tree written into tmp_path, evaluate.write_trajectory
against the expected text, the host helpers of evaluate (padding, 4-gons, bounds) and the NumPy restatement the GPU tests compare
with (tests/poly_util.py) against closed forms."""
import os

import numpy as np
import pytest

import poly_util as P

L_SHAPE = [(0, 0), (40, 0), (40, 10), (10, 10), (10, 40), (0, 40)]
SQUARE = [(0, 0), (1, 0), (1, 1), (0, 1)]


# ------------------------------------------------------------------------------------------------------------- vot_clips
def write_vot_tree(root):
    """Two sequences of 32 x 48 (H x W) frames: ``boxes`` has 4-number lines and its frames in color/, ``quads`` has 8-number lines
    (one line unparsable, one a 4-number line) and its frames in the sequence folder."""
    from PIL import Image
    rng = np.random.default_rng(3)
    os.makedirs(os.path.join(root, "boxes", "color"))
    os.makedirs(os.path.join(root, "quads"))
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write("boxes\nquads\n")
    boxes = [[5.5, 6.0, 20.0, 10.25], [6.0, 6.5, 20.0, 10.0], [7.0, 7.0, 19.5, 10.0]]
    quads = [[10.0, 5.0, 30.5, 8.0, 28.0, 20.0, 8.0, 17.25], None, [4.0, 3.0, 12.0, 9.0], [11.0, 6.0, 31.0, 9.0, 29.0, 21.0, 9.0, 18.0]]
    with open(os.path.join(root, "boxes", "groundtruth.txt"), "w") as f:
        f.write("".join(",".join(repr(v) for v in r) + "\n" for r in boxes))
    with open(os.path.join(root, "quads", "groundtruth.txt"), "w") as f:
        f.write("".join(("nan,1,2\n" if r is None else ",".join(repr(v) for v in r) + "\n") for r in quads))
    for name, sub, n in (("boxes", "color", len(boxes)), ("quads", "", len(quads))):
        for i in range(n):
            Image.fromarray(rng.integers(0, 256, size=(32, 48, 3), dtype=np.uint8)).save(os.path.join(root, name, sub, "%08d.jpg" % (i + 1)))
    return boxes, quads


def test_vot_clips_reads_both_layouts_and_both_region_forms(tmp_path, monkeypatch):
    from ntmtrack import data, evaluate as E
    boxes, quads = write_vot_tree(str(tmp_path))
    decoded = []
    real = data._decode_image
    monkeypatch.setattr(data, "_decode_image", lambda path: decoded.append(path) or real(path))
    clips = data.vot_clips(str(tmp_path))
    assert len(clips) == 2 and all(isinstance(c, E.Clip) for c in clips)
    assert decoded == []                                            # lazy: nothing decoded until the validator asks
    a, b = clips
    assert a.regions.shape == (3, 4) and a.regions.dtype == np.float64 and a.regions.tolist() == boxes
    assert b.regions.shape == (4, E.POLY_DOUBLES)
    assert b.regions[0, :8].tolist() == quads[0] and np.isnan(b.regions[0, 8:]).all()
    assert np.isnan(b.regions[1]).all()                             # the unparsable line: an absent object
    assert b.regions[2, :8].tolist() == [4.0, 3.0, 16.0, 3.0, 16.0, 12.0, 4.0, 12.0] and np.isnan(b.regions[2, 8:]).all()
    assert b.regions[3, :8].tolist() == quads[3]
    assert a.size == (32, 48) and b.size == (32, 48) and a.init is None and b.init is None
    fa, fb = a.frames(), b.frames()
    assert fa.shape == (3, 32, 48, 3) and fb.shape == (4, 32, 48, 3) and fa.dtype == np.float32
    assert [os.path.relpath(p, str(tmp_path)) for p in decoded] == \
        [os.path.join("boxes", "color", "%08d.jpg" % i) for i in (1, 2, 3)] + [os.path.join("quads", "%08d.jpg" % i) for i in (1, 2, 3, 4)]
    # names= picks and orders the sequences without list.txt
    os.remove(os.path.join(str(tmp_path), "list.txt"))
    only = data.vot_clips(str(tmp_path), names=["quads"])
    assert len(only) == 1 and only[0].regions.shape == (4, E.POLY_DOUBLES)


def test_parse_vot_region_takes_the_two_forms():
    from ntmtrack import data
    assert data.parse_vot_region("1,2,3,4\n") == [1.0, 2.0, 3.0, 4.0]
    assert data.parse_vot_region("1,2,3,4,5,6") == [1.0, 2.0, 3.0, 4.0, 5.0, 6.0]
    for bad in ("", "1,2,3", "1,2,3,4,5", "a,b,c,d", "1,2,,4"):
        assert data.parse_vot_region(bad) is None
    with pytest.raises(ValueError):
        data.parse_vot_region(",".join(["1"] * 18))


# ------------------------------------------------------------------------------------------------------- write_trajectory
def test_write_trajectory_writes_codes_and_regions(tmp_path):
    from ntmtrack import evaluate as E
    regions = np.array([[10.0, 20.5, 30.25, 40.125], [11.0, 21.0, 30.0, 40.0], [np.nan] * 4, [np.nan] * 4, [50.0, 60.0, 7.0, 8.0],
                        [50.12346, 60.0, 7.0, 8.99996]])
    codes = np.array([0, 2, 3, 3, 1, 0], dtype=np.int8)             # tracked, failure, sat out twice, restart, tracked
    path = str(tmp_path / "clip_001.txt")
    E.write_trajectory(path, [9.0, 19.0, 30.0, 40.0], regions, codes)
    assert open(path).read() == "1\n10.0000,20.5000,30.2500,40.1250\n2\n0\n0\n1\n50.1235,60.0000,7.0000,9.0000\n"
    E.write_trajectory(path, [9.0, 19.0, 30.0, 40.0], regions[[0, 1, 4]])
    assert open(path).read() == "1\n10.0000,20.5000,30.2500,40.1250\n11.0000,21.0000,30.0000,40.0000\n50.0000,60.0000,7.0000,8.0000\n"
    with pytest.raises(ValueError):
        E.write_trajectory(path, [9.0, 19.0, 30.0], regions, codes)
    with pytest.raises(ValueError):
        E.write_trajectory(path, [9.0, 19.0, 30.0, 40.0], regions, codes[:3])


# ---------------------------------------------------------------------------------------------------- evaluate's host helpers
def test_padding_four_gons_and_host_bounds():
    from ntmtrack import evaluate as E
    tri = np.array([[0.0, 0.0, 4.0, 0.0, 0.0, 3.0]])
    padded = E.pad_polygons(tri)
    assert padded.shape == (1, 16) and padded[0, :6].tolist() == tri[0].tolist() and np.isnan(padded[0, 6:]).all()
    for cols in (4, 5, 7, 18):
        with pytest.raises(ValueError):
            E.pad_polygons(np.zeros((2, cols)))
    rects = np.array([[2.0, 3.0, 10.0, 5.0], [np.nan, 3.0, 10.0, 5.0], [2.0, 3.0, 0.0, 5.0], [2.0, 3.0, -4.0, 5.0]])
    gons = E.rect_polygons(rects)
    assert gons[0, :8].tolist() == [2.0, 3.0, 12.0, 3.0, 12.0, 8.0, 2.0, 8.0] and np.isnan(gons[0, 8:]).all()
    assert np.isnan(gons[1:]).all()                                 # an absent rectangle stays absent, a negative width too
    regions = np.stack([P.pad(P.rotated_rect(-30.0, -20.0, 12.0, 9.0, 0.35)), P.pad([(0, 0), (5, 5)]), P.pad([(0, 0), (5, 5), (9, 9)]),
                        P.pad(L_SHAPE), gons[0]])
    got, want = E.polygon_bounds(regions), P.bounds_array(regions)
    assert got.shape == (5, 4) and got.tobytes() == want.tobytes()
    assert np.isnan(got[1]).all() and np.isnan(got[2]).all() and got[3].tolist() == [0.0, 0.0, 40.0, 40.0] and got[4].tolist() == rects[0].tolist()
    assert got[0, 0] < 0 and got[0, 0] + got[0, 2] < 0             # all coordinates negative: the true maximum, not the reference's seed


def test_validation_converts_regions_once(monkeypatch):
    """The bookkeeping of Validation's constructor, which needs no device: a run without a polygon clip keeps [L,4]; with one, every
    clip holds [L,16] and starts from its first region's bounding rectangle."""
    from ntmtrack import evaluate as E
    monkeypatch.setattr(E, "OverlapScores", lambda *a, **k: None)
    frames = np.zeros((3, 8, 8, 3), dtype=np.uint8)
    box = np.array([[1.0, 2.0, 3.0, 4.0], [1.5, 2.0, 3.0, 4.0], [np.nan] * 4])
    quad = np.stack([np.asarray(P.rotated_rect(4.0, 4.0, 3.0, 2.0, t)).reshape(-1) for t in (0.1, 0.2, 0.3)])
    v = E.Validation(None, [E.Clip(frames, box)], 1, 1, device="cpu")
    assert not v.polygons and v._gt[0].shape == (3, 4) and v._init_region(0).tolist() == box[0].tolist()
    v = E.Validation(None, [E.Clip(frames, box), E.Clip(frames, quad)], 1, 1, device="cpu")
    assert v.polygons and v._gt[0].shape == (3, 16) and v._gt[1].shape == (3, 16)
    assert v._gt[0][0, :8].tolist() == [1.0, 2.0, 4.0, 2.0, 4.0, 6.0, 1.0, 6.0] and np.isnan(v._gt[0][2]).all()
    assert v._init_region(0).tolist() == box[0].tolist()
    assert v._init_region(1).tobytes() == P.bounds(P.pad(quad[0])).tobytes()
    assert E.Validation(None, [E.Clip(frames, quad, init=(0.1, 0.2, 0.3, 0.4))], 1, 1, device="cpu")._init_region(0).tolist() == [0.1, 0.2, 0.3, 0.4]


# ------------------------------------------------------------------------------------- the restatement against closed forms
@pytest.mark.parametrize("rect,want", [((0, 0, 1, 1), 1.0),                    # itself
                                       ((0.5, 0, 1, 1), 0.5 / 1.5),             # half a square shared
                                       ((0.5, 0.5, 1, 1), 0.25 / 1.75),         # a quarter
                                       ((0.25, 0.25, 0.5, 0.5), 0.25),          # the rectangle inside the square
                                       ((-1, -1, 3, 3), 1.0 / 9.0),             # the square inside the rectangle
                                       ((1, 0, 1, 1), 0.0),                     # touching along a side
                                       ((1, 1, 1, 1), 0.0),                     # touching in a corner
                                       ((2, 2, 1, 1), 0.0),                     # apart
                                       ((0.25, 0.25, 0.0, 0.5), 0.0)])          # a rectangle without width
@pytest.mark.parametrize("flip", [False, True])
def test_unit_square_cases(rect, want, flip):
    g = P.pad(SQUARE[::-1] if flip else SQUARE)
    got = P.poly_iou(rect, g)
    assert got == want if want in (0.0, 1.0, 0.25) else abs(got - want) <= 1e-15


def test_l_shape_and_rotated_square():
    g = P.pad(L_SHAPE)
    assert P.area(P.vertices(g)) == 700.0
    assert P.poly_iou((5, 5, 30, 30), g) == 275.0 / 1325.0
    assert P.poly_iou((5, 5, 30, 30), P.pad(L_SHAPE[::-1])) == 275.0 / 1325.0
    assert P.poly_iou((15, 15, 20, 20), g) == 0.0                   # the rectangle sits in the notch: bounding boxes overlap, shapes do not
    diamond = P.pad([(10, 0), (20, 10), (10, 20), (0, 10)])          # a square turned by 45 degrees against its own bounding box
    assert P.bounds(diamond).tolist() == [0.0, 0.0, 20.0, 20.0]
    assert P.poly_iou(P.bounds(diamond), diamond) == 0.5


def test_present_rules_and_integer_boxes_against_rect_iou():
    import evaluate_util as U
    assert P.bounds(P.pad([(0, 0), (5, 5)])) is None                 # 2 vertices
    assert P.bounds(P.pad([(0, 0), (5, 5), (9, 9)])) is None         # collinear: area 0
    assert P.bounds(P.pad([(0, 3), (5, 3), (9, 3)])) is None         # no height
    g = P.pad(SQUARE)
    g[0] = np.nan
    assert P.bounds(g) is None and P.frame_score((0, 0, 1, 1), g) is None      # the first pair is not finite: no vertex at all
    g = P.pad(SQUARE + [(7, 7)])
    g[6] = np.inf                                                    # the fourth pair ends the list: the fifth is never read
    assert len(P.vertices(g)) == 3 and P.bounds(g).tolist() == [0.0, 0.0, 1.0, 1.0]
    rng = np.random.default_rng(5)
    a = np.concatenate([rng.integers(0, 300, (200, 2)), rng.integers(1, 150, (200, 2))], axis=1).astype(np.float64)
    b = a + rng.integers(-40, 41, (200, 4))
    b[:, 2:] = np.maximum(b[:, 2:], 0)
    got = np.array([P.poly_iou(p, P.pad(P.rect_points(g_))) for p, g_ in zip(b, a)])
    want = np.array([U.rect_iou(p, g_) for p, g_ in zip(b, a)])
    assert got.tobytes() == want.tobytes() and (want > 0).sum() >= 50 and (want == 0).sum() >= 1
    # the score of a frame: the distance goes to the centre of the bounding rectangle
    iou, dist = P.frame_score((0, 0, 20, 20), P.pad([(10, 0), (20, 10), (10, 20), (0, 10)]))
    assert iou == 0.5 and dist == 0.0
    assert P.frame_score((np.nan, 0, 20, 20), P.pad(SQUARE)) == (0.0, np.inf)
