"""CPU: the host side of validation from image files -- the clip readers' frames="files", the round staging (data.stage_round)
against ClipSchedule, pack_jpeg_frames' offsets, and the C ABI of ntk_track_decode_mask (exported, bound, refuses null pointers and
bad sizes before anything is launched; ntk_jpeg_parse is host code, so no GPU is needed anywhere here)."""
import ctypes
import os
import re

import numpy as np
import pytest

import jpeg_util as J
import validate_files_util as F
from test_evaluate_host import write_record
from test_polygon_host import write_vot_tree

ONE = ctypes.c_void_p(16)                       # non-null, aligned, never dereferenced: the checks fire first


# ------------------------------------------------------------------------------------------------------------ clip readers
def test_vot_clips_as_files(tmp_path):
    from ntmtrack import data
    write_vot_tree(str(tmp_path))
    default, files = data.vot_clips(str(tmp_path)), data.vot_clips(str(tmp_path), frames="files")
    assert all(callable(c.frames) for c in default)                 # the default is today's
    assert all(callable(c.frames) for c in data.vot_clips(str(tmp_path), frames="arrays"))
    assert len(files) == len(default) == 2
    for d, f, (name, sub, n) in zip(default, files, (("boxes", "color", 3), ("quads", "", 4))):
        assert isinstance(f.frames, list)
        assert f.frames == [os.path.join(str(tmp_path), name, sub, "%08d.jpg" % (i + 1)) for i in range(n)]
        assert f.size == d.size == (32, 48) and f.init is None and d.init is None
        assert np.array_equal(f.regions, d.regions, equal_nan=True) and f.regions.dtype == d.regions.dtype
    with pytest.raises(ValueError, match="frames"):
        data.vot_clips(str(tmp_path), frames="paths")


def test_validation_clips_as_files(tmp_path):
    from PIL import Image
    from ntmtrack import data
    rng = np.random.default_rng(4)
    root, W, H = tmp_path / "seqs" / "val_seq_0", 40, 24
    os.makedirs(str(root))
    boxes = [(0.2, 0.3, 0.25, 0.2), (0.25, 0.3, 0.25, 0.25), (0.3, 0.35, 0.2, 0.25)]
    for i, box in enumerate(boxes):
        Image.fromarray(rng.integers(0, 256, size=(H, W, 3), dtype=np.uint8)).save(str(tmp_path / ("f%d.png" % i)))
        write_record(str(root), "%06d" % i, box, "f%d.png" % i)
    _all, _train, val = data.get_valid_sequences(str(tmp_path / "seqs"), 3)
    (d,), (f,) = data.validation_clips(val, image_root=str(tmp_path)), data.validation_clips(val, image_root=str(tmp_path), frames="files")
    assert callable(d.frames) and f.frames == [str(tmp_path / ("f%d.png" % i)) for i in range(3)]
    assert f.size == d.size == (H, W) and f.init == d.init and np.array_equal(f.regions, d.regions)
    with pytest.raises(ValueError, match="frames"):
        data.validation_clips(val, image_root=str(tmp_path), frames=None)


def test_bad_decode_and_on_undecoded_values_are_refused(tmp_path):
    from ntmtrack import data, evaluate as E
    clips, _c = F.write_clips(tmp_path, [2], F.SMALL_H, F.SMALL_W, F.SMALL_KINDS, 1)
    assert data.DECODE_MODES == ("host", "device")
    for kw in ({"decode": "gpu"}, {"decode": None}, {"on_undecoded": "ignore"}, {"prefetch": 0}):
        with pytest.raises(ValueError):
            E.Validation(None, clips, 2, 2, device="cpu", **kw)
    with pytest.raises(ValueError):
        data.stage_round(data.RoundFiles((F.SMALL_H, F.SMALL_W), 1, 1, [(0, 0, clips[0].frames[1])], []), decode="pillow")
    with pytest.raises(ValueError, match="1 files for 2 regions"):
        E.Validation(None, [E.Clip(clips[0].frames[:1], clips[0].regions)], 2, 2, device="cpu")
    arrays = E.Clip(np.zeros((2, F.SMALL_H, F.SMALL_W, 3), np.uint8), clips[0].regions)
    for decode in data.DECODE_MODES:                                # a frame size holds only file clips or none
        with pytest.raises(ValueError, match="file clips"):
            E.Validation(None, [clips[0], arrays], 2, 2, device="cpu", decode=decode)
        E.Validation(None, [arrays, arrays], 2, 2, device="cpu", decode=decode)


# ----------------------------------------------------------------------------------------- round staging against ClipSchedule
@pytest.fixture(scope="module")
def file_clips(tmp_path_factory):
    return F.write_clips(tmp_path_factory.mktemp("clips"), F.LENGTHS, F.H, F.W, F.KINDS, 3)


@pytest.mark.parametrize("decode", ["device", "host"])
def test_every_round_stages_its_own_files_and_no_other(file_clips, decode):
    from ntmtrack import data, evaluate as E
    clips, contents = file_clips
    B, T, frame = 2, 2, F.H * F.W * 3
    v = E.Validation(None, [E.Clip(c.frames, c.regions, None, None) for c in clips], B, T, device="cpu", decode=decode)
    assert [c.size for c in v.classes] == [(F.H, F.W)]              # read from the first file's header
    cls = v.classes[0]
    seen, rounds = set(), 0
    for rnd in E.ClipSchedule(F.LENGTHS, B, T):
        spec = cls.source.round_files(rnd)
        staged = data.stage_round(spec, data.Staging(pin=False), decode=decode)
        rounds += 1
        want = [clips[int(rnd.clip_of[b])].frames[int(rnd.frame_index[t, b])] for t, b in zip(*np.nonzero(rnd.active))]
        want += [clips[c].frames[0] for _s, c in rnd.resets]
        assert staged.names == want and staged.packed.n == len(rnd.resets) + int(rnd.active.sum())
        assert not seen & set(want)                                 # no file is read in two rounds
        seen |= set(want)
        # the table: full frames, cell (t, b) at (t B + b) H W 3, the starting frames behind the block
        table = staged.packed.table.numpy()
        assert (table[:, 1:] == [F.H, F.W, 0, 0, F.H, F.W]).all()
        assert (staged.cell_index >= 0).tolist() == rnd.active.astype(bool).tolist()
        for t, b in zip(*np.nonzero(rnd.active)):
            assert table[staged.cell_index[t, b], 0] == (t * B + b) * frame
        assert staged.start_index.tolist() == [int(rnd.active.sum()) + [s for s, _c in rnd.resets].index(b)
                                               if b in [s for s, _c in rnd.resets] else -1 for b in range(B)]
        for k, (s, _c) in enumerate(rnd.resets):
            assert table[staged.start_index[s], 0] == (T * B + k) * frame
        assert staged.packed.nbytes == (T * B + len(rnd.resets)) * frame
        assert staged.packed.jpeg.on_device == [decode == "device"] * staged.packed.n
        if decode == "host":                                        # Pillow's pixels, zero frames where the round has no file
            frames, firsts = staged.host_frames()
            for t in range(T):
                for b in range(B):
                    c, k = int(rnd.clip_of[b]), int(rnd.frame_index[t, b])
                    assert (frames[t, b] == (J.pillow_decode(contents[c][k]) if rnd.active[t, b] else 0)).all()
            for k, (_s, c) in enumerate(rnd.resets):
                assert (firsts[k] == J.pillow_decode(contents[c][0])).all()
    assert rounds == 5 and len(seen) == sum(F.LENGTHS)            # clips 0, 1 | 2, 3 | 2, 3 | 2, 4 | 4


def test_files_the_device_does_not_take_and_files_of_another_size(file_clips, tmp_path):
    from PIL import Image
    from ntmtrack import data
    clips, contents = file_clips
    img = J.image(F.H, F.W, "smooth", 9)
    png, prog = str(tmp_path / "a.png"), str(tmp_path / "p.jpg")
    Image.fromarray(img).save(png)
    Image.fromarray(img).save(prog, "JPEG", quality=90, progressive=True)
    spec = data.RoundFiles((F.H, F.W), 2, 2, [(0, 0, png), (0, 1, clips[0].frames[1]), (1, 1, contents[1][1])], [(1, prog)])
    staged = data.stage_round(spec, data.Staging(pin=False))
    assert staged.packed.jpeg.on_device == [False, True, True, False]
    assert staged.cell_index.tolist() == [[0, 1], [-1, 2]] and staged.start_index.tolist() == [-1, 3]
    assert staged.names[:2] == [png, clips[0].frames[1]] and staged.names[3] == prog and "bytes" in staged.names[2]
    frames, firsts = staged.host_frames()
    assert (frames[0, 0] == img).all() and (firsts[0] == J.pillow_decode(open(prog, "rb").read())).all()
    small, _c = F.write_clips(tmp_path, [2], F.SMALL_H, F.SMALL_W, F.SMALL_KINDS, 2)
    for decode in data.DECODE_MODES:
        with pytest.raises(ValueError) as e:
            data.stage_round(data.RoundFiles((F.H, F.W), 1, 2, [(0, 0, clips[0].frames[1]), (0, 1, small[0].frames[1])], []),
                             data.Staging(pin=False), decode=decode)
        assert small[0].frames[1] in str(e.value) and "64x80" in str(e.value) and "90x120" in str(e.value)
    with pytest.raises(ValueError, match=str(data.MAX_FRAMES_PER_LAUNCH)):
        data.stage_round(data.RoundFiles((F.H, F.W), 1, 1, [], [(0, png)] * (data.MAX_FRAMES_PER_LAUNCH + 1)))
    with pytest.raises(ValueError, match="not_an_image"):
        bad = str(tmp_path / "not_an_image.jpg")
        open(bad, "wb").write(b"nothing of the kind")
        data.stage_round(data.RoundFiles((F.H, F.W), 1, 1, [(0, 0, bad)], []), data.Staging(pin=False))


def test_pack_jpeg_frames_without_offsets_writes_todays_table(file_clips):
    from ntmtrack import data
    _clips, contents = file_clips
    files = [contents[0][0], contents[3][1], contents[4][2]]
    probed = [data._probe_frame(f, "file %d" % i) for i, f in enumerate(files)]
    rects = [(0, 0, F.H, F.W), (3, 5, 40, 33), (10, 0, 17, F.W)]
    packed = data.pack_jpeg_frames(probed, rects, staging=data.Staging(pin=False))
    sizes = [h * w * 3 for _y, _x, h, w in rects]
    want = [[sum(sizes[:i]), F.H, F.W] + list(r) for i, r in enumerate(rects)]
    assert packed.table.numpy().tolist() == want and packed.nbytes == sum(sizes)
    same = data.pack_jpeg_frames(probed, rects, staging=data.Staging(pin=False), offsets=None)
    assert same.table.numpy().tolist() == want
    moved = data.pack_jpeg_frames(probed, rects, staging=data.Staging(pin=False), offsets=([64, 20000, 40000], 50000))
    assert moved.table.numpy()[:, 0].tolist() == [64, 20000, 40000] and moved.nbytes == 50000
    assert (moved.table.numpy()[:, 1:] == packed.table.numpy()[:, 1:]).all()
    with pytest.raises(ValueError):                                 # a rectangle that leaves the buffer
        data.pack_jpeg_frames(probed, rects, staging=data.Staging(pin=False), offsets=([0, 20000, 49000], 50000))


def test_the_two_packers_place_alike_and_a_packed_batch_moves_whole(file_clips):
    """pack_frames and pack_jpeg_frames share one layout-and-fit step: on the same rectangles of the same files (Pillow's
    pixels) they write the same table rows and pixel bytes, both pack a batch that does not fit with grow=False into an
    unpinned set of its own, and Staging.adopt copies what a batch uses of every buffer a set has."""
    import torch
    from ntmtrack import data
    _clips, contents = file_clips
    files = [contents[0][0], contents[3][1], contents[4][2]]
    rects = [(0, 0, F.H, F.W), (3, 5, 40, 33), (10, 0, 17, F.W)]
    cut = [np.ascontiguousarray(J.pillow_decode(f)[y:y + h, x:x + w]) for f, (y, x, h, w) in zip(files, rects)]
    boxes = [(0.1, 0.2, 0.8, 0.9), (0.0, 0.0, 1.0, 1.0), (0.3, 0.1, 0.6, 0.7)]
    as_probed = [{"data": None, "image": img, "size": img.shape[:2], "what": "image %d" % i} for i, img in enumerate(cut)]
    whole = [(0, 0) + img.shape[:2] for img in cut]
    given = [data.Staging(pin=False), data.Staging(pin=False)]
    a = data.pack_frames(cut, boxes, pack="full", staging=given[0], grow=False)
    b = data.pack_jpeg_frames(as_probed, whole, boxes, staging=given[1], grow=False)
    assert a.nbytes == b.nbytes == sum(img.size for img in cut) and a.n == b.n == 3
    want = [[sum(i.size for i in cut[:k]), h, w, 0, 0, h, w] for k, (_y, _x, h, w) in enumerate(rects)]
    assert a.table.numpy().tolist() == want and b.table.numpy().tolist() == want
    assert a.pixels.numpy().tobytes() == b.pixels.numpy().tobytes() == b"".join(img.tobytes() for img in cut)
    assert a.boxes.numpy().tobytes() == b.boxes.numpy().tobytes() == np.asarray(boxes, np.float32).tobytes()
    for packed, st in zip((a, b), given):                           # did not fit, must not grow: a fresh unpinned set
        assert packed.staging is not st and packed.staging.pin is False and st.pixels.numel() == 0 and st.table.shape[0] == 0
    again = data.pack_frames(cut, boxes, pack="full", staging=given[0])
    assert again.staging is given[0] and data.pack_jpeg_frames(as_probed, whole, boxes, staging=given[1]).staging is given[1]
    assert again.table.numpy().tolist() == a.table.numpy().tolist()
    # the same rectangles of the whole files, every file decoded by the host: the same offsets and pixel bytes
    host = [data._probe_frame(f, "file %d" % i, decode="host") for i, f in enumerate(files)]
    c = data.pack_jpeg_frames(host, rects, staging=data.Staging(pin=False))
    assert c.jpeg.on_device == [False] * 3 and c.table.numpy()[:, 0].tolist() == a.table.numpy()[:, 0].tolist()
    assert c.pixels.numpy().tobytes() == a.pixels.numpy().tobytes()
    # adopt: frames for the device decoder, so that the streams, descriptors and segments are in use
    probed = [data._probe_frame(f, "file %d" % i) for i, f in enumerate(files)]
    old = data.pack_jpeg_frames(probed, rects, boxes, staging=data.Staging(pin=False))
    assert old.jpeg.on_device == [True] * 3
    old.staging.pixels.numpy()[:old.nbytes] = np.arange(old.nbytes) % 251   # the device frames' pixels are not written on the host
    old.staging.labels.numpy()[:3] = np.arange(3 * 66, dtype=np.float32).reshape(3, 66)
    new = data.Staging(pin=False)
    moved = new.adopt(old)
    j = old.jpeg
    used = {"pixels": old.nbytes, "table": 3, "boxes": 3, "labels": 3, "streams": j.stream_bytes, "descs": 3, "segments": j.n_segments}
    assert set(used) == {name for name, t in vars(new).items() if torch.is_tensor(t)}       # every buffer a set has
    for name, k in used.items():
        assert k > 0 and torch.equal(getattr(new, name)[:k], getattr(old.staging, name)[:k]), name
    assert moved.staging is new and moved.jpeg is j and (moved.nbytes, moved.n, moved.channels) == (old.nbytes, 3, 3)
    assert (moved.resize_to, moved.crop) == (old.resize_to, old.crop) and torch.equal(moved.table, old.table)


# ------------------------------------------------------------------------------------------------- ntk_track_decode_mask
@pytest.fixture(scope="module")
def L():
    from ntmtrack import _lib
    return _lib.lib()


def mask(L, status=ONE, n_status=5, cell_index=ONE, start_index=ONE, clip_of=ONE, T=2, B=3, n_clips=4, dead=ONE, active=ONE, table=ONE):
    return L.ntk_track_decode_mask(status, n_status, cell_index, start_index, clip_of, T, B, n_clips, dead, active, table, None)


def test_decode_mask_is_exported_and_bound(L):
    from ntmtrack import _lib
    assert hasattr(L, "ntk_track_decode_mask") and "ntk_track_decode_mask" in _lib.exported_symbols()
    assert len(L.ntk_track_decode_mask.argtypes) == 12


@pytest.mark.parametrize("arg", ["status", "cell_index", "start_index", "clip_of", "dead", "active", "table"])
def test_decode_mask_refuses_null_pointers(L, arg):
    assert mask(L, **{arg: None}) == -2


@pytest.mark.parametrize("kw,named", [({"T": 0}, b"T=0"), ({"T": -3}, b"T=-3"), ({"B": 0}, b"B=0"), ({"B": -1}, b"B=-1"),
                                      ({"B": 65536}, b"B=65536"), ({"n_clips": 0}, b"n_clips=0"), ({"n_clips": -2}, b"n_clips=-2"),
                                      ({"n_status": 0}, b"n_status=0"), ({"n_status": -9}, b"n_status=-9")])
def test_decode_mask_refuses_bad_sizes_and_names_the_value(L, kw, named):
    assert mask(L, **kw) == -1
    assert named in L.ntk_last_error()


def test_the_clipdec_layout_of_the_header_is_the_one_python_uses():
    from ntmtrack import evaluate as E
    import decode_mask_util as M
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "ntmtrack.h")).read()
    d = {k: int(v) for k, v in re.findall(r"#define (NTK_CLIPDEC_[A-Z_]+)\s+(\d+)", hdr)}
    names = ("DECODED", "FAILED", "MASKED", "FIRST_FAILED", "FIRST_STATUS", "START_STATUS", "HEAD")
    assert d == {"NTK_CLIPDEC_" + k: getattr(E, "CLIPDEC_" + k) for k in names}
    assert [d["NTK_CLIPDEC_" + k] for k in names] == [0, 1, 2, 3, 4, 5, 6] == [getattr(M, k) for k in names]
    assert M.BAD_DESC == int(re.search(r"#define NTK_JPEG_STATUS_BAD_DESC\s+(\d+)", hdr).group(1))
