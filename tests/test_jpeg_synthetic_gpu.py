"""GPU: the device JPEG decoder on what Pillow's encoder never writes and on the parts of its kernels no Pillow-grid test reaches.
Every assertion is byte equality with Pillow's decode, status 0 and a decode on the device.

  * the synthetic corpus of tests/jpeg_write.py (table indices 2 and 3, chain / single-code / length-limited Huffman tables, DC
    differences of category 11, ZRL rows, blocks without an EOB, fill bytes, repeated DRI / DHT / DQT, 250 restart segments in one
    frame) in shuffled batches mixed with files of the Pillow grid.  tests/test_jpeg_host.py proves on the CPU that the restatement
    equals Pillow on every corpus file and that the segment decoder stays in bounds on them, under the sanitizers;
  * rectangles of 4:4:4 and gray files (the window's branch without a halo) and of 4:2:0 / 4:2:2 files at an odd size, where the
    chroma clamp of the window meets the far edge;
  * frames whose window has more than 4096 blocks, so that the inverse DCT kernel's block loop wraps (and the colour kernel's
    pixel loop, and with restart interval 8 the entropy kernel's lane loop);
  * a workspace used a second time: only non-zero coefficients are stored, so the entry's clearing is what a sparse frame after
    a dense one rests on;
  * a frame with 250 segments at three places of a batch: the segment table's offsets do not leak between frames."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as J  # noqa: E402
import jpeg_write as JW  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def corpus():
    return JW.corpus()


def test_the_corpus_is_pillows_bytes_in_batches_mixed_with_the_grid(cuda, corpus):
    from ntmtrack import data
    files = corpus + J.grid()[::7]                                          # 36 synthetic + 40 Pillow-written
    want = [J.pillow_decode(f) for _n, f in files]
    order = np.random.default_rng(1).permutation(len(files))
    on_device, bad = 0, []
    for chunk in np.array_split(order, 3):
        res = data.decode_jpeg_batch([files[i][1] for i in chunk], device=cuda)
        torch.cuda.synchronize()
        status = res.status.cpu().numpy()
        on_device += sum(res.on_device)
        pixels = res.pixels.cpu().numpy()
        for k, i in enumerate(chunk):
            off, H, W = [int(v) for v in res.table[k, :3]]
            got = pixels[off:off + H * W * 3].reshape(H, W, 3)
            if status[k] != 0 or got.shape != want[i].shape or not np.array_equal(got, want[i]):
                bad.append((files[i][0], int(status[k]), int(np.count_nonzero(got != want[i])) if got.shape == want[i].shape else -1))
    assert not bad, "%d files differ from Pillow (name, status, bytes that differ): %s" % (len(bad), bad[:10])
    assert on_device == len(files), "only %d of %d files were decoded on the device" % (on_device, len(files))


H_ODD, W_ODD = 121, 199
RECT_FILES = {
    "4:4:4": dict(subsampling=0),
    "4:4:4 with a restart interval": dict(subsampling=0, restart_marker_blocks=7),      # 25 MCUs a row
    "gray": dict(gray=True),
    "gray with a restart interval": dict(gray=True, restart_marker_blocks=7),
    "4:2:0": dict(subsampling=2),
    "4:2:2": dict(subsampling=1),
}


def _rectangles(H, W):
    rects = [None, (0, 0, 1, 1), (H - 1, W - 1, 1, 1), (H - 2, W - 2, 1, 1), (0, W - 1, H, 1), (H - 1, 0, 1, W)]
    for y0 in (0, 15, 16, 17):
        for x0 in (0, 15, 16, 17):
            rects.append((y0, x0, 33 + y0 % 3, 30 + x0 % 2))
            rects.append((y0, x0, H - y0, W - x0))                          # through the last row and column
    return rects + [(57, 93, 1, 1), (40, 0, 16, W), (0, 96, H, 16)]


@pytest.mark.parametrize("kind", sorted(RECT_FILES))
def test_rectangles_of_odd_sized_files_equal_slices_and_touch_nothing_else(cuda, kind):
    H, W = H_ODD, W_ODD
    kw = dict(RECT_FILES[kind])
    img = J.image(H, W, "noise", 4)
    f = J.encode(img[:, :, 1].copy() if kw.pop("gray", False) else img, quality=90, **kw)
    full = J.pillow_decode(f)
    rects = _rectangles(H, W)
    images, status, guard_ok = J.decode_guarded(cuda, [f] * len(rects), rects)
    assert not status.any(), status
    assert guard_ok, "bytes outside the rectangles were written"
    for img, r in zip(images, rects):
        y0, x0, h, w = (0, 0, H, W) if r is None else r
        assert np.array_equal(img, full[y0:y0 + h, x0:x0 + w]), "rectangle %s of the %s file differs from the slice" % (r, kind)


def _axis(p0, n, size, s, mcus):
    """jpeg_window_axis of csrc/jpeg_entropy.h restated -> number of MCUs"""
    a, b = p0, p0 + n - 1
    if s == 2:
        a, b = max((p0 >> 1) - 1, 0), min(((p0 + n - 1) >> 1) + 1, ((size + 1) >> 1) - 1)
    b = min(b >> 3, mcus - 1)
    return b - min(a >> 3, b) + 1


# sampling -> (side, hs, vs, blocks per MCU): the smallest squares of whole MCUs with more than 4096 blocks, none a multiple of 4096
WRAP_FRAMES = {"gray": (520, 1, 1, 1), "4:4:4": (304, 1, 1, 3), "4:2:2": (360, 2, 1, 4), "4:2:0": (424, 2, 2, 6)}


@pytest.mark.parametrize("restarts", [False, True])
@pytest.mark.parametrize("sampling", sorted(WRAP_FRAMES))
def test_frames_of_more_than_4096_blocks_are_pillows_bytes_whole_and_as_a_rectangle(cuda, sampling, restarts):
    """Written by Pillow, without restart markers and with an interval of 8 MCUs (5 for 4:2:0, whose 729 MCUs make 92 segments at 8):
    more than 128 segments each."""
    side, hs, vs, bpm = WRAP_FRAMES[sampling]
    restart = (5 if sampling == "4:2:0" else 8) if restarts else 0
    img = J.image(side, side, "noise" if restart else "smooth", 5)
    kw = {"restart_marker_blocks": restart} if restart else {}
    if sampling == "gray":
        f = J.encode(img[:, :, 0].copy(), quality=75, **kw)
    else:
        f = J.encode(img, quality=75, subsampling={"4:4:4": 0, "4:2:2": 1, "4:2:0": 2}[sampling], **kw)
    mx, my = -(-side // (8 * hs)), -(-side // (8 * vs))
    rect = (3, 9, side - 5, side - 12)
    for y0, x0, h, w in ((0, 0, side, side), rect):
        blocks = _axis(x0, w, side, hs, mx) * _axis(y0, h, side, vs, my) * bpm
        assert blocks > 4096 and blocks % 4096, "the window of %s has %d blocks" % ((y0, x0, h, w), blocks)
    if restart:
        assert -(-mx * my // restart) > 128
    full = J.pillow_decode(f)
    images, status, guard_ok = J.decode_guarded(cuda, [f, f], [None, rect])
    assert not status.any() and guard_ok, status
    assert np.array_equal(images[0], full), "%d bytes of the whole frame differ" % np.count_nonzero(images[0] != full)
    y0, x0, h, w = rect
    assert np.array_equal(images[1], full[y0:y0 + h, x0:x0 + w]), "the rectangle differs from the slice"


@pytest.mark.parametrize("sampling", ["s420", "s444"])
def test_a_reused_workspace_is_cleared(cuda, sampling):
    """Two calls on the same workspace, status and descriptor buffers: a dense quality-100 noise file, then a DC-only synthetic
    file of the same size and sampling (the same workspace offsets).  The workspace starts out as ones, too."""
    from ntmtrack import _lib, data
    H, W = 48, 64
    dense = J.encode(J.image(H, W, "noise", 6), quality=100, subsampling={"s444": 0, "s420": 2}[sampling])
    rng = np.random.default_rng(7)
    coef = np.zeros(JW.grid_shape(H, W, sampling) + (64,), np.int64)
    coef[..., 0] = rng.integers(-60, 61, size=coef.shape[:-1])
    std = {(0, 0): JW.STD_DC_LUMA, (1, 0): JW.STD_AC_LUMA, (0, 1): JW.STD_DC_CHROMA, (1, 1): JW.STD_AC_CHROMA}
    sparse = JW.write(coef, H, W, sampling, {0: JW.quant_ramp(8, 0)}, (0, 0, 0), std, ((0, 0), (1, 1), (1, 1)))
    assert np.array_equal(J.decode(sparse), J.pillow_decode(sparse))
    packs = [data.pack_jpeg_frames([data._probe_frame(f, "file")], [(0, 0, H, W)], staging=data.Staging()) for f in (dense, sparse)]
    assert all(p.jpeg.on_device == [True] for p in packs) and packs[0].jpeg.workspace_bytes == packs[1].jpeg.workspace_bytes
    ws_bytes = packs[0].jpeg.workspace_bytes
    ws = torch.full((ws_bytes,), 0xFF, dtype=torch.uint8, device=cuda)
    descs = torch.empty((data.JPEG_DESC_BYTES,), dtype=torch.uint8, device=cuda)
    status = torch.full((1,), 77, dtype=torch.int32, device=cuda)
    pix = torch.zeros((H * W * 3,), dtype=torch.uint8, device=cuda)
    P = _lib.ptr
    for packed, f in zip(packs, (dense, sparse)):
        j, st = packed.jpeg, packed.staging
        streams, segs = st.streams[:j.stream_bytes].to(cuda), st.segments[:j.n_segments].to(cuda)
        table = packed.table.to(cuda)
        descs.copy_(st.descs[0])
        _lib.check(_lib.lib().ntk_jpeg_decode_batch(P(streams), j.stream_bytes, P(descs), P(segs), j.n_segments, P(table), P(pix),
                                                    H * W * 3, P(ws), ws_bytes, P(status), 1, _lib.stream()), "ntk_jpeg_decode_batch")
        torch.cuda.synchronize()
        assert int(status.cpu()[0]) == 0
        got, want = pix.cpu().numpy().reshape(H, W, 3), J.pillow_decode(f)
        assert np.array_equal(got, want), "%d bytes differ" % np.count_nonzero(got != want)


def test_a_frame_of_250_segments_is_the_same_at_every_place_of_a_batch(cuda, corpus):
    files = dict(corpus)
    many, other, single = files["gray_manyseg_160x200"], files["s444_manyseg_88x96"], files["s420_dcwalk_64x80"]
    want = J.pillow_decode(many)
    one, s1, g1 = J.decode_guarded(cuda, [many], [None])
    mid, s2, g2 = J.decode_guarded(cuda, [other, many, single], [None] * 3)
    last, s3, g3 = J.decode_guarded(cuda, [single, other, many], [None] * 3)
    assert not s1.any() and not s2.any() and not s3.any() and g1 and g2 and g3
    assert np.array_equal(one[0], want)
    assert one[0].tobytes() == mid[1].tobytes() == last[2].tobytes()
    assert np.array_equal(mid[0], J.pillow_decode(other)) and np.array_equal(last[0], J.pillow_decode(single))
