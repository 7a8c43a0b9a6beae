"""GPU: the device JPEG decoder (ntk_jpeg_decode_batch through data.decode_jpeg_batch) gives Pillow's bytes -- tolerance zero --
over a grid of Pillow-written files decoded as a few mixed batches; rectangles equal slices of the full decode and touch nothing
outside themselves; a batch of three gives frame 0 the bits of a batch of one; a truncated file among good ones is flagged in
`status` and leaves the others alone (its bounds were proven on the CPU first: tests/test_jpeg_host.py decodes the same file)."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as J  # noqa: E402

pytestmark = pytest.mark.gpu

@pytest.fixture(scope="module")
def grid():
    return J.grid()


def test_the_grid_is_pillows_bytes_and_all_of_it_is_decoded_on_the_device(cuda, grid):
    from ntmtrack import data
    assert len(grid) == 280
    # the restatement of the arithmetic decodes every file of the grid to Pillow's bytes: the count below is met by the reference
    want = [J.pillow_decode(f) for _n, f in grid]
    assert all(np.array_equal(J.decode(f), w) for (_n, f), w in zip(grid, want))
    order = np.random.default_rng(0).permutation(len(grid))                 # mixed batches: sizes, samplings and restarts together
    on_device, bad = 0, []
    for chunk in np.array_split(order, 4):
        res = data.decode_jpeg_batch([grid[i][1] for i in chunk], device=cuda)
        torch.cuda.synchronize()
        status = res.status.cpu().numpy()
        on_device += sum(res.on_device)
        pixels = res.pixels.cpu().numpy()
        for k, i in enumerate(chunk):
            off, H, W = [int(v) for v in res.table[k, :3]]
            got = pixels[off:off + H * W * 3].reshape(H, W, 3)
            if status[k] != 0 or not np.array_equal(got, want[i]):
                bad.append((grid[i][0], int(status[k]), int(np.count_nonzero(got != want[i]))))
    assert not bad, "%d files differ from Pillow (name, status, bytes that differ): %s" % (len(bad), bad[:10])
    assert on_device == len(grid), "only %d of %d files were decoded on the device" % (on_device, len(grid))


_decode_guarded = J.decode_guarded


RECT_FILES = {
    "4:2:0": dict(subsampling=2),
    "4:2:2 with a restart interval": dict(subsampling=1, restart_marker_blocks=3),
}


@pytest.mark.parametrize("kind", sorted(RECT_FILES))
def test_rectangles_equal_slices_of_the_full_decode_and_touch_nothing_else(cuda, kind):
    H, W = 120, 200
    f = J.encode(J.image(H, W, "noise", 2), quality=90, **RECT_FILES[kind])
    full = J.pillow_decode(f)
    rects = [None, (0, 0, 1, 1), (H - 1, W - 1, 1, 1), (0, W - 1, H, 1), (H - 1, 0, 1, W)]
    for y0 in (0, 15, 16, 17):
        for x0 in (0, 15, 16, 17):
            rects.append((y0, x0, 33 + y0 % 3, 30 + x0 % 2))
            rects.append((y0, x0, H - y0, W - x0))                          # through the last row and column
    rects += [(57, 93, 1, 1), (40, 0, 16, W), (0, 96, H, 16)]
    images, status, guard_ok = _decode_guarded(cuda, [f] * len(rects), rects)
    assert not status.any(), status
    assert guard_ok, "bytes outside the rectangles were written"
    for img, r in zip(images, rects):
        y0, x0, h, w = (0, 0, H, W) if r is None else r
        assert np.array_equal(img, full[y0:y0 + h, x0:x0 + w]), "rectangle %s of the %s file differs from the slice" % (r, kind)


def test_frame_0_of_a_batch_of_three_is_a_batch_of_one(cuda, grid):
    files = [grid[100][1], grid[7][1], grid[250][1]]
    three, s3, g3 = _decode_guarded(cuda, files, [None] * 3)
    one, s1, g1 = _decode_guarded(cuda, files[:1], [None])
    assert not s3.any() and not s1.any() and g3 and g1
    assert three[0].tobytes() == one[0].tobytes()


def test_a_truncated_scan_is_flagged_and_the_other_frames_are_untouched(cuda, grid):
    """Runs once.  The file is the one tests/test_jpeg_host.py sends through the same segment decoder on the CPU under the
    sanitizers (NTK_JPEG_STATUS_TRUNCATED there too)."""
    from ntmtrack import data
    good = [grid[33][1], grid[200][1], grid[279][1]]
    files = [good[0], good[1], J.truncated_file(), good[2]]
    images, status, guard_ok = _decode_guarded(cuda, files, [None] * 4)
    assert guard_ok
    assert status[2] == 2 and data.JPEG_STATUS[2].startswith("the scan ends"), status
    assert list(status[[0, 1, 3]]) == [0, 0, 0]
    for img, f in zip([images[0], images[1], images[3]], good):
        assert np.array_equal(img, J.pillow_decode(f))


def test_files_the_device_does_not_take_are_decoded_by_the_host_in_the_same_batch(cuda, grid):
    from ntmtrack import data
    prog = J.encode(J.image(40, 56, "smooth"), quality=90, progressive=True)
    res = data.decode_jpeg_batch([grid[5][1], prog, grid[150][1]], rects=[None, (3, 4, 20, 31), None], device=cuda)
    torch.cuda.synchronize()
    assert res.on_device == [True, False, True] and not res.status.cpu().numpy().any()
    assert np.array_equal(res.image(0), J.pillow_decode(grid[5][1]))
    assert np.array_equal(res.image(1), J.pillow_decode(prog)[3:23, 4:35])
    assert np.array_equal(res.image(2), J.pillow_decode(grid[150][1]))
