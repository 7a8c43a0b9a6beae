"""GPU: the one-launch training input -- ntk_frames_crop_batch (resize, mean, crop and flip of n packed uint8 frames of different
sizes) and data.get_input_batch on top of it -- against the per-frame chain it replaces (ntk_resize_bilinear on the fp32 image,
then ntk_crop_and_resize), bit for bit, and against the float64 chain (small_kernel_util.resize_ref, then
oracle.online_oracle.crop_and_resize) within the 5e-3 that test_data_gpu.py holds get_input to.

Shapes: resize_to 36 x 64, crop 24 x 24 (576 output pixels: three workgroups per frame, the last one partly idle), C = 3, unless a
case says otherwise.  Every output lies in a NaN-guarded buffer; the guards are checked in every case (FlatGuarded.written).

The float64 comparison and the border: the oracle decides "inside the image" on its own float64 sample position, and for the whole
frame box [0,0,1,1] at 64 -> 24 columns that position is 23 * (63 / 23) = 63.00000000000001 > 63 -- outside by one float64
rounding, where the exact position (63) and the kernels' fp32 one (63.0) are inside.  So the oracle is evaluated twice, at the box
and at the box drawn in by 1e-12 towards its centre (which moves no value by more than 1e-8), and every element must be within
the bound of one of the two; where the two agree -- everywhere but such a border sample -- that is the plain comparison.
"""
import numpy as np
import pytest
import torch

from oracle import online_oracle as OO
from small_kernel_util import FlatGuarded, raw_bytes_equal, resize_ref, vptr

pytestmark = pytest.mark.gpu

RESIZE, CROP = (36, 64), (24, 24)
MEAN = np.array([123.68, 116.78, 103.94, 110.0], np.float32)
ATOL = 5e-3
SIZES = [(60, 80), (45, 37), (36, 64), (9, 200), (200, 9), (2, 2), (1, 1)]
BOXES = [("interior", [0.2, 0.25, 0.7, 0.8]), ("whole", [0.0, 0.0, 1.0, 1.0]), ("partly_outside", [-0.23, -0.1, 0.6, 1.3]),
         ("wholly_outside", [1.2, 1.3, 1.8, 1.9]), ("y1_eq_y2", [0.4, 0.1, 0.4, 0.9]), ("inverted", [0.8, 0.9, 0.1, 0.2])]
VARIANTS = [(True, 0.0), (True, -3.5), (False, 0.0), (False, -3.5)]        # (mean present, extrapolation)


def _image(H, W, C, seed):
    return np.random.default_rng(seed).integers(0, 256, size=(H, W, C), dtype=np.uint8)


class Dev(object):
    def __init__(self, cuda):
        from ntmtrack import _lib, data
        self.cuda, self.L, self.lib, self.data = cuda, _lib.lib(), _lib, data
        self.means = {C: torch.from_numpy(MEAN[:C].copy()).to(cuda) for C in (1, 3, 4)}

    def chain(self, img, box, mean, ext, resize=RESIZE, crop=CROP):
        """The per-frame chain of get_input: ntk_resize_bilinear of the fp32 image, then ntk_crop_and_resize."""
        H, W, C = img.shape
        src = torch.from_numpy(img.astype(np.float32)).to(self.cuda)
        big = torch.empty((resize[0], resize[1], C), device=self.cuda)
        st = self.lib.stream()
        self.lib.check(self.L.ntk_resize_bilinear(vptr(src), H, W, C, vptr(big), resize[0], resize[1], st), "ntk_resize_bilinear")
        out = FlatGuarded((crop[0], crop[1], C), self.cuda)
        b = [float(np.float32(v)) for v in box]
        self.lib.check(self.L.ntk_crop_and_resize(vptr(big), resize[0], resize[1], C, vptr(self.means[C]) if mean else None,
                                                  b[0], b[1], b[2], b[3], out.ptr, crop[0], crop[1], ext, st), "ntk_crop_and_resize")
        torch.cuda.synchronize()
        return out.written()

    def fused(self, images, boxes, mean, ext, resize=RESIZE, crop=CROP, pack="full", pad=0, flip=False, edit=None):
        """One ntk_frames_crop_batch launch over the packed batch; `edit(table)` may rewrite the frame table after packing."""
        packed = self.data.pack_frames(images, boxes, resize_to=resize, crop=crop, margin=2, pack=pack, pad=pad)
        if edit is not None:
            edit(packed.table.numpy(), packed.nbytes)
        C = images[0].shape[2]
        out = FlatGuarded((len(images), crop[0], crop[1], C), self.cuda)
        got = self.data.frames_crop_batch(packed, self.cuda, mean=self.means[C] if mean else None, flip_x=flip, extrapolation=ext,
                                          out=out.view)
        assert got.data_ptr() == out.view.data_ptr()
        torch.cuda.synchronize()
        return out.written(), packed


@pytest.fixture(scope="module")
def dev(cuda):
    return Dev(cuda)


@pytest.fixture(scope="module")
def batch():
    """The 7 frames x 6 boxes of the issue as one batch of 42 rows (frame-major)."""
    frames = [_image(H, W, 3, seed=10 + i) for i, (H, W) in enumerate(SIZES)]
    images = [f for f in frames for _b in BOXES]
    boxes = [b for _f in frames for _n, b in BOXES]
    return images, boxes


@pytest.fixture(scope="module")
def chain_ref(dev, batch):
    """The parent's per-frame chain on the batch, computed once per (mean, extrapolation)."""
    images, boxes = batch
    return {v: np.stack([dev.chain(img, box, v[0], v[1]) for img, box in zip(images, boxes)]) for v in VARIANTS}


def _row_names(batch):
    return ["%dx%d/%s" % (SIZES[i // len(BOXES)] + (BOXES[i % len(BOXES)][0],)) for i in range(len(batch[0]))]


@pytest.mark.parametrize("mean,ext", VARIANTS)
def test_same_bits_as_the_per_frame_chain(dev, batch, chain_ref, mean, ext):
    images, boxes = batch
    got, _ = dev.fused(images, boxes, mean, ext)
    ref = chain_ref[(mean, ext)]
    for i, name in enumerate(_row_names(batch)):
        diff = float(np.max(np.abs(got[i].astype(np.float64) - ref[i])))
        assert raw_bytes_equal(got[i], ref[i]), "%s: fused launch and chain differ, max |difference| %.3g" % (name, diff)


def _drawn_in(box, eps=1e-12):
    b = [float(np.float32(v)) for v in box]
    cy, cx = 0.5 * (b[0] + b[2]), 0.5 * (b[1] + b[3])
    return [b[0] + np.sign(cy - b[0]) * eps, b[1] + np.sign(cx - b[1]) * eps, b[2] + np.sign(cy - b[2]) * eps,
            b[3] + np.sign(cx - b[3]) * eps]


def float64_chain(img, box, mean, ext, resize=RESIZE, crop=CROP):
    """(oracle at the box, oracle at the box drawn in by 1e-12): see the module docstring."""
    C = img.shape[2]
    big = resize_ref(img, resize[0], resize[1]) - (MEAN[:C].astype(np.float64) if mean else 0.0)
    b = [float(np.float32(v)) for v in box]
    return OO.crop_and_resize(big, b, crop[0], crop[1], ext), OO.crop_and_resize(big, _drawn_in(box), crop[0], crop[1], ext)


@pytest.mark.parametrize("mean,ext", VARIANTS)
def test_against_the_float64_chain(dev, batch, mean, ext):
    images, boxes = batch
    got, _ = dev.fused(images, boxes, mean, ext)
    for i, name in enumerate(_row_names(batch)):
        a, b = float64_chain(images[i], boxes[i], mean, ext)
        err = np.minimum(np.abs(got[i] - a), np.abs(got[i] - b))
        print("%s mean=%s ext=%g: max |kernel - float64 chain| = %.3g" % (name, mean, ext, err.max()))
        assert err.max() <= ATOL, "%s: max |kernel - float64 chain| = %.3g > %.3g" % (name, err.max(), ATOL)


BORDER_BOXES = [[0.0, 0.3, 0.4, 0.7], [0.6, 0.3, 1.0, 0.7], [0.3, 0.0, 0.7, 0.4], [0.3, 0.6, 0.7, 1.0], [0.2, 0.25, 0.7, 0.8],
                [-0.23, -0.1, 0.6, 1.3], [1.2, 1.3, 1.8, 1.9]]


@pytest.mark.parametrize("pad", [1, 0])
def test_rect_packing_gives_the_bits_of_full_packing(dev, pad):
    """Boxes touching each of the four borders (and inside, partly and wholly outside) on sources larger and smaller than the
    resized image; with pad = 1 the first frame starts at byte 1, and between the two pads every frame starts once at an odd byte."""
    frames = [_image(H, W, 3, seed=40 + i) for i, (H, W) in enumerate([(60, 80), (45, 37), (200, 9), (9, 200), (130, 150)])]
    images = [f for f in frames for _b in BORDER_BOXES]
    boxes = [b for _f in frames for b in BORDER_BOXES]
    full, pf = dev.fused(images, boxes, True, -3.5, pack="full", pad=pad)
    rect, pr = dev.fused(images, boxes, True, -3.5, pack="rect", pad=pad)
    assert int(pr.table[0, 0]) == pad and int(pf.table[0, 0]) == pad
    if pad:
        assert (pr.table[:, 0].numpy() % 2 == 1).any() and (pr.table[:, 0].numpy() % 4 != 0).any()
    assert pr.nbytes < pf.nbytes, "rect packing took %d bytes, full packing %d" % (pr.nbytes, pf.nbytes)
    assert (pr.table[:, 5:7].numpy() >= 1).all()
    assert raw_bytes_equal(rect, full)


def test_flip_x_is_the_flipped_crop(dev, batch):
    images, boxes = batch
    plain, _ = dev.fused(images, boxes, True, -3.5)
    flipped, _ = dev.fused(images, boxes, True, -3.5, flip=True)
    assert raw_bytes_equal(flipped, torch.flip(torch.from_numpy(plain), dims=[2]).numpy())
    assert not raw_bytes_equal(flipped, plain)


def test_bad_rows_are_not_dereferenced(dev):
    """Rows whose rectangle leaves the buffer, is empty, lies at a negative offset or leaves its image, and a row of an absurd
    frame size: the extrapolation value everywhere, the other rows unchanged."""
    frames = [_image(H, W, 3, seed=60 + i) for i, (H, W) in enumerate([(60, 80), (45, 37), (36, 64), (9, 200), (50, 50), (20, 30), (24, 28)])]
    boxes = [[0.2, 0.25, 0.7, 0.8]] * len(frames)
    good, _ = dev.fused(frames, boxes, True, -3.5)

    def edit(table, nbytes):
        table[1, 0] = nbytes - 5            # 45 * 37 * 3 bytes from 5 before the end: leaves pixels_bytes
        table[2, 5] = 0                     # h = 0
        table[3, 0] = -1                    # starts before the buffer
        table[4, 6] = 51                    # w = 51 in a 50-wide image
        table[6, 1] = 1 << 31               # a frame of 2^31 rows: above the 2^30 the index arithmetic is held to
    bad, _ = dev.fused(frames, boxes, True, -3.5, edit=edit)
    for i in (1, 2, 3, 4, 6):
        assert (bad[i] == np.float32(-3.5)).all(), "row %d was read" % i
    for i in (0, 5):
        assert raw_bytes_equal(bad[i], good[i])

    def edit_h(table, nbytes):
        table[0, 5] = 0
    bad, _ = dev.fused(frames, boxes, False, 0.0, edit=edit_h)
    assert (bad[0] == 0).all() and bad[0].tobytes() == np.zeros_like(bad[0]).tobytes()
    plain, _ = dev.fused(frames, boxes, False, 0.0)
    assert raw_bytes_equal(bad[1:], plain[1:])


@pytest.mark.parametrize("crop,C", [((1, 1), 3), ((1, 24), 3), ((24, 1), 3), ((24, 24), 1), ((24, 24), 4), ((5, 300), 3)])
def test_crop_shapes_and_channel_counts(dev, crop, C):
    """crop_h == 1 / crop_w == 1 take the centre-sample branches; C = 1 and C = 4; 5 x 300: a crop wider than it is tall, 1 500
    pixels in six workgroups."""
    frames = [_image(H, W, C, seed=80 + i) for i, (H, W) in enumerate([(60, 80), (45, 37), (2, 2)])]
    rows = [(f, b) for f in frames for _n, b in BOXES]
    images, boxes = [f for f, _b in rows], [b for _f, b in rows]
    got, _ = dev.fused(images, boxes, True, -3.5, crop=crop, pack="rect", pad=1)
    for i, (img, box) in enumerate(rows):
        assert raw_bytes_equal(got[i], dev.chain(img, box, True, -3.5, crop=crop)), (i, box)


@pytest.mark.parametrize("reverse", [False, True])
def test_get_input_batch_equals_get_input(cuda, tmp_path, reverse):
    from PIL import Image
    from ntmtrack import data
    rng = np.random.default_rng(5)
    d = tmp_path / "train_seq_0"
    d.mkdir()
    names = []
    boxes = ["0.1,0.15,0.9,0.8", "0.0,0.0,1.0,1.0", "-0.2,0.3,0.6,1.2", "0.45,0.4,0.75,0.7"]
    for i in range(4):
        arr = rng.integers(0, 256, size=(60, 80, 3) if i % 2 == 0 else (45, 37, 3), dtype=np.uint8)
        png = str(d / ("img%d.png" % i))
        Image.fromarray(arr).save(png)
        stem = str(d / ("%06d" % i))
        rng.random((8, 8)).tofile(stem + ".bin")
        with open(stem + ".txt", "w") as f:
            f.write("%s,0.3,0.3,0.6,0.6,%s,%g,%g" % (boxes[i], png, 0.05 * i, -0.1 * i))
        names.append(stem)
    ref = data.get_input(names, device=cuda, reverse_image=reverse)
    for pack in ("rect", "full"):
        got = data.get_input_batch(names, device=cuda, reverse_image=reverse, workers=2, pack=pack)
        torch.cuda.synchronize()
        for g, r, what in zip(got, ref, ("batch_img", "batch_gt", "y_offsets", "x_offsets")):
            assert g.shape == r.shape and g.dtype == r.dtype, what
            assert raw_bytes_equal(g.cpu().numpy(), r.cpu().numpy()), "%s differs (pack=%s)" % (what, pack)
    assert got[0].shape == (4, 224, 224, 3) and got[1].shape == (4, 8, 8)
