"""GPU: the image kernels of csrc/image_crop.hip -- crop_resize_kernel (ntk_crop_and_resize), crop_resize_batch_kernel<float> and
<unsigned char> (ntk_crop_and_resize_batch), resize_bilinear_kernel (ntk_resize_bilinear) -- against
oracle/online_oracle.crop_and_resize and small_kernel_util.resize_ref in float64, through the C entries with device pointers.

Every output starts as GUARD_NAN between guard words: afterwards no element is NaN and the guards hold their bits.  Every fp32 image
is followed (and preceded) by at least two image rows of INPUT_NAN: a neighbour fetched from behind the last row or column of the
last row turns the result into a NaN that is not the guard's (a weight of exactly 0 does not hide it: 0 x NaN = NaN).

kernel                       case                                          the loop, branch or limit it sits on
crop_resize_kernel and       crops 5 x 9 and 9 x 5, C 1, 3, 4              `x = (idx / C) % cw, y = idx / (C cw)`: ch != cw shows a swap; C = 4 and 1
both batch kernels                                                         beside the usual 3; 135 / 180 elements < one block of 256
                             crops 1 x 9, 9 x 1, 1 x 1                     the centre-sample branch 0.5 (y1 + y2) (H - 1); 1 x 1, C 1: the minimum
                             images 1 x 53 and 37 x 1                      H - 1 = 0: every sample is row 0, ty = by = 0
                             mean null                                     `mean ? mean[c] : 0`
                             extrapolation -7.5, box partly outside        the value is NOT mean-subtracted
                             y2 < y1, x2 < x1                              negative scales: the unflipped crop reversed
                             33 x 65 -> 17 x 9 and 65 x 33 -> 9 x 17,      scales exactly 2 and 8: the sample (16, 8) is pixel (32, 64), in_y == H - 1 and
                             box [0, 0, 1, 1] and [.5, .5, 1.5, 1.5]       in_x == W - 1 are inside, the next sample is outside; in_y == 0 inside; bit for bit
                             pixels 0 and 255                              u8 -> fp32 is exact: bit-equal to the fp32 entry
                             crop 24 x 40, C 3                             2880 elements: 12 blocks, the last one partly idle
                             B = 1; B = 70, F = 3, seven kinds of box      blockIdx.y = tracker; frame_of holds the first and the last frame
resize_bilinear_kernel       19 x 23 -> 19 x 23                            ratio exactly 1: identity, bit for bit
                             32 x 48 -> 16 x 24                            ratio exactly 2: img[::2, ::2], bit for bit
                             16 x 24 -> 32 x 48, integer pixels            ratio exactly 1/2: quarter-integers, exact in fp32; the last output row and
                                                                           column have y0 = H - 1: `min(y0 + 1, H - 1)`
                             37 x 53 <-> 24 x 40, C 1, 3; 1 x 1 -> 3 x 2   non-square ratios down and up; 2880 / 5883 elements = 12 / 23 blocks

The 2e-3 bound of the interior cases (tests/test_online_gpu.py).  The kernels compute the sample coordinate in fp32, as the TF ops
they restate do.  Bilinear interpolation is continuous in the coordinate, so a coordinate error d costs at most d x (largest
difference between neighbouring pixels) per axis.  Pixels are 0..255, image sides at most 64: a coordinate below 64 has an fp32
spacing of 2^-18 = 3.8e-6; the scale carries three roundings (relative 1.8e-7, times at most 63 steps = 1.1e-5 in the worst case,
a few e-6 typically) and the product and the sum one half-spacing each.  2e-3 / 255 = 7.8e-6 is two spacings of the coordinate:
the typical error with room, not the worst case; the interpolation itself adds four roundings of values below 256 (6e-5).  The
inside / outside decision is NOT continuous: interior cases keep every sample at least 1e-3 pixels away from the image's border
(checked with the float64 coordinates), unless the sample's coordinate is computed without any rounding in fp32 (then it is the
float64 one, with or without FMA contraction); the exact cases consist of such samples only and are compared bit for bit."""
import numpy as np
import pytest
import torch

from oracle import online_oracle as OO
from small_kernel_util import FlatGuarded, raw_bytes_equal, resize_ref, vptr

pytestmark = pytest.mark.gpu

F32, U8 = 0, 1                                          # NTK_IMAGE_F32, NTK_IMAGE_U8
BOUND = 2e-3
MEAN = np.array([123.68, 116.779, 103.939, 110.5], np.float32)
f64 = lambda a: np.asarray(a, np.float64)


def _image(H, W, C, seed):
    """Integer pixels 0..255 (the same values serve the fp32 and the u8 entry), both extremes present in the corners."""
    img = np.random.default_rng(seed).integers(0, 256, size=(H, W, C)).astype(np.float32)
    img[0, 0], img[-1, -1] = 0, 255
    img[0, -1], img[-1, 0] = 255, 0
    return img


def _axis(lo, hi, D, n):
    """float64 sample coordinates of one axis and, per sample, whether the kernel's fp32 arithmetic gives exactly that number (every
    intermediate representable: then contraction into an FMA cannot change it either)."""
    lo32, hi32, k = np.float32(lo), np.float32(hi), np.arange(n)
    if D == 1:                                          # every product with H - 1 = 0 is 0 in any precision
        return np.zeros(n), np.ones(n, bool)
    if n == 1:
        c64 = np.array([0.5 * (f64(lo32) + f64(hi32)) * (D - 1)])
        s32 = lo32 + hi32
        c32 = np.array([np.float32(0.5) * s32 * np.float32(D - 1)])
        exact = (f64(s32) == f64(lo32) + f64(hi32)) & (f64(c32) == c64)
        return c64, exact
    d32 = hi32 - lo32
    p32 = d32 * np.float32(D - 1)
    s32 = p32 / np.float32(n - 1)
    s64 = (f64(hi32) - f64(lo32)) * (D - 1) / (n - 1)
    o32 = lo32 * np.float32(D - 1)
    c64 = f64(lo32) * (D - 1) + k * s64
    ks32 = k.astype(np.float32) * s32
    c32 = o32 + ks32
    scale_exact = (f64(d32) == f64(hi32) - f64(lo32)) and (f64(p32) == f64(d32) * (D - 1)) and (f64(s32) == s64) \
        and (f64(o32) == f64(lo32) * (D - 1))
    return c64, scale_exact & (f64(ks32) == k * s64) & (f64(c32) == c64)


def assert_decidable(box, H, W, ch, cw):
    """Every sample is at least 1e-3 pixels inside or outside the image, or its fp32 coordinate is exact."""
    for lo, hi, D, n in ((box[0], box[2], H, ch), (box[1], box[3], W, cw)):
        c, exact = _axis(lo, hi, D, n)
        far = (np.abs(c) >= 1e-3) & (np.abs(c - (D - 1)) >= 1e-3)
        assert (far | exact).all(), (box, D, n, c[~(far | exact)])


class Img(object):
    def __init__(self, cuda):
        from ntmtrack import _lib
        self.cuda, self.L, self.lib, self.st = cuda, _lib.lib(), _lib, _lib.stream()

    def image(self, a):
        rows = a.shape[-2] * a.shape[-1]
        return FlatGuarded(a.shape, self.cuda, init=a, pad=(2 * rows + 63) // 64 * 64)

    def mean(self, C, on):
        return FlatGuarded((C,), self.cuda, init=MEAN[:C]) if on else None

    def crop(self, img, box, ch, cw, mean=True, extrapolation=0.0):
        H, W, C = img.shape
        out, m, gi = FlatGuarded((ch, cw, C), self.cuda), self.mean(C, mean), self.image(img)
        b = [float(np.float32(v)) for v in box]
        self.lib.check(self.L.ntk_crop_and_resize(gi.ptr, H, W, C, m.ptr if m else None, b[0], b[1], b[2], b[3], out.ptr, ch, cw,
                                                  extrapolation, self.st), "ntk_crop_and_resize")
        torch.cuda.synchronize()
        return out.written()

    def crop_batch(self, frames, dtype, frame_of, boxes, ch, cw, mean=True, extrapolation=0.0):
        F, H, W, C = frames.shape
        B = len(frame_of)
        if dtype == U8:
            assert (frames == np.floor(frames)).all() and frames.min() >= 0 and frames.max() <= 255
            dimg = torch.from_numpy(frames.astype(np.uint8)).to(self.cuda)
            iptr = vptr(dimg)
        else:
            dimg = self.image(frames)
            iptr = dimg.ptr
        fo = torch.tensor(list(frame_of), dtype=torch.int32, device=self.cuda)
        bx = FlatGuarded((B, 4), self.cuda, init=np.asarray(boxes, np.float32))
        out, m = FlatGuarded((B, ch, cw, C), self.cuda), self.mean(C, mean)
        self.lib.check(self.L.ntk_crop_and_resize_batch(iptr, dtype, F, H, W, C, vptr(fo), bx.ptr, m.ptr if m else None, out.ptr, B, ch, cw,
                                                        extrapolation, self.st), "ntk_crop_and_resize_batch")
        torch.cuda.synchronize()
        return out.written()

    def resize(self, img, OH, OW):
        H, W, C = img.shape
        out, gi = FlatGuarded((OH, OW, C), self.cuda), self.image(img)
        self.lib.check(self.L.ntk_resize_bilinear(gi.ptr, H, W, C, out.ptr, OH, OW, self.st), "ntk_resize_bilinear")
        torch.cuda.synchronize()
        return out.written()


@pytest.fixture(scope="module")
def dev(cuda):
    return Img(cuda)


def crop_ref(img, box, ch, cw, mean=True, extrapolation=0.0):
    C = img.shape[2]
    m = f64(MEAN[:C]) if mean else 0.0
    return OO.crop_and_resize(f64(img) - m, [float(np.float32(v)) for v in box], ch, cw, extrapolation)


def close(got, ref, what=""):
    err = float(np.max(np.abs(f64(got) - ref)))
    assert err <= BOUND, "%s: max |kernel - float64 oracle| = %.3g > %.3g" % (what, err, BOUND)


INSIDE, PARTLY = [0.1, 0.2, 0.8, 0.9], [-0.23, -0.1, 0.6, 1.3]
#        name                 image (H, W, C)  crop      box                       mean   extrapolation
CROPS = [("5x9_c1", (37, 53, 1), (5, 9), INSIDE, True, 0.0),
         ("5x9_c3", (37, 53, 3), (5, 9), INSIDE, True, 0.0),
         ("5x9_c4", (37, 53, 4), (5, 9), INSIDE, True, 0.0),
         ("9x5_c1", (37, 53, 1), (9, 5), INSIDE, True, 0.0),
         ("9x5_c3", (37, 53, 3), (9, 5), INSIDE, True, 0.0),
         ("9x5_c4", (37, 53, 4), (9, 5), INSIDE, True, 0.0),
         ("1x9", (37, 53, 3), (1, 9), INSIDE, True, 0.0),
         ("9x1", (37, 53, 3), (9, 1), INSIDE, True, 0.0),
         ("1x1_c1", (37, 53, 1), (1, 1), INSIDE, True, 0.0),
         ("1x1_outside", (37, 53, 3), (1, 1), [-0.9, 0.2, 0.1, 0.9], True, -7.5),           # centre row -0.4 * 36: outside
         ("one_row_image", (1, 53, 3), (5, 9), INSIDE, True, 0.0),
         ("one_column_image", (37, 1, 3), (5, 9), INSIDE, True, 0.0),
         ("one_pixel_image", (1, 1, 1), (5, 9), PARTLY, True, 0.0),                           # H - 1 = W - 1 = 0: all inside
         ("no_mean", (37, 53, 3), (5, 9), INSIDE, False, 0.0),
         ("partly_outside", (37, 53, 3), (9, 5), PARTLY, True, -7.5),
         ("partly_outside_no_mean", (37, 53, 4), (5, 9), PARTLY, False, -7.5),
         ("many_blocks", (37, 53, 3), (24, 40), PARTLY, True, -7.5),
         ("sides_64", (64, 64, 3), (9, 5), [0.05, 0.1, 0.95, 0.85], True, 0.0)]
FLIPS = [("flip_y", [0.8, 0.2, 0.1, 0.9], [0.1, 0.2, 0.8, 0.9], 0), ("flip_x", [0.1, 0.9, 0.8, 0.2], [0.1, 0.2, 0.8, 0.9], 1),
         ("flip_y_partly_outside", [0.6, -0.1, -0.23, 1.3], PARTLY, 0), ("flip_x_partly_outside", [-0.23, 1.3, 0.6, -0.1], PARTLY, 1)]


def _three_entries(dev, img, box, ch, cw, mean, ext, seed):
    """The one-box entry's crop, after asserting that the batched entry gives the same bits from fp32 and from u8 frames (B = 1, the
    image being the second of two frames)."""
    got = dev.crop(img, box, ch, cw, mean, ext)
    frames = np.stack([_image(*img.shape, seed=seed + 1), img])
    for dtype in (F32, U8):
        b = dev.crop_batch(frames, dtype, [1], [box], ch, cw, mean, ext)
        assert raw_bytes_equal(b[0], got), "batched entry, dtype %d" % dtype
    return got


@pytest.mark.parametrize("name,shape,crop,box,mean,ext", CROPS, ids=[c[0] for c in CROPS])
def test_crop_cases(dev, name, shape, crop, box, mean, ext):
    img = _image(*shape, seed=len(name))
    assert_decidable(box, shape[0], shape[1], crop[0], crop[1])
    ref = crop_ref(img, box, crop[0], crop[1], mean, ext)
    got = _three_entries(dev, img, box, crop[0], crop[1], mean, ext, len(name))
    close(got, ref, name)
    if ext != 0.0:
        outside = ref == ext
        assert outside.any() and raw_bytes_equal(got[outside], np.full(int(outside.sum()), ext, np.float32)), "extrapolation value as given"


@pytest.mark.parametrize("name,box,unflipped,axis", FLIPS, ids=[c[0] for c in FLIPS])
def test_flipped_boxes(dev, name, box, unflipped, axis):
    img = _image(37, 53, 3, seed=3)
    assert_decidable(box, 37, 53, 5, 9)
    got = _three_entries(dev, img, box, 5, 9, True, -7.5, 3)
    close(got, crop_ref(img, box, 5, 9, True, -7.5), name)
    close(got, f64(np.flip(dev.crop(img, unflipped, 5, 9, True, -7.5), axis)), name + ": the unflipped crop reversed")


EXACT = [((33, 65), (17, 9), (2, 8)), ((65, 33), (9, 17), (8, 2))]          # image, crop, pixel steps of the box [0, 0, 1, 1]


@pytest.mark.parametrize("mean", [True, False], ids=["mean", "no_mean"])
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("hw,crop,step", EXACT, ids=["33x65", "65x33"])
def test_exact_boxes_bit_for_bit(dev, hw, crop, step, C, mean):
    (H, W), (ch, cw), (sy, sx) = hw, crop, step
    img = _image(H, W, C, seed=H)
    m = MEAN[:C] if mean else np.zeros(C, np.float32)
    # the whole image: every (sy, sx)-th pixel, the last row and column included
    for box in ([0, 0, 1, 1], [0.5, 0.5, 1.5, 1.5]):
        for lo, hi, D, n in ((box[0], box[2], H, ch), (box[1], box[3], W, cw)):
            assert _axis(lo, hi, D, n)[1].all(), "every coordinate of an exact case is exact in fp32"
    got = _three_entries(dev, img, [0, 0, 1, 1], ch, cw, mean, -7.5, H)
    assert raw_bytes_equal(got, img[::sy, ::sx] - m)
    assert raw_bytes_equal(got[-1, -1], img[H - 1, W - 1] - m)
    # shifted by half the image: the in-image quadrant are the pixels (its last row and column the image's), the rest the value
    got = _three_entries(dev, img, [0.5, 0.5, 1.5, 1.5], ch, cw, mean, -7.5, H)
    want = np.full((ch, cw, C), -7.5, np.float32)
    qy, qx = (ch + 1) // 2, (cw + 1) // 2
    want[:qy, :qx] = img[(H - 1) // 2::sy, (W - 1) // 2::sx] - m
    assert raw_bytes_equal(got, want)
    # and by minus half: the first row and column of the image sit on in_y == 0, in_x == 0
    box = [-0.5, -0.5, 0.5, 0.5]
    assert _axis(box[0], box[2], H, ch)[1].all() and _axis(box[1], box[3], W, cw)[1].all()
    got = _three_entries(dev, img, box, ch, cw, mean, -7.5, H)
    want = np.full((ch, cw, C), -7.5, np.float32)
    want[ch - qy:, cw - qx:] = img[:(H - 1) // 2 + 1:sy, :(W - 1) // 2 + 1:sx] - m
    assert raw_bytes_equal(got, want)


def test_u8_extremes_equal_the_f32_entry(dev):
    """Frames of 0 and 255 only (a checkerboard of the two extremes): the u8 kernel converts exactly, the crops are bit-equal to the
    fp32 entry's and to the fp32 batch's, and within the bound of the oracle."""
    H, W, C = 37, 53, 3
    yy, xx = np.meshgrid(np.arange(H), np.arange(W), indexing="ij")
    img = np.repeat((((yy + xx) % 2) * 255.0)[:, :, None], C, axis=2).astype(np.float32)
    img[..., 1] = 255 - img[..., 1]
    for box in (INSIDE, PARTLY, [0, 0, 1, 1]):
        assert_decidable(box, H, W, 9, 5)
        got = _three_entries(dev, img, box, 9, 5, True, 0.0, 9)
        close(got, crop_ref(img, box, 9, 5), "checkerboard")


def test_seventy_boxes_over_three_frames(dev):
    H, W, C, ch, cw, B, F = 37, 53, 3, 5, 9, 70, 3
    frames = np.stack([_image(H, W, C, seed=20 + f) for f in range(F)])
    kinds = [INSIDE, PARTLY, [0.8, 0.2, 0.1, 0.9], [0.1, 0.9, 0.8, 0.2], [0, 0, 1, 1], [0.5, 0.5, 1.5, 1.5], [-0.5, -0.5, -0.1, -0.1]]
    rng = np.random.default_rng(70)
    boxes, frame_of = [], []
    for b in range(B):
        k = list(kinds[b % len(kinds)])
        if b >= len(kinds) and b % len(kinds) < 4:          # later rounds: the generic kinds moved a little, every box its own
            k = [float(v + d) for v, d in zip(k, rng.uniform(-0.02, 0.02, 4))]
        boxes.append([float(np.float32(v)) for v in k])
        frame_of.append(b % F if b not in (0, B - 1) else (0 if b == 0 else F - 1))
        assert_decidable(boxes[-1], H, W, ch, cw)
    assert 0 in frame_of and F - 1 in frame_of and frame_of[0] == 0 and frame_of[-1] == F - 1
    got = dev.crop_batch(frames, F32, frame_of, boxes, ch, cw, True, -7.5)
    assert raw_bytes_equal(dev.crop_batch(frames, U8, frame_of, boxes, ch, cw, True, -7.5), got)
    for b in range(B):
        close(got[b], crop_ref(frames[frame_of[b]], boxes[b], ch, cw, True, -7.5), "box %d" % b)
        if b < 2 * len(kinds):
            assert raw_bytes_equal(dev.crop(frames[frame_of[b]], boxes[b], ch, cw, True, -7.5), got[b]), b
    assert raw_bytes_equal(got[6], np.full((ch, cw, C), -7.5, np.float32))          # wholly outside


# --------------------------------------------------------------------------------------------------------------------- resize
@pytest.mark.parametrize("C", [1, 3])
def test_resize_exact_ratios_bit_for_bit(dev, C):
    img = _image(19, 23, C, seed=1) + np.float32(0.37)                       # identity keeps any pixel value
    assert raw_bytes_equal(dev.resize(img, 19, 23), img)
    img = _image(32, 48, C, seed=2) + np.float32(0.37)
    assert raw_bytes_equal(dev.resize(img, 16, 24), img[::2, ::2])
    img = _image(16, 24, C, seed=3)                                          # integers: halves and quarters are exact in fp32
    ref = resize_ref(img, 32, 48)
    assert (ref * 4 == np.round(ref * 4)).all()
    got = dev.resize(img, 32, 48)
    assert raw_bytes_equal(got, ref.astype(np.float32))
    assert raw_bytes_equal(got[-1, -1], img[-1, -1]) and raw_bytes_equal(got[::2, ::2], img)


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("src,dst", [((37, 53), (24, 40)), ((24, 40), (37, 53)), ((1, 1), (3, 2)), ((37, 53), (1, 1))],
                         ids=["down", "up", "from_one_pixel", "to_one_pixel"])
def test_resize_generic_ratios(dev, src, dst, C):
    img = _image(src[0], src[1], C, seed=src[0] + C)
    err = float(np.max(np.abs(f64(dev.resize(img, dst[0], dst[1])) - resize_ref(img, dst[0], dst[1]))))
    assert err <= BOUND, err
