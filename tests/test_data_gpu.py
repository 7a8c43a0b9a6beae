"""GPU: get_input (format (B) -> the four tensors): resize(720x1280) - mean, crop_and_resize(224) vs a numpy chain."""
import os

import numpy as np
import pytest
import torch

from oracle import online_oracle as OO
from small_kernel_util import resize_ref as _resize_ref

pytestmark = pytest.mark.gpu


def test_get_input_matches_numpy_chain(cuda, tmp_path):
    from PIL import Image
    from ntmtrack import data
    rng = np.random.default_rng(0)
    d = tmp_path / "train_seq_0"
    d.mkdir()
    names = []
    for i in range(2):
        arr = rng.integers(0, 256, size=(60, 80, 3), dtype=np.uint8)
        png = str(d / ("img%d.png" % i))
        Image.fromarray(arr).save(png)
        stem = str(d / ("%06d" % i))
        gt = rng.random((8, 8)); gt.tofile(stem + ".bin")
        with open(stem + ".txt", "w") as f:
            f.write("0.1,0.15,0.9,0.8,0.3,0.3,0.6,0.6,%s,%g,%g" % (png, 0.05 * i, -0.1 * i))
        names.append(stem)
    img, gts, yo, xo = data.get_input(names, device=cuda)
    torch.cuda.synchronize()
    assert img.shape == (2, 224, 224, 3) and gts.shape == (2, 8, 8)
    np.testing.assert_allclose(yo.cpu().numpy(), [0.0, 0.05], atol=1e-7)
    np.testing.assert_allclose(xo.cpu().numpy(), [0.0, -0.1], atol=1e-7)
    arr0 = np.asarray(Image.open(str(d / "img0.png")).convert("RGB"), dtype=np.float64)
    big = _resize_ref(arr0, 720, 1280) - np.array(data.VGG_MEAN)
    ref = OO.crop_and_resize(big, [0.1, 0.15, 0.9, 0.8], 224, 224)
    np.testing.assert_allclose(img[0].cpu().numpy(), ref, atol=5e-3)
