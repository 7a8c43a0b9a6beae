"""Dev: fp32 error of Winograd F(4x4,3x3) vs F(2x2,3x3) vs a float64 direct convolution on VGG-like layer data
(numpy emulation of the kernel's arithmetic order: fp32 transforms, fp32 products accumulated over channels in fp32)."""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "tests"))
from conv_value_util import direct64, wino23, wino43        # the restatement lives with the tests that use it

rng = np.random.default_rng(0)


for C, O, H in ((64, 64, 16), (128, 128, 16), (256, 256, 12), (512, 512, 12)):
    x = np.maximum(rng.standard_normal((H, H, C)), 0).astype(np.float32) * 2       # post-ReLU-like activations
    w = (rng.standard_normal((3, 3, C, O)) * np.sqrt(2.0 / (9 * C))).astype(np.float32)
    ref = direct64(x, w)
    s = np.abs(ref).max()
    e2 = np.abs(wino23(x, w) - ref).max() / s
    e4 = np.abs(wino43(x, w) - ref).max() / s
    print("C%4d O%4d: F(2x2) %.2e   F(4x4) %.2e   (max abs error / max |y|)" % (C, O, e2, e4), flush=True)
