"""Where "the bits of Pillow's decode" stops holding for the device JPEG decoder (CPU only; DESIGN.md §4.5 records the output).

libjpeg-turbo, which Pillow links, runs a SIMD inverse DCT whose intermediates are saturating 16-bit values; the device kernel and
its NumPy restatement (tests/jpeg_util.py) keep int32 throughout.  Files from a real encoder hold dequantised coefficients within
about +-1024 and never notice.  This script finds the boundary: it takes a quality-100 noise file (every quantisation value 1, so
the coefficients are large), overwrites every quantisation value of the file with q = 1, 2, ... and reports, per q, the blocks in
which Pillow and the restatement differ, the largest dequantised coefficient and the largest column-pass output.

    python scripts/jpeg_domain_boundary.py"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import jpeg_util as J  # noqa: E402


def with_quantiser(data, q):
    """the file with every value of every DQT table set to q"""
    b, p = bytearray(data), 2
    while b[p + 1] != 0xDA:
        L = (b[p + 2] << 8) | b[p + 3]
        if b[p + 1] == 0xDB:
            for i in range(p + 4, p + 2 + L, 65):
                b[i + 1:i + 65] = bytes([q]) * 64
        p += 2 + L
    return bytes(b)


def main():
    base = J.encode(J.image(48, 64, "noise"), quality=100, subsampling=0)
    first = None
    for q in list(range(1, 17)) + [24, 32]:
        data = with_quantiser(base, q)
        info = J.parse(data)
        coef, _hs, _vs = J.coefficients(info)
        deq = coef * q
        cols = J._idct8(np.swapaxes(deq.reshape(deq.shape[:-1] + (8, 8)), -1, -2), 11)
        diff = (J.decode(data) != J.pillow_decode(data)).any(axis=-1)
        blocks = diff.reshape(diff.shape[0] // 8, 8, diff.shape[1] // 8, 8).any(axis=(1, 3))
        print("q = %2d: %2d of %d 8x8 pixel blocks differ; largest dequantised coefficient %5d, largest column-pass output %6d"
              % (q, int(blocks.sum()), blocks.size, int(np.abs(deq).max()), int(np.abs(cols).max())))
        if first is None and blocks.any():
            first = (q, int(np.abs(deq).max()))
    print("first difference at q = %s, where the largest dequantised coefficient is %s" % (first or ("none", "-")))


if __name__ == "__main__":
    main()
