"""Fixtures of the validation-from-files tests: clips of the validator tests' shapes (tests/test_evaluate_gpu.py: 90 x 120 clips of
lengths [2, 3, 6, 4, 5], 64 x 80 clips of lengths [3, 2, 4]) written as JPEG files by Pillow at test time, from seeds
(tests/jpeg_util.py: image, encode).  Quality 90; one clip each 4:2:0, 4:4:4, 4:2:2 with a restart marker per MCU row, and gray,
the other 4:2:0 noise."""
import os

import numpy as np

import jpeg_util as J

H, W = 90, 120
LENGTHS = [2, 3, 6, 4, 5]
SMALL_H, SMALL_W, SMALL_LENGTHS = 64, 80, [3, 2, 4]
# per clip: (kind of image, keywords of Pillow's encoder; "gray" writes a one-component file)
KINDS = [("smooth", {"subsampling": 2}), ("smooth", {"subsampling": 0}), ("smooth", {"subsampling": 1, "restart_marker_rows": 1}),
         ("gray", {}), ("noise", {"subsampling": 2})]
SMALL_KINDS = [("smooth", {"subsampling": 2}), ("smooth", {"subsampling": 0}), ("noise", {"subsampling": 1, "restart_marker_rows": 1})]


def frame_file(h, w, kind, kw, seed):
    if kind == "gray":
        return J.encode(J.image(h, w, "smooth", seed)[:, :, 1].copy(), quality=90, **kw)
    return J.encode(J.image(h, w, kind, seed), quality=90, **kw)


def drifting_regions(rng, n, h, w):
    start = np.array([rng.uniform(0.15, 0.4) * w, rng.uniform(0.15, 0.4) * h, rng.uniform(0.25, 0.4) * w, rng.uniform(0.25, 0.4) * h])
    regions = start + np.cumsum(rng.uniform(-2, 2, size=(n, 4)), axis=0)
    regions[0] = start
    return regions


def write_clips(folder, lengths, h, w, kinds, seed, check_bits=False):
    """-> (clips with frames = lists of paths under `folder`, the files' bytes per clip).  check_bits: every file is inside the
    decoder's bit-exact domain -- the NumPy restatement of the decoder gives Pillow's bytes for it."""
    from ntmtrack.evaluate import Clip
    rng = np.random.default_rng(seed)
    clips, contents = [], []
    for i, (n, (kind, kw)) in enumerate(zip(lengths, kinds)):
        paths, files = [], []
        for k in range(n):
            data = frame_file(h, w, kind, kw, seed * 100 + i * 10 + k)
            if check_bits:
                assert (J.decode(data) == J.pillow_decode(data)).all(), "clip %d frame %d" % (i, k)
            path = os.path.join(str(folder), "%dx%d_clip%d_%08d.jpg" % (h, w, i, k + 1))
            with open(path, "wb") as f:
                f.write(data)
            paths.append(path)
            files.append(data)
        clips.append(Clip(paths, drifting_regions(rng, n, h, w)))
        contents.append(files)
    return clips, contents


def array_clips(clips, contents):
    """The same clips as uint8 arrays decoded by Pillow: today's path."""
    from ntmtrack.evaluate import Clip
    return [Clip(np.stack([J.pillow_decode(d) for d in files]), c.regions, c.init) for c, files in zip(clips, contents)]


def truncated(h, w, seed):
    """tests/jpeg_util.truncated_file's recipe at h x w: a 4:2:0 noise file whose scan is cut to 40 % of its bytes (no restart
    markers, no EOI): the parser accepts it, the decoder runs out of data (NTK_JPEG_STATUS_TRUNCATED = 2)."""
    data = J.encode(J.image(h, w, "noise", seed), quality=90, subsampling=2)
    start = J.parse(data)["scan_start"]
    return data[:start + int(0.4 * (len(data) - start))]
