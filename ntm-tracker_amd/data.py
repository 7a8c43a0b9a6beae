"""Input contract of the tracking path ("sequence_generator input contract").

Two generations exist in the reference:
 (A) legacy pickle from sequence_generator.py:76-154: a list of
     ``(seq_dir, obj_name, subseq_id, seq_len, [(frame.JPEG, (w,h), bbox, [gt maps])])`` consumed by
     ``default_get_batch`` (direct_offset_output.py:122-142);
 (B) current on-disk format from preprocess.py:321-334: ``<out>/<seq>_<track>/NNNNNN.txt`` (one CSV line
     ``crop_y1,crop_x1,crop_y2,crop_x2,bbox_y1,bbox_x1,bbox_y2,bbox_x2,image_path,y_offset,x_offset``) and
     ``NNNNNN.bin`` (8x8 float64 heat-map, 512 bytes), enumerated by ``get_valid_sequences`` (:94-120), batched
     by ``sevenbyseven_get_batch`` (:144-157) and decoded by ``get_input`` (:159-224) into the four tensors the
     hot path consumes: batch_img [B*T,224,224,3] (mean-subtracted), batch_gt [B*T,8,8], y_offsets, x_offsets.
Host-side file parsing is plain Python; the image math (resize to 720x1280, mean subtraction, crop_and_resize to
224x224) runs in HIP kernels.  ``SyntheticSequences`` produces the same four tensors without a dataset.
``get_input`` does the image math frame by frame; ``get_input_batch`` (second half of this file) gives the same tensors, bit for
bit, from ONE launch over the packed uint8 frames, with the decoding on a thread pool, and ``InputPrefetcher`` stages the next
batch while the current one trains (``train.fit`` is the loop that uses them).
"""
import collections
import os

import numpy as np
import torch

from . import _lib
from .geometry import apply_transformation, calculate_transformation, discrete_gauss
from .regions import MASK_MAX_PIXELS, POLY_DOUBLES, POLY_MAX_POINTS, Clip, MaskRegions, rect_polygons

VGG_MEAN = (123.68, 116.78, 103.94)


SPLITS = ("train", "val")


def _stems(seqdir, suffix=".txt"):
    """Frame stems ('000000', ...) of one <seq>_<track> folder, in name order."""
    return sorted(name[:-len(suffix)] for name in os.listdir(seqdir) if name.endswith(suffix))


def get_valid_sequences(sequences_dir, min_length):
    """Enumerate the format-(B) folders under `sequences_dir` that hold at least `min_length` frames.

    Contract (behaviour of direct_offset_output.py:94-120): a folder with n >= min_length frame records is
    subsampled with the integer stride n // min_length starting at its first frame, keeping exactly min_length
    stems; shorter folders are dropped.  Returns (all, train, val), each a list of (folder, stems); the split is
    decided by 'train' / 'val' appearing in the folder path ('train' is tested first), and a folder that names
    neither is an error."""
    everything = []
    by_split = {name: [] for name in SPLITS}
    for entry in sorted(os.listdir(sequences_dir)):
        folder = os.path.join(sequences_dir, entry)
        stems = _stems(folder)
        stride = len(stems) // min_length
        if stride < 1:
            continue
        item = (folder, stems[0:(min_length - 1) * stride + 1:stride])
        split = next((name for name in SPLITS if name in folder), None)
        everything.append(item)
        if split is None:
            raise ValueError("sequence folder %r names neither of the splits %s" % (folder, "/".join(SPLITS)))
        by_split[split].append(item)
    return everything, by_split["train"], by_split["val"]


def default_get_batch(index, batch_size, seq_length, seqs):
    """Legacy pickle contract (A) (behaviour of direct_offset_output.py:122-142): `seqs` holds records
    (seq_dir, obj_name, subseq_id, seq_len, frames) with frames = [(path, (w, h), bbox, [gt maps per layer])].
    Takes records [index, index + batch_size), the first `seq_length` frames of each, and returns
    (frame paths flattened [B*T], first-layer gt maps flattened to [B, T, F], index + batch_size)."""
    stop = index + batch_size
    names, gts = [], []
    for record in seqs[index:stop]:
        frames = record[4][:seq_length]
        names.extend(frame[0] for frame in frames)
        gts.append(np.array([np.asarray(frame[-1][0]).reshape(-1) for frame in frames]))
    return names, np.array(gts), stop


def sevenbyseven_get_batch(index, batch_size, seqs):
    """Format (B) batching (behaviour of direct_offset_output.py:144-157): `seqs` as returned by
    get_valid_sequences; -> (frame paths without suffix [B*T], index + batch_size)."""
    stop = index + batch_size
    names = [os.path.join(folder, stem) for folder, stems in seqs[index:stop] for stem in stems]
    return names, stop


def load_frame_record(path_nosuffix, gt_width=8):
    """One frame of format (B): the CSV line and the float64 heat-map."""
    with open(path_nosuffix + '.txt') as f:
        fields = f.readline().strip().split(',')
    if len(fields) != 11:
        raise ValueError("%s.txt: expected 11 comma-separated fields, got %d" % (path_nosuffix, len(fields)))
    vals = [float(v) for v in fields[:8]]
    raw = np.fromfile(path_nosuffix + '.bin', dtype=np.float64)
    if raw.size != gt_width * gt_width:
        raise ValueError("%s.bin: expected %d float64 values, got %d" % (path_nosuffix, gt_width * gt_width, raw.size))
    return {"cropbox": vals[:4], "bbox": vals[4:8], "image_path": fields[8], "y_offset": float(fields[9]),
            "x_offset": float(fields[10]), "gt": raw.astype(np.float32).reshape(gt_width, gt_width)}


def load_frame_region(path_nosuffix):
    """The object box of one frame record as the tracker's contract takes it (behaviour of validate_tracker.py:12-24): only the
    ``.txt`` line is read, not the heat-map.  The record holds the box in CROP coordinates; it goes back through the inverse of
    the crop transformation.  -> (image_path, (x, y, w, h) normalised by (W-1, H-1))."""
    with open(path_nosuffix + '.txt') as f:
        fields = f.readline().strip().split(',')
    if len(fields) < 9:
        raise ValueError("%s.txt: expected at least 9 comma-separated fields, got %d" % (path_nosuffix, len(fields)))
    vals = [float(v) for v in fields[:8]]
    inverse = np.linalg.inv(calculate_transformation(vals[:4]))
    y1, x1, y2, x2 = apply_transformation(vals[4:8], inverse)
    return fields[8], (x1, y1, x2 - x1, y2 - y1)


def pixel_region(size, normalized_region):
    """Normalised (x, y, w, h) -> pixels, size = (width, height): the inverse of geometry.normalize_bbox, times (W-1, H-1)."""
    width, height = size
    return tuple(np.asarray(normalized_region, dtype=np.float64) * np.array([width - 1, height - 1, width - 1, height - 1], dtype=np.float64))


CLIP_FRAMES = ("arrays", "files")


def _clip_frames(paths, frames):
    """What a clip reader puts into Clip.frames: frames="arrays" a callable that decodes the whole clip with Pillow (float32
    [L,H,W,3]) when the validator schedules it; frames="files" the list of paths itself -- a file clip, which the validator reads
    a round at a time (evaluate.Validation, decode=)."""
    if frames == "files":
        return list(paths)
    return lambda paths=paths: np.stack([_decode_image(p) for p in paths])


def _check_clip_frames(frames):
    if frames not in CLIP_FRAMES:
        raise ValueError("frames must be 'arrays' or 'files', not %r" % (frames,))


def validation_clips(seqs, image_root=None, frames="arrays"):
    """``seqs`` as get_valid_sequences returns them -> one evaluate.Clip per sequence (the reference's validation loop,
    validate_tracker.py:26-38).  Only the first image's header is opened here (for the frame size); a clip's frames are decoded
    when the validator schedules it (frames="files": a round at a time, from the paths; _clip_frames).  The tracker is started
    with the first region NORMALISED, as the reference passes it (the trackers take a region whose four numbers are below 1 as
    normalised); the ground truth for scoring is in pixels."""
    from PIL import Image
    _check_clip_frames(frames)
    clips = []
    for folder, stems in seqs:
        records = [load_frame_region(os.path.join(folder, stem)) for stem in stems]
        paths = [p if image_root is None else os.path.join(image_root, p) for p, _r in records]
        with Image.open(paths[0]) as im:
            width, height = im.size
        regions = np.array([pixel_region((width, height), r) for _p, r in records], dtype=np.float64)
        clips.append(Clip(_clip_frames(paths, frames), regions, init=records[0][1], size=(height, width)))
    return clips


def parse_vot_region(line):
    """One line of a VOT groundtruth.txt as vot.py:27-33 (parse_region) reads it: 4 numbers are a rectangle (x, y, w, h), an even
    count above 4 a polygon (x0, y0, x1, y1, ...).  -> a list of 4 or of 2P floats, or None for a line that is neither (an absent
    object).  A polygon of more than evaluate.POLY_MAX_POINTS points is an error: the device layout cannot hold it."""
    try:
        tokens = [float(t) for t in line.strip().split(',')]
    except ValueError:
        return None
    if len(tokens) == 4:
        return tokens
    if len(tokens) > 4 and len(tokens) % 2 == 0:
        if len(tokens) > POLY_DOUBLES:
            raise ValueError("a region of %d points; at most %d are supported" % (len(tokens) // 2, POLY_MAX_POINTS))
        return tokens
    return None


def parse_vot_mask(line):
    """One mask line of a VOT groundtruth.txt, ``m x0,y0,w,h,c0,c1,...`` (the sets from 2020 on): the mask's box in frame pixels
    and the run-length counts over it, even-indexed counts runs of zeros, odd-indexed ones runs of ones, row-major.
    -> (x0, y0, w, h, counts int32 array), the counts as they are written (evaluate.MaskRegions, include/ntmtrack.h NTK_MASK_*).
    ValueError, with the reason: a line that does not begin with ``m``, fewer than four numbers, a number that is not an integer
    (of 32 bits), a negative count, a box of more than evaluate.MASK_MAX_PIXELS pixels.  A box with w <= 0 or h <= 0 is returned as it is: an absent object."""
    text = line.strip()
    if not text.startswith("m"):
        raise ValueError("not a mask line (it does not begin with 'm'): %r" % (text[:40],))
    tokens = [t.strip() for t in text[1:].split(",")]
    if tokens == [""]:
        tokens = []
    if len(tokens) < 4:
        raise ValueError("a mask line of %d number(s); at least x0,y0,w,h are needed" % len(tokens))
    numbers = []
    for t in tokens:
        try:
            v = int(t)
        except ValueError:
            raise ValueError("a mask line holds %r, which is not an integer" % (t,))
        if not -2 ** 31 <= v < 2 ** 31:
            raise ValueError("a mask line holds %d, which does not fit 32 bits" % v)
        numbers.append(v)
    x0, y0, w, h = numbers[:4]
    if w > 0 and h > 0 and w * h > MASK_MAX_PIXELS:
        raise ValueError("a mask box of %d x %d pixels; at most %d pixels are supported" % (w, h, MASK_MAX_PIXELS))
    counts = np.asarray(numbers[4:], dtype=np.int32)
    if (counts < 0).any():
        raise ValueError("a mask line holds the negative count %d" % int(counts[counts < 0][0]))
    return x0, y0, w, h, counts


def _vot_mask_regions(path, lines):
    """The lines of a groundtruth.txt that holds mask lines -> evaluate.MaskRegions: a line that is neither a mask nor parseable
    is an absent object, a rectangle or polygon line among them a ValueError naming the file and the line."""
    frames = []
    for k, line in enumerate(lines):
        try:
            if line.strip().startswith("m"):
                frames.append(parse_vot_mask(line))
            elif parse_vot_region(line) is None:
                frames.append(None)
            else:
                raise ValueError("a rectangle or polygon among mask lines")
        except ValueError as e:
            raise ValueError("%s, line %d: %s" % (path, k + 1, e))
    return MaskRegions.from_lists(frames)


def vot_clips(root, names=None, frames="arrays"):
    """The VOT directory layout -> one evaluate.Clip per sequence.  ``root/list.txt`` names the sequences when ``names`` is None.
    A ``groundtruth.txt`` that holds mask lines (``m x0,y0,w,h,c0,...``: parse_vot_mask) gives a mask clip, its regions an
    evaluate.MaskRegions; a line of it that is neither a mask nor parseable is an absent object, a rectangle or polygon line
    among the mask lines a ValueError naming the file and the line.  Otherwise:
    A sequence folder holds ``groundtruth.txt``, one region per line (parse_vot_region; a line that is neither form is an absent
    object, a row of NaN), and its frames as ``color/%08d.jpg`` or ``%08d.jpg``, numbered from 1.  Regions are in pixels: [L,4]
    where every line is a rectangle or absent, else [L,16] polygons padded with NaN (a rectangle line among them as its 4-gon).
    Only the first image's header is opened here (for ``size``); a clip's frames are decoded when the validator schedules it
    (frames="files": a round at a time, from the paths; _clip_frames)."""
    from PIL import Image
    _check_clip_frames(frames)
    if names is None:
        with open(os.path.join(root, "list.txt")) as f:
            names = [line.strip() for line in f if line.strip()]
    clips = []
    for name in names:
        folder = os.path.join(root, name)
        with open(os.path.join(folder, "groundtruth.txt")) as f:
            lines = f.read().splitlines()
        while lines and not lines[-1].strip():
            lines.pop()
        masks = any(line.strip().startswith("m") for line in lines)
        try:
            parsed = lines if masks else [parse_vot_region(line) for line in lines]
        except ValueError as e:
            raise ValueError("%s: %s" % (os.path.join(folder, "groundtruth.txt"), e))
        if masks:
            regions = _vot_mask_regions(os.path.join(folder, "groundtruth.txt"), lines)
        elif any(r is not None and len(r) > 4 for r in parsed):
            regions = np.full((len(parsed), POLY_DOUBLES), np.nan)
            for i, r in enumerate(parsed):
                if r is not None:
                    corners = rect_polygons(r)[:8] if len(r) == 4 else r
                    regions[i, :len(corners)] = corners
        else:
            regions = np.array([[np.nan] * 4 if r is None else r for r in parsed], dtype=np.float64).reshape(-1, 4)
        sub = "color" if os.path.isdir(os.path.join(folder, "color")) else ""
        paths = [os.path.join(folder, sub, "%08d.jpg" % (i + 1)) for i in range(len(parsed))]
        with Image.open(paths[0]) as im:
            width, height = im.size
        clips.append(Clip(_clip_frames(paths, frames), regions, size=(height, width)))
    return clips


def _decode_image(file, dtype=np.float32):
    """Pillow's RGB pixels of an image file (a path, or the file's bytes) -> `dtype` [H,W,3]: the one host decoder."""
    import io
    from PIL import Image
    with Image.open(io.BytesIO(file) if isinstance(file, bytes) else file) as im:
        return np.asarray(im.convert("RGB"), dtype=dtype)


def preprocess_frame(image, cropbox, device, resize_to=(720, 1280), crop=224, out=None):
    """image [H,W,3] float array -> mean-subtracted 224x224 crop on the device
    (direct_offset_output.py:193-211: resize_images(720x1280) - VGG_MEAN, then crop_and_resize)."""
    L, P = _lib.lib(), _lib.ptr
    img = torch.as_tensor(image, dtype=torch.float32).to(device).contiguous()
    H, W, C = img.shape
    big = torch.empty((resize_to[0], resize_to[1], C), device=device)
    _lib.check(L.ntk_resize_bilinear(P(img), H, W, C, P(big), resize_to[0], resize_to[1], _lib.stream()), "ntk_resize_bilinear")
    if out is None:
        out = torch.empty((crop, crop, C), device=device)
    mean = torch.tensor(VGG_MEAN, device=device)
    y1, x1, y2, x2 = [float(v) for v in cropbox]
    _lib.check(L.ntk_crop_and_resize(P(big), resize_to[0], resize_to[1], C, P(mean), y1, x1, y2, x2, P(out), crop, crop, 0.0,
                                     _lib.stream()), "ntk_crop_and_resize")
    return out


def get_input(frame_names_nosuffix, device="cuda", reverse_image=False, image_root=None):
    """direct_offset_output.py:159-224 -> (batch_img [n,224,224,3], batch_gt [n,8,8], y_offsets [n], x_offsets [n])."""
    n = len(frame_names_nosuffix)
    dev = torch.device(device)
    batch_img = torch.empty((n, 224, 224, 3), device=dev)
    gts, ys, xs = [], [], []
    for i, name in enumerate(frame_names_nosuffix):
        rec = load_frame_record(name)
        path = rec["image_path"] if image_root is None else os.path.join(image_root, rec["image_path"])
        preprocess_frame(_decode_image(path), rec["cropbox"], dev, out=batch_img[i])
        gts.append(rec["gt"]); ys.append(rec["y_offset"]); xs.append(rec["x_offset"])
    batch_gt = torch.from_numpy(np.stack(gts)).to(dev)
    y_off = torch.tensor(ys, dtype=torch.float32, device=dev)
    x_off = torch.tensor(xs, dtype=torch.float32, device=dev)
    if reverse_image:                                   # :187-188, :203-204
        x_off = -x_off
        batch_img = torch.flip(batch_img, dims=[2])
    return batch_img, batch_gt, y_off, x_off


class SyntheticSequences(object):
    """The four tensors of the contract without a dataset: frames U[0,255) - VGG_MEAN, frame-0 heat-map
    = discrete_gauss((.5,.5),(8,8),1), offsets U(-.5,.5) with frame 0 = 0."""

    def __init__(self, batch_size, sequence_length, seed=42, device="cuda"):
        self.B, self.T, self.seed, self.device = batch_size, sequence_length, seed, torch.device(device)

    def batch(self, step=0):
        B, T = self.B, self.T
        g = torch.Generator(device="cpu").manual_seed(self.seed + step)
        mean = torch.tensor(VGG_MEAN)
        frames = torch.empty((B * T, 224, 224, 3), dtype=torch.float32)
        for i in range(0, B * T, 64):
            n = min(64, B * T - i)
            frames[i:i + n] = torch.rand((n, 224, 224, 3), generator=g) * 255.0 - mean
        hm = discrete_gauss((.5, .5), (8, 8), 1.0)
        gts = torch.from_numpy(np.tile(hm.astype(np.float32)[None], (B * T, 1, 1)))
        offs = torch.rand((B, T, 2), generator=g) - 0.5
        offs[:, 0, :] = 0
        d = self.device
        return frames.to(d), gts.to(d), offs[:, :, 0].reshape(-1).to(d), offs[:, :, 1].reshape(-1).to(d)


# ---------------------------------------------------------------------------------------------------------------------------
# The batched input path: uint8 frames packed into one pinned buffer, three uploads and ONE ntk_frames_crop_batch launch per
# batch (get_input above stays as the per-frame statement of the same contract; the two give the same bits).
# ---------------------------------------------------------------------------------------------------------------------------

RESIZE_TO = (720, 1280)
CROP = (224, 224)
FRAME_TABLE_COLS = 7            # byte_offset, H, W, y0, x0, h, w  (NTK_FRAME_TABLE_COLS)
MAX_FRAMES_PER_LAUNCH = 65535   # blockIdx.y = frame


def default_workers():
    """Decoder threads: the CPUs this process may run on, at most 16 (never the machine's CPU count)."""
    return max(1, min(16, len(os.sched_getaffinity(0))))


def _axis_source_range(size, resized, crop_n, lo, hi, margin):
    """One axis of crop_source_rect: (first, count) of the source indices the composed sampling can touch, or None."""
    scale = float(resized - 1)
    if crop_n > 1:
        step = (hi - lo) * scale / float(crop_n - 1)
        ends = (lo * scale, lo * scale + float(crop_n - 1) * step)
    else:
        ends = (0.5 * (lo + hi) * scale,) * 2
    a, b = min(ends), max(ends)
    if not (np.isfinite(a) and np.isfinite(b)) or b < -1.0 or a > scale + 1.0:
        return None
    # taps of the crop stage are rows floor(v) and ceil(v) of the resized image for the samples v inside [0, resized-1]; one
    # resized row more on either side absorbs the fp32 rounding of v against this float64 restatement
    r0 = int(max(0.0, np.floor(max(a, 0.0)) - 1.0))
    r1 = int(min(scale, np.ceil(min(b, scale)) + 1.0))
    # resized row r reads source rows floor(r * size / resized) and the next one
    ratio = float(size) / float(resized)
    s0 = int(np.floor(r0 * ratio)) - margin
    s1 = int(np.floor(r1 * ratio)) + 1 + margin
    s0, s1 = max(0, min(s0, size - 1)), max(0, min(s1, size - 1))
    return s0, s1 - s0 + 1


def crop_source_rect(size_hw, cropbox, resize_to=RESIZE_TO, crop=CROP, margin=2):
    """The rectangle (y0, x0, h, w) of a source image of size_hw = (H, W) that ntk_frames_crop_batch can read for `cropbox`
    (y1, x1, y2, x2, normalised): the source pixels behind every tap of crop_and_resize(resize_images(image, resize_to), cropbox)
    to `crop`, widened by one row / column of the resized image (the kernel's fp32 sample positions against this float64
    restatement) and by `margin` source pixels, clipped to the image.  A box whose samples all fall outside the image touches
    nothing: the result is then the 1x1 rectangle at the origin.  Pure NumPy, float64."""
    H, W = int(size_hw[0]), int(size_hw[1])
    y1, x1, y2, x2 = [float(v) for v in cropbox]
    rows = _axis_source_range(H, int(resize_to[0]), int(crop[0]), y1, y2, int(margin))
    cols = _axis_source_range(W, int(resize_to[1]), int(crop[1]), x1, x2, int(margin))
    if rows is None or cols is None:
        return 0, 0, 1, 1
    return rows[0], cols[0], rows[1], cols[1]


def check_frame_table(table, pixels_bytes, channels):
    """Host validation of a frame table (the kernel repeats it per row and turns a bad row into the extrapolation value; here a
    bad row is an error, since the host built it): every rectangle non-empty, inside its image and inside the buffer."""
    t = np.asarray(table)
    if t.ndim != 2 or t.shape[1] != FRAME_TABLE_COLS or t.dtype != np.int64:
        raise ValueError("frame table must be int64 [n,%d], not %s %s" % (FRAME_TABLE_COLS, t.dtype, t.shape))
    for i, (off, H, W, y0, x0, h, w) in enumerate(t.tolist()):
        if H < 1 or W < 1 or h < 1 or w < 1 or y0 < 0 or x0 < 0 or y0 + h > H or x0 + w > W:
            raise ValueError("frame table row %d: rectangle y0=%d x0=%d h=%d w=%d leaves the %dx%d image" % (i, y0, x0, h, w, H, W))
        if off < 0 or off + h * w * channels > pixels_bytes:
            raise ValueError("frame table row %d: bytes [%d, %d) leave the buffer of %d bytes"
                             % (i, off, off + h * w * channels, pixels_bytes))


class Staging(object):
    """One set of host staging buffers of the batched path, owned and reused by the caller: pixels (uint8), the frame table
    (int64 [n,7]), the boxes (fp32 [n,4]) and the labels (fp32 [n,66]: the 8x8 heat-map, y offset, x offset).  Pinned where a
    device is present (pin=None), so that the uploads can be asynchronous.  Buffers grow when a batch needs more."""

    def __init__(self, pin=None):
        self.pin = torch.cuda.is_available() if pin is None else bool(pin)
        self.pixels = self._new((0,), torch.uint8)
        self.table = self._new((0, FRAME_TABLE_COLS), torch.int64)
        self.boxes = self._new((0, 4), torch.float32)
        self.labels = self._new((0, 66), torch.float32)
        # decode="device": the unstuffed scans, one descriptor per frame and the restart-segment table (ntk_jpeg_parse writes them)
        self.streams = self._new((0,), torch.uint8)
        self.descs = self._new((0, JPEG_DESC_BYTES), torch.uint8)
        self.segments = self._new((0,), torch.int32)
        self._device = {}               # device buffers of this set, grown and reused: no allocator call in the steady state

    def _new(self, shape, dtype):
        return torch.empty(shape, dtype=dtype, pin_memory=self.pin)

    def fits(self, nbytes, n, jpeg=None):
        """Room for nbytes of pixels, n frames and, with `jpeg` = (stream bytes, segments), their JPEG part?"""
        return self.pixels.numel() >= nbytes and self.table.shape[0] >= n and (jpeg is None or self.fits_jpeg(jpeg[0], n, jpeg[1]))

    def ensure(self, nbytes, n, jpeg=None):
        """Grow (with a quarter of headroom, so that batches of slightly different size do not grow it again)."""
        if self.pixels.numel() < nbytes:
            self.pixels = self._new((nbytes + nbytes // 4,), torch.uint8)
        if self.table.shape[0] < n:
            self.table = self._new((n, FRAME_TABLE_COLS), torch.int64)
            self.boxes = self._new((n, 4), torch.float32)
            self.labels = self._new((n, 66), torch.float32)
        if jpeg is not None:
            self.ensure_jpeg(jpeg[0], n, jpeg[1])

    def fits_jpeg(self, stream_bytes, n, n_segments):
        return self.streams.numel() >= stream_bytes and self.descs.shape[0] >= n and self.segments.numel() >= n_segments

    def ensure_jpeg(self, stream_bytes, n, n_segments):
        if self.streams.numel() < stream_bytes:
            self.streams = self._new((stream_bytes + stream_bytes // 4,), torch.uint8)
        if self.descs.shape[0] < n:
            self.descs = self._new((n, JPEG_DESC_BYTES), torch.uint8)
        if self.segments.numel() < n_segments:
            self.segments = self._new((n_segments + n_segments // 4,), torch.int32)

    def adopt(self, packed):
        """Move a batch that was packed into another set into this one: grow, copy what the batch uses of EVERY buffer a set has
        (a buffer added above belongs in this list) -> the PackedFrames in this set."""
        old, n, j = packed.staging, packed.n, packed.jpeg
        jpeg = None if j is None else (j.stream_bytes, j.n_segments)
        self.ensure(packed.nbytes, n, jpeg)
        used = [("pixels", packed.nbytes), ("table", n), ("boxes", n), ("labels", n)]
        if j is not None:
            used += [("streams", jpeg[0]), ("descs", n), ("segments", jpeg[1])]
        for name, k in used:
            getattr(self, name)[:k].copy_(getattr(old, name)[:k])
        moved = PackedFrames(self, packed.nbytes, n, packed.channels, packed.resize_to, packed.crop)
        moved.jpeg = j
        return moved

    def device_buffer(self, dev, name, numel, dtype):
        """The first `numel` elements of this set's device buffer `name` (grown with a quarter of headroom when too small)."""
        key = (str(dev), name)
        buf = self._device.get(key)
        if buf is None or buf.numel() < numel or buf.dtype != dtype:
            buf = self._device[key] = torch.empty((numel + numel // 4,), dtype=dtype, device=dev)
        return buf[:numel]


class PackedFrames(object):
    """pack_frames' result: views of the first `nbytes` bytes / n rows of a Staging set."""

    def __init__(self, staging, nbytes, n, channels, resize_to, crop):
        self.staging, self.nbytes, self.n, self.channels = staging, nbytes, n, channels
        self.resize_to, self.crop = tuple(resize_to), tuple(crop)
        self.pixels, self.table, self.boxes = staging.pixels[:nbytes], staging.table[:n], staging.boxes[:n]
        self.jpeg = None                # JpegPart when frames of this batch are decoded on the device (pack_jpeg_frames)
        self.status = None              # int32 [n] on the device after frames_crop_batch of such a batch


def _check_pack(pack):
    if pack not in ("rect", "full"):
        raise ValueError("pack must be 'rect' or 'full', not %r" % (pack,))


def _place(sizes, rects, channels, boxes, staging, grow, pad=0, offsets=None, jpeg=None):
    """The layout-and-fit step of both packers.  sizes (H, W) and rects (y0, x0, h, w) per frame: the rectangles get their byte
    offsets in the pixel buffer -- back to back behind `pad` bytes, or the caller's `offsets` = (offset per frame, the buffer's
    size); the Staging set is chosen (`staging`, made when None; one that is too small for the pixels, the rows and the `jpeg` =
    (stream bytes, segments) part grows, or with grow=False gives way to a fresh unpinned set); the frame table is written and
    checked (check_frame_table) and the boxes (nullable) are written.  -> (the set, the table's rows, the pixel bytes)."""
    n = len(rects)
    rows, off = [], int(pad)
    for i, ((H, W), (y0, x0, h, w)) in enumerate(zip(sizes, rects)):
        if offsets is not None:
            off = int(offsets[0][i])
        rows.append((off, H, W, y0, x0, h, w))
        off += h * w * channels
    nbytes = off if offsets is None else int(offsets[1])
    if staging is None:
        staging = Staging()
    if not staging.fits(nbytes, n, jpeg):
        if not grow:
            staging = Staging(pin=False)
        staging.ensure(nbytes, n, jpeg)
    table = staging.table.numpy()[:n]
    table[:] = np.asarray(rows, dtype=np.int64)
    check_frame_table(table, nbytes, channels)
    if boxes is not None:
        staging.boxes.numpy()[:n] = np.asarray(boxes, dtype=np.float64).reshape(n, 4).astype(np.float32)
    return staging, rows, nbytes


def pack_frames(images, cropboxes, resize_to=RESIZE_TO, crop=CROP, margin=2, pack="rect", staging=None, pad=0, grow=True):
    """uint8 images [H_i,W_i,C] and their crop boxes -> PackedFrames: the pixels ntk_frames_crop_batch may read, packed one frame
    after another behind `pad` leading bytes, with the int64 frame table and the fp32 boxes.  pack="rect" packs only
    crop_source_rect of each frame, pack="full" all of it (same crops, bit for bit; more bytes).  `staging`: the Staging set to
    fill (made when None); it grows when the batch needs more -- unless grow=False, when a batch that does not fit is packed
    into a fresh unpinned set instead (a thread that must make no device-runtime call packs this way).  Every table row is
    validated (check_frame_table)."""
    _check_pack(pack)
    n = len(images)
    if n < 1 or len(cropboxes) != n:
        raise ValueError("pack_frames: %d images, %d crop boxes" % (n, len(cropboxes)))
    C = int(images[0].shape[2])
    for img in images:
        if img.dtype != np.uint8 or img.ndim != 3 or img.shape[2] != C:
            raise ValueError("pack_frames: images must be uint8 [H,W,%d], not %s %s" % (C, img.dtype, img.shape))
    sizes = [img.shape[:2] for img in images]
    rects = [crop_source_rect(s, box, resize_to, crop, margin) if pack == "rect" else (0, 0) + tuple(s)
             for s, box in zip(sizes, cropboxes)]
    staging, rows, nbytes = _place(sizes, rects, C, cropboxes, staging, grow, pad=pad)
    buf = staging.pixels.numpy()
    buf[:pad] = 0
    for img, (o, _H, _W, y0, x0, h, w) in zip(images, rows):
        buf[o:o + h * w * C].reshape(h, w, C)[...] = img[y0:y0 + h, x0:x0 + w]
    return PackedFrames(staging, nbytes, n, C, resize_to, crop)


_MEANS = {}


def _vgg_mean(dev):
    key = (dev.type, dev.index if dev.index is not None else torch.cuda.current_device())
    if key not in _MEANS:
        _MEANS[key] = torch.tensor(VGG_MEAN, device=dev)
    return _MEANS[key]


def frames_crop_batch(packed, device="cuda", mean=None, flip_x=False, extrapolation=0.0, out=None):
    """Upload a PackedFrames (pixels, table, boxes: one asynchronous copy each when the staging is pinned) and crop it on the
    current stream: -> fp32 [n,crop_h,crop_w,C] on the device; ONE ntk_frames_crop_batch launch per 65 535 frames."""
    L, P = _lib.lib(), _lib.ptr
    dev = torch.device(device)
    n, C, (ch, cw) = packed.n, packed.channels, packed.crop
    if packed.jpeg is not None:
        pix, table, packed.status = decode_packed(packed, dev)
    else:
        pix = packed.pixels.to(dev, non_blocking=True)
        table = packed.table.to(dev, non_blocking=True)
    boxes = packed.boxes.to(dev, non_blocking=True)
    if out is None:
        out = torch.empty((n, ch, cw, C), device=dev)
    elif tuple(out.shape) != (n, ch, cw, C) or out.dtype != torch.float32:
        raise _lib.NtkError("frames_crop_batch: out must be fp32 %s, not %s %s" % ((n, ch, cw, C), out.dtype, tuple(out.shape)))
    for s in range(0, n, MAX_FRAMES_PER_LAUNCH):
        e = min(n, s + MAX_FRAMES_PER_LAUNCH)
        _lib.check(L.ntk_frames_crop_batch(P(pix), packed.nbytes, P(table[s:e]), P(boxes[s:e]), P(mean), P(out[s:e]), e - s, C,
                                           packed.resize_to[0], packed.resize_to[1], ch, cw, 1 if flip_x else 0,
                                           float(extrapolation), _lib.stream()), "ntk_frames_crop_batch")
    return out


def _load_frame(name, image_root, decode="host"):
    """-> (the frame's record, its image): decoded by Pillow (uint8 [H,W,3]), or with decode="device" probed (_probe_frame)."""
    rec = load_frame_record(name)
    path = rec["image_path"] if image_root is None else os.path.join(image_root, rec["image_path"])
    if decode == "host":
        return rec, _decode_image(path, np.uint8)
    with open(path, "rb") as f:
        return rec, _probe_frame(f.read(), path)


class StagedBatch(object):
    """A batch on the host, ready for upload_staged: the packed frames and, in the same Staging set, the labels."""

    def __init__(self, names, packed):
        self.names, self.packed = names, packed
        self.labels = packed.staging.labels[:packed.n]
        self.uploaded = None            # event after the uploads (set by upload_staged on a device)
        self.status = None              # decode="device": int32 [n] on the device after upload_staged, one NTK_JPEG_STATUS_* per frame

    def check_status(self):
        """decode="device": read the decoder's status from the device (this SYNCHRONISES with the stream that decoded) and raise
        NtkError naming the first frame's file whose status is not zero.  Nothing to do for a host-decoded batch."""
        if self.status is None:
            return
        status = self.status.cpu().numpy()
        bad = np.nonzero(status)[0]
        if bad.size:
            i = int(bad[0])
            raise _lib.NtkError("device JPEG decode of %s (frame %d of the batch) failed: %s (status %d)"
                                % (self.packed.jpeg.paths[i], i, JPEG_STATUS.get(int(status[i]), "unknown"), int(status[i])))


def stage_batch(frame_names_nosuffix, image_root=None, pool=None, pack="rect", staging=None, grow=True, decode="host"):
    """Host half of get_input_batch: read and decode the records and images (on `pool`'s threads when given), pack them.
    No device-runtime call is made when grow=False.  decode="device": a baseline JPEG is not decoded here -- its headers are parsed
    and its scan is copied, unstuffed, into the staging set (ntk_jpeg_parse; ctypes releases the GIL), for ntk_jpeg_decode_batch to
    decode in upload_staged; any other file (PNG, progressive JPEG, ...) is decoded by Pillow as with decode="host" and its
    rectangle packed into the same set."""
    _check_decode(decode)
    _check_pack(pack)
    names = list(frame_names_nosuffix)
    load = lambda nm: _load_frame(nm, image_root, decode)
    loaded = list(pool.map(load, names)) if pool is not None else [load(nm) for nm in names]
    images, boxes = [img for _r, img in loaded], [r["cropbox"] for r, _i in loaded]
    if decode == "host":
        packed = pack_frames(images, boxes, pack=pack, staging=staging, grow=grow)
    else:
        rects = [crop_source_rect(pr["size"], box) if pack == "rect" else (0, 0) + tuple(pr["size"]) for pr, box in zip(images, boxes)]
        packed = pack_jpeg_frames(images, rects, boxes, staging=staging, grow=grow, pool=pool)
    lab = packed.staging.labels.numpy()[:len(names)]
    for i, (rec, _img) in enumerate(loaded):
        lab[i, :64] = rec["gt"].reshape(-1)
        lab[i, 64], lab[i, 65] = rec["y_offset"], rec["x_offset"]
    return StagedBatch(names, packed)


# ---------------------------------------------------------------------------------------------------------------------------
# Validation from files: the files of ONE round of evaluate.Validation, staged as one set whose pixel buffer IS the round's
# [T,B,H,W,3] block with the starting frames of the slots reset in the round behind it.
# ---------------------------------------------------------------------------------------------------------------------------

RoundFiles = collections.namedtuple("RoundFiles", ["size", "T", "B", "cells", "starts"])
RoundFiles.__doc__ = """The files of one round: size (H, W) of the clips' frames; cells a list of (t, b, file) for the active cells
that have a file; starts a list of (slot, file), the starting frames of the slots reset in the round, in reset order.  A file is a
path or the file's bytes."""


class StagedRound(object):
    """stage_round's result.  `packed`: the PackedFrames (full-frame rectangles; with decode="host" every frame is in its host
    ranges).  `cell_index` int32 [T,B]: the row of cell (t, b) in the set, -1 where the round has no file for it; `start_index`
    int32 [B]: the row of the slot's starting frame, -1 for a slot that is not reset; `names` the files' names, by row.  Rows
    are the cells in (t, b) order, then the starting frames."""

    def __init__(self, packed, spec, cell_index, start_index, names):
        self.packed, self.spec, self.cell_index, self.start_index, self.names = packed, spec, cell_index, start_index, names
        self.uploaded = None            # event after the uploads (set by the consumer on a device)

    def host_frames(self):
        """-> (frames uint8 [T,B,H,W,3], starting frames uint8 [n_resets,H,W,3]): views of the pinned pixel buffer.  Whole only
        with decode="host"; cells without a file are zero."""
        (H, W), T, B, n = self.spec.size, self.spec.T, self.spec.B, len(self.spec.starts)
        block = T * B * H * W * 3
        buf = self.packed.staging.pixels.numpy()
        return buf[:block].reshape(T, B, H, W, 3), buf[block:block + n * H * W * 3].reshape(n, H, W, 3)


def _file_name(f, row):
    return "<%d bytes, file %d of the round>" % (len(f), row) if isinstance(f, (bytes, bytearray, memoryview)) else str(f)


def stage_round(spec, staging=None, pool=None, grow=True, decode="device"):
    """Host half of one validation round from files (``spec``: a RoundFiles) -> StagedRound.  Only the round's files are read, on
    `pool`'s threads when given.  decode="device": a baseline JPEG is parsed and its scan copied, unstuffed, into the set
    (ntk_jpeg_parse) for ntk_jpeg_decode_batch; any other file (PNG, progressive JPEG, ...) is decoded by Pillow into the same
    set, as in stage_batch.  decode="host": Pillow decodes every file.  The frame table's offsets put cell (t, b) at byte
    (t * B + b) * H * W * 3 and the k-th starting frame at (T * B + k) * H * W * 3, so the pixel buffer holds the round's
    [T,B,H,W,3] block and [n_resets,H,W,3] behind it without a further copy.  A file whose size is not the clip's is a ValueError
    naming it, as are more than MAX_FRAMES_PER_LAUNCH files.  No device-runtime call is made when grow=False.  Usable as
    InputPrefetcher's ``stage`` (with `batches` an iterable of RoundFiles)."""
    _check_decode(decode)
    (H, W), T, B = spec.size, int(spec.T), int(spec.B)
    files = [f for _t, _b, f in spec.cells] + [f for _s, f in spec.starts]
    n = len(files)
    if n < 1 or n > MAX_FRAMES_PER_LAUNCH:
        raise ValueError("stage_round: %d files in one round; 1..%d (MAX_FRAMES_PER_LAUNCH) can be staged" % (n, MAX_FRAMES_PER_LAUNCH))
    names = [_file_name(f, i) for i, f in enumerate(files)]

    def load(i):
        data, _what = _read_bytes(files[i])
        try:
            return _probe_frame(data, names[i], decode)
        except _lib.NtkError:
            raise
        except Exception as e:          # Pillow's errors do not name the file
            raise ValueError("%s: %s" % (names[i], e))

    probed = list(pool.map(load, range(n))) if pool is not None else [load(i) for i in range(n)]
    for pr in probed:
        if tuple(pr["size"]) != (H, W):
            raise ValueError("%s: the file is %dx%d (height x width) but its clip's frames are %dx%d"
                             % (pr["what"], pr["size"][0], pr["size"][1], H, W))
    frame = H * W * 3
    cell_index, start_index = np.full((T, B), -1, dtype=np.int32), np.full((B,), -1, dtype=np.int32)
    offsets = []
    for i, (t, b, _f) in enumerate(spec.cells):
        if not (0 <= t < T and 0 <= b < B) or cell_index[t, b] >= 0:
            raise ValueError("stage_round: cell (%d, %d) outside [%d,%d] or named twice" % (t, b, T, B))
        cell_index[t, b] = i
        offsets.append((t * B + b) * frame)
    for k, (slot, _f) in enumerate(spec.starts):
        if not 0 <= slot < B or start_index[slot] >= 0:
            raise ValueError("stage_round: slot %d outside [0,%d) or reset twice" % (slot, B))
        start_index[slot] = len(spec.cells) + k
        offsets.append((T * B + k) * frame)
    total = (T * B + len(spec.starts)) * frame
    packed = pack_jpeg_frames(probed, [(0, 0, H, W)] * n, staging=staging, grow=grow, pool=pool, offsets=(offsets, total))
    if decode == "host":                # the block goes to the tracker as it is: cells without a file are zero frames
        block = packed.staging.pixels.numpy()[:T * B * frame].reshape(T * B, frame)
        block[(cell_index < 0).reshape(-1)] = 0
    return StagedRound(packed, spec, cell_index, start_index, names)


def upload_staged(staged, device="cuda", reverse_image=False):
    """Device half of get_input_batch, on the current stream: -> get_input's four tensors."""
    dev = torch.device(device)
    batch_img = frames_crop_batch(staged.packed, dev, mean=_vgg_mean(dev), flip_x=reverse_image)
    staged.status = staged.packed.status
    lab = staged.labels.to(dev, non_blocking=True)
    if dev.type == "cuda":
        staged.uploaded = torch.cuda.Event()
        staged.uploaded.record()
    batch_gt = lab[:, :64].reshape(-1, 8, 8).contiguous()
    y_off, x_off = lab[:, 64].contiguous(), lab[:, 65].contiguous()
    if reverse_image:                                   # :187-188; the image itself is flipped by the kernel
        x_off = -x_off
    return batch_img, batch_gt, y_off, x_off


def get_input_batch(frame_names_nosuffix, device="cuda", reverse_image=False, image_root=None, workers=None, pack="rect",
                    staging=None, decode="host"):
    """get_input's contract -- (batch_img [n,224,224,3], batch_gt [n,8,8], y_offsets [n], x_offsets [n]), x_offsets negated and
    the crops flipped when reverse_image is set -- and its bits, in one launch: the records and images are read and decoded by
    `workers` threads (default_workers() when None; threads, not processes, and they make no device-runtime call), the uint8
    pixels each crop can touch are packed into pinned memory (`staging`, reused by the caller across batches), and after three
    asynchronous uploads ntk_frames_crop_batch resizes, subtracts the mean, crops and flips on the current stream.  A caller
    that reuses `staging` must not call again before the previous call's uploads have run (synchronise the stream, or use
    InputPrefetcher, which alternates two sets).  decode="device": baseline JPEG files are decoded by ntk_jpeg_decode_batch on the
    current stream instead of by the threads (same bits; stage_batch); the decoder's status is read before returning -- one
    synchronisation -- and a frame it could not decode raises NtkError naming the file."""
    from concurrent.futures import ThreadPoolExecutor
    workers = default_workers() if workers is None else int(workers)
    if workers > 1 and len(frame_names_nosuffix) > 1:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            staged = stage_batch(frame_names_nosuffix, image_root, pool, pack, staging, decode=decode)
    else:
        staged = stage_batch(frame_names_nosuffix, image_root, None, pack, staging, decode=decode)
    result = upload_staged(staged, device, reverse_image)
    staged.check_status()
    return result


class InputPrefetcher(object):
    """Iterator over `batches` (an iterable of lists of frame names, consumed lazily) that yields each as a StagedBatch, in order, while a background thread
    already stages the next one: batch i+1 is read, decoded (by `workers` pool threads) and packed into the other of `depth`
    Staging sets while the caller trains on batch i.  The background threads make no device-runtime call: uploads and the
    launch (upload_staged) stay on the consumer's thread, and a batch that outgrows its pinned set is packed unpinned and
    moved into a grown pinned set by the consumer.  A set is handed back to the background thread when the consumer asks for the
    next batch, after the uploads from it have run.  An exception while staging batch i is re-raised by the __next__ that
    would have returned batch i.  close() stops and joins the threads; it is also called by __del__ and on leaving a
    ``with`` block.  `stage`: the staging function, stage(names, staging) -> StagedBatch (default: stage_batch)."""

    def __init__(self, batches, depth=2, image_root=None, workers=None, pack="rect", stage=None, decode="host"):
        import queue
        import threading
        from concurrent.futures import ThreadPoolExecutor
        if depth < 1:
            raise ValueError("depth must be at least 1, not %d" % depth)
        _check_decode(decode)
        self._batches = batches         # any iterable of name lists, consumed as the run goes (a generator: nothing is built ahead)
        self._sets = [Staging() for _ in range(depth)]
        self._free, self._ready = queue.Queue(), queue.Queue()
        for k in range(depth):
            self._free.put(k)
        self._held = None               # (set index, StagedBatch) the consumer is using
        self._next, self._closed, self._done = 0, False, False
        self._stop = threading.Event()
        workers = default_workers() if workers is None else int(workers)
        self._pool = ThreadPoolExecutor(max_workers=workers) if workers > 1 else None
        if stage is None:
            stage = lambda names, staging: stage_batch(names, image_root, self._pool, pack, staging, grow=False, decode=decode)
        self._stage = stage
        self._thread = threading.Thread(target=self._produce, name="ntmtrack-input-prefetch", daemon=True)
        self._thread.start()

    _END = object()                     # after the last batch

    def _produce(self):
        import queue
        source, i = iter(self._batches), 0
        while True:
            k = None
            while k is None:
                if self._stop.is_set():
                    return
                try:
                    k = self._free.get(timeout=0.05)
                except queue.Empty:
                    pass
            try:
                names = next(source)
            except StopIteration:
                self._ready.put((i, k, None, self._END))
                return
            except BaseException as e:          # noqa: B902 -- the source of batches itself failed: nothing can follow
                self._ready.put((i, k, None, e))
                self._ready.put((i + 1, None, None, self._END))
                return
            try:
                item = (i, k, self._stage(names, self._sets[k]), None)
            except BaseException as e:          # noqa: B902 -- handed to the consumer, which re-raises it at this batch
                item = (i, k, None, e)
            self._ready.put(item)
            i += 1

    def _release(self):
        if self._held is not None:
            k, staged = self._held
            if staged is not None and getattr(staged, "uploaded", None) is not None:
                staged.uploaded.synchronize()
            self._held = None
            self._free.put(k)

    def __iter__(self):
        return self

    def __len__(self):
        return len(self._batches)       # TypeError for a generator, as for any iterator without a length

    def __next__(self):
        import queue
        if self._closed or self._done:
            raise StopIteration
        self._release()
        while True:
            try:
                i, k, staged, err = self._ready.get(timeout=0.05)
                break
            except queue.Empty:
                if not self._thread.is_alive() and self._ready.empty():
                    raise RuntimeError("InputPrefetcher: the staging thread ended before batch %d" % self._next)
        if err is self._END:
            self._done = True
            raise StopIteration
        assert i == self._next
        self._next += 1
        self._held = (k, staged)
        if err is not None:
            raise err
        packed = getattr(staged, "packed", None)
        if packed is not None and packed.staging is not self._sets[k]:
            # the batch outgrew set k: grow the pinned set here, on the consumer's thread, and move the batch into it
            staged.packed = self._sets[k].adopt(packed)
            staged.labels = self._sets[k].labels[:packed.n]
        return staged

    def close(self):
        if getattr(self, "_closed", True):
            return
        self._closed = True
        self._stop.set()
        self._thread.join()
        if self._pool is not None:
            self._pool.shutdown(wait=True)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


# ---------------------------------------------------------------------------------------------------------------------------
# decode="device": baseline JPEG decoded by HIP kernels into the pixel buffer ntk_frames_crop_batch reads (csrc/jpeg_decode.hip).
# The host parses the headers and removes the byte stuffing (ntk_jpeg_parse); everything else runs on the device, in libjpeg's
# default integer arithmetic: the bytes are Pillow's.
# ---------------------------------------------------------------------------------------------------------------------------

DECODE_MODES = ("host", "device")
JPEG_HOST_PATH = 1              # NTK_JPEG_HOST_PATH: the file is not for the device decoder (not an error)
JPEG_MIN_SIDE = 16
JPEG_DESC_BYTES = 7936
JPEG_DESC_HDR_WORDS = 32
JPEG_DESC = {"H": 0, "W": 1, "NCOMP": 2, "HS": 3, "VS": 4, "RESTART": 5, "MCUS_X": 6, "MCUS_Y": 7, "NSEG": 8, "SEG_FIRST": 9,
             "STREAM_OFF": 10, "WS_OFF": 12, "STREAM_BYTES": 14, "TQ": 16, "TD": 19, "TA": 22}     # NTK_JPEG_DESC_*
JPEG_WS_BYTES_PER_BLOCK = 192
JPEG_STATUS = {0: "ok", 1: "a bit pattern that no Huffman code matches", 2: "the scan ends before the image does",
               3: "the workspace is too small", 4: "a descriptor or frame table row outside the buffers",
               5: "fewer restart segments than the image needs"}                                # NTK_JPEG_STATUS_*


def _check_decode(decode):
    if decode not in DECODE_MODES:
        raise ValueError("decode must be 'host' or 'device', not %r" % (decode,))


def _np_ptr(a, byte_offset=0):
    import ctypes
    return ctypes.c_void_p(a.ctypes.data + byte_offset)


def _jpeg_parse_raw(data, desc, dst, dst_offset, dst_cap, seg, seg_offset, seg_cap, what):
    """ntk_jpeg_parse on the bytes `data`: desc uint8 [JPEG_DESC_BYTES] (NumPy), dst uint8 / seg int32 NumPy arrays or None.
    -> (rc, stream_bytes, n_segments); a malformed file raises NtkError naming `what`."""
    import ctypes
    sbytes, nseg = ctypes.c_longlong(0), ctypes.c_int(0)
    rc = _lib.lib().ntk_jpeg_parse(data, len(data), _np_ptr(desc), None if dst is None else _np_ptr(dst, dst_offset), dst_cap,
                                   None if seg is None else _np_ptr(seg, 4 * seg_offset), seg_cap, ctypes.byref(sbytes),
                                   ctypes.byref(nseg))
    if rc < 0:
        msg = _lib.lib().ntk_last_error()
        raise _lib.NtkError("%s: %s (%d)" % (what, msg.decode() if msg else "", rc))
    return rc, sbytes.value, nseg.value


class ParsedJpeg(object):
    """parse_jpeg's result: the descriptor (uint8 [JPEG_DESC_BYTES]; `hdr` its int32 header words, JPEG_DESC names them), the
    unstuffed scan (`stream`, uint8) and the restart-segment offsets into it (`segments`, int32 [n_segments + 1])."""

    def __init__(self, desc, stream, segments):
        self.desc, self.stream, self.segments = desc, stream, segments
        self.hdr = desc[:4 * JPEG_DESC_HDR_WORDS].view(np.int32)
        h = self.hdr
        self.height, self.width, self.components = int(h[JPEG_DESC["H"]]), int(h[JPEG_DESC["W"]]), int(h[JPEG_DESC["NCOMP"]])
        self.sampling = (int(h[JPEG_DESC["HS"]]), int(h[JPEG_DESC["VS"]]))
        self.restart_interval = int(h[JPEG_DESC["RESTART"]])
        self.mcus = (int(h[JPEG_DESC["MCUS_Y"]]), int(h[JPEG_DESC["MCUS_X"]]))
        self.n_segments, self.stream_bytes = int(h[JPEG_DESC["NSEG"]]), int(h[JPEG_DESC["STREAM_BYTES"]])


def _read_bytes(bytes_or_path):
    if isinstance(bytes_or_path, (bytes, bytearray, memoryview)):
        return bytes(bytes_or_path), "<%d bytes>" % len(bytes_or_path)
    with open(bytes_or_path, "rb") as f:
        return f.read(), str(bytes_or_path)


def parse_jpeg(bytes_or_path, dst=None):
    """Parse one file for the device decoder (ntk_jpeg_parse; pure host code) -> ParsedJpeg, or None for a file that is not for
    the device (not a JPEG, progressive, 12 bit, CMYK, ...: the host path).  A malformed JPEG raises NtkError.  `dst`: a uint8
    NumPy array to receive the unstuffed scan (at least the file's length always suffices); made when None."""
    data, what = _read_bytes(bytes_or_path)
    desc = np.zeros(JPEG_DESC_BYTES, np.uint8)
    rc, sbytes, nseg = _jpeg_parse_raw(data, desc, None, 0, 0, None, 0, 0, what)
    if rc == JPEG_HOST_PATH:
        return None
    if dst is None:
        dst = np.empty(max(sbytes, 1), np.uint8)
    elif dst.dtype != np.uint8 or dst.ndim != 1 or not dst.flags.c_contiguous or dst.size < sbytes:
        raise ValueError("parse_jpeg: dst must be a contiguous uint8 vector of at least %d bytes" % sbytes)
    seg = np.zeros(nseg + 1, np.int32)
    _jpeg_parse_raw(data, desc, dst, 0, dst.size, seg, 0, nseg + 1, what)
    return ParsedJpeg(desc, dst[:sbytes], seg)


class JpegPart(object):
    """What a PackedFrames holds for the device decoder: sizes of the filled parts of the staging set's streams / segments, the
    workspace the batch needs, which frames the device decodes, the byte ranges of `pixels` the host filled, and the files."""

    def __init__(self, stream_bytes, n_segments, workspace_bytes, on_device, host_ranges, paths):
        self.stream_bytes, self.n_segments, self.workspace_bytes = stream_bytes, n_segments, workspace_bytes
        self.on_device, self.host_ranges, self.paths = on_device, host_ranges, paths


def _probe_frame(data, what, decode="device"):
    """File bytes -> dict: for a device frame `data`, the frame's size and the sizes of its stream and segment table; for any
    other file, and for every file with decode="host", `image`, decoded by Pillow (uint8 [H,W,3])."""
    if decode == "device":
        desc = np.zeros(JPEG_DESC_BYTES, np.uint8)
        rc, sbytes, nseg = _jpeg_parse_raw(data, desc, None, 0, 0, None, 0, 0, what)
        if rc != JPEG_HOST_PATH:
            hdr = desc[:4 * JPEG_DESC_HDR_WORDS].view(np.int32)
            return {"data": data, "image": None, "size": (int(hdr[JPEG_DESC["H"]]), int(hdr[JPEG_DESC["W"]])),
                    "stream_bytes": sbytes, "n_segments": nseg, "what": what}
    img = _decode_image(data, np.uint8)
    return {"data": None, "image": img, "size": img.shape[:2], "what": what}


def pack_jpeg_frames(probed, rects, boxes=None, resize_to=RESIZE_TO, crop=CROP, staging=None, grow=True, pool=None, offsets=None):
    """_probe_frame results and one rectangle (y0, x0, h, w) per frame -> PackedFrames whose `jpeg` part is filled: the frame
    table and boxes as pack_frames writes them; per device frame its descriptor, unstuffed scan and segment offsets in the staging
    set (written by ntk_jpeg_parse on `pool`'s threads: the one copy the file's bytes get); per other frame its rectangle's
    pixels.  The workspace is sized and each frame's share of it written into its descriptor (ntk_jpeg_decode_workspace_bytes).
    Staging rules as in pack_frames (`grow`).  `offsets`: (byte offset of each frame's rectangle in the pixel buffer, the buffer's
    size in bytes) -- the caller's own layout, checked like every table row; None packs the rectangles back to back."""
    import ctypes
    n = len(probed)
    if n < 1 or n > MAX_FRAMES_PER_LAUNCH or len(rects) != n:
        raise ValueError("pack_jpeg_frames: %d frames (1..%d), %d rectangles" % (n, MAX_FRAMES_PER_LAUNCH, len(rects)))
    if offsets is not None and len(offsets[0]) != n:
        raise ValueError("pack_jpeg_frames: %d offsets for %d frames" % (len(offsets[0]), n))
    soff, goff, place = 0, 0, []
    for pr in probed:
        place.append((soff, goff))
        if pr["data"] is not None:
            soff += (len(pr["data"]) + 15) // 16 * 16           # the unstuffed scan is shorter than the file
            goff += pr["n_segments"] + 1
    sbytes, nsegs = max(soff, 16), max(goff, 2)
    staging, rows, nbytes = _place([pr["size"] for pr in probed], rects, 3, boxes, staging, grow, offsets=offsets, jpeg=(sbytes, nsegs))
    table = staging.table.numpy()[:n]
    buf, streams, descs, segs = staging.pixels.numpy(), staging.streams.numpy(), staging.descs.numpy(), staging.segments.numpy()

    def fill(i):
        pr, (o, _H, _W, y0, x0, h, w), (so, go) = probed[i], rows[i], place[i]
        if pr["data"] is None:
            descs[i, :4 * JPEG_DESC_HDR_WORDS] = 0              # NCOMP = 0: the device skips the frame
            buf[o:o + h * w * 3].reshape(h, w, 3)[...] = pr["image"][y0:y0 + h, x0:x0 + w]
            return
        _jpeg_parse_raw(pr["data"], descs[i], streams, so, len(pr["data"]), segs, go, pr["n_segments"] + 1, pr["what"])
        hdr = descs[i, :4 * JPEG_DESC_HDR_WORDS].view(np.int32)
        hdr[JPEG_DESC["SEG_FIRST"]] = go
        hdr[JPEG_DESC["STREAM_OFF"]:JPEG_DESC["STREAM_OFF"] + 2].view(np.int64)[0] = so

    list(pool.map(fill, range(n)) if pool is not None else map(fill, range(n)))
    ws = ctypes.c_longlong(0)
    _lib.check(_lib.lib().ntk_jpeg_decode_workspace_bytes(_np_ptr(descs), _np_ptr(table), n, ctypes.byref(ws)),
               "ntk_jpeg_decode_workspace_bytes")
    packed = PackedFrames(staging, nbytes, n, 3, resize_to, crop)
    on_device = [pr["data"] is not None for pr in probed]
    packed.jpeg = JpegPart(sbytes, nsegs, ws.value, on_device,
                           [(r[0], r[0] + r[5] * r[6] * 3) for r, d in zip(rows, on_device) if not d], [pr["what"] for pr in probed])
    return packed


def decode_packed(packed, device, uploaded=None):
    """Device half of the JPEG path, on the current stream: upload the streams, descriptors, segment offsets and frame table of a
    PackedFrames with a `jpeg` part, and the pixel ranges the host decoded, into the staging set's device buffers (grown and
    reused: no allocator call in the steady state but the status vector's), then ONE ntk_jpeg_decode_batch call.  `uploaded`: an
    event recorded behind the uploads and before the launch (what the owner of the pinned set waits for before refilling it).
    -> (pixels uint8 [nbytes], frame table int64 [n,7], status int32 [n]), all on the device."""
    L, P = _lib.lib(), _lib.ptr
    dev = torch.device(device)
    st, j, n = packed.staging, packed.jpeg, packed.n
    pix = st.device_buffer(dev, "pixels", packed.nbytes, torch.uint8)
    for o, e in j.host_ranges:
        pix[o:e].copy_(st.pixels[o:e], non_blocking=True)
    table = st.device_buffer(dev, "table", n * FRAME_TABLE_COLS, torch.int64).view(n, FRAME_TABLE_COLS)
    table.copy_(packed.table, non_blocking=True)
    status = torch.zeros((n,), dtype=torch.int32, device=dev)   # outlives the staging set's reuse: read at a logged step
    if not any(j.on_device):
        if uploaded is not None:
            uploaded.record()
        return pix, table, status
    streams = st.device_buffer(dev, "streams", j.stream_bytes, torch.uint8)
    streams.copy_(st.streams[:j.stream_bytes], non_blocking=True)
    descs = st.device_buffer(dev, "descs", n * JPEG_DESC_BYTES, torch.uint8)
    descs.copy_(st.descs[:n].view(-1), non_blocking=True)
    segs = st.device_buffer(dev, "segments", j.n_segments, torch.int32)
    segs.copy_(st.segments[:j.n_segments], non_blocking=True)
    ws = st.device_buffer(dev, "workspace", j.workspace_bytes, torch.uint8)
    if uploaded is not None:
        uploaded.record()
    _lib.check(L.ntk_jpeg_decode_batch(P(streams), j.stream_bytes, P(descs), P(segs), j.n_segments, P(table), P(pix), packed.nbytes,
                                       P(ws), j.workspace_bytes, P(status), n, _lib.stream()), "ntk_jpeg_decode_batch")
    return pix, table, status


class DecodedJpegs(object):
    """decode_jpeg_batch's result: `pixels` uint8 on the device, the frames' rectangles packed one after another as h*w*3 RGB
    bytes; `table` the int64 [n,7] frame table (NumPy; `table_device` the same on the device: what ntk_frames_crop_batch takes);
    `status` int32 [n] on the device (0: decoded; JPEG_STATUS names the others); `on_device[i]`: the device decoded frame i
    (False: Pillow did -- not a baseline JPEG the device takes).  image(i) -> frame i's rectangle as uint8 [h,w,3] (NumPy)."""

    def __init__(self, packed, pixels, table_device, status):
        self.packed, self.pixels, self.table_device, self.status = packed, pixels, table_device, status
        self.table = packed.table.numpy().copy()
        self.on_device = list(packed.jpeg.on_device)

    def image(self, i):
        off, _H, _W, _y0, _x0, h, w = [int(v) for v in self.table[i]]
        return self.pixels[off:off + h * w * 3].cpu().numpy().reshape(h, w, 3)


def decode_jpeg_batch(streams, rects=None, device="cuda", staging=None):
    """Decode a batch of image files on the device, on the current stream: `streams` a list of file contents (bytes) or paths;
    `rects` one (y0, x0, h, w) per file, the part of the image wanted (None: all of it, for that file or for all).  Baseline JPEG
    files (8 bit, gray or YCbCr with 4:4:4 / 4:2:2 / 4:2:0 sampling, one interleaved scan, sides of 16 pixels or more) are decoded
    by ntk_jpeg_decode_batch to the bytes Pillow gives; any other file is decoded by Pillow here and uploaded.  Nothing is
    synchronised: read `status` (or call image()) after the stream has run.  -> DecodedJpegs."""
    probed = [_probe_frame(*_read_bytes(s)) for s in streams]
    if rects is None:
        rects = [None] * len(probed)
    rects = [(0, 0) + tuple(pr["size"]) if r is None else tuple(int(v) for v in r) for pr, r in zip(probed, rects)]
    packed = pack_jpeg_frames(probed, rects, staging=staging)
    pix, table, status = decode_packed(packed, device)
    return DecodedJpegs(packed, pix, table, status)
