"""Validation over clips on the device: the reference's validate_tracker.py:26-38 (one NTMTracker per clip, one frame at a time,
nothing scored) as continuous batching over B slots of a BatchNTMTracker / BatchDNCTracker, with the overlap scores of every clip
accumulated in one device table (ntk_track_overlap_scores) that is read back once, at the end.

  ClipSchedule   which clip sits in which slot in which round (host arithmetic only: no torch, no device)
  OverlapScores  the device table and its one synchronising read-out
  Supervisor     the supervised protocol (a lost tracker is restarted from the ground truth): per-slot state and per-clip table
                 on the device (ntk_track_supervise), decided frame by frame without a read-back
  Validation     the driver: per round the resets, ONE track_clip and ONE scores.add, no host synchronisation after the first
                 round of a frame size.  The frames of a round come from the frame size's source: _ArraySource (arrays and
                 callables), _HostFileSource (image files read a round at a time, a round ahead: data.stage_round,
                 data.InputPrefetcher) or _DeviceFileSource (the files decoded on the device on a second stream,
                 ntk_jpeg_decode_batch, ntk_track_decode_mask turning off the frames that could not be decoded)
  multistart_runs    the multi-start protocol's runs of a set of clips (host arithmetic only): a run is a clip whose frames are
                 read in another order
  MultiStart     the multi-start protocol's run table and overlap trace on the device (ntk_track_multistart) and the EAO
                 reduction (ntk_track_eao_curve)
  validate       runs a Validation to the end; protocol="one_pass" (the default), "supervised" or "multistart"
  write_trajectory   the toolkit's trajectory file of one clip, from regions() and codes()

The ground truth of a clip is a rectangle per frame ([L,4]) or a polygon per frame ([L,2P], 3 <= P <= 8: VOT regions), which is
scored as the toolkit scores it -- the polygon against the tracker's rectangle (ntk_track_overlap_scores_poly,
ntk_track_supervise_poly) -- while the tracker is started and restarted from the polygon's bounding rectangle, as the reference's
vot.VOT("rectangle") hands it over.  A run without a polygon clip makes exactly the rectangle calls.

Or it is a segmentation mask per frame (MaskRegions: the run-length coded masks of the VOT sets from 2020 on, include/ntmtrack.h
NTK_MASK_*), scored straight from the counts against the pixel set of the tracker's rectangle (ntk_track_mask_overlaps,
ntk_track_overlap_scores_mask, ntk_track_supervise_mask) while the tracker is started and restarted from the bounds of the set
pixels (ntk_track_mask_bounds).  A run holds either only mask clips or none.

The overlap is the VOT / OTB one on real-valued rectangles.  The reference's own bb_iou (test_tracker.py:59-83) is never called
there, uses a +1 pixel convention and does not clamp an empty intersection: it is not the model here.
"""
import collections

import numpy as np

# row layout of the score table: include/ntmtrack.h NTK_SCORE_*
SCORE_FRAMES, SCORE_SUM_IOU, SCORE_SUM_DIST, SCORE_LOST, SCORE_FIRST_LOST, SCORE_HEAD = 0, 1, 2, 3, 4, 5
SCORE_MAX_THRESHOLDS = 256

# include/ntmtrack.h NTK_SUP_*: the supervised protocol's table row, slot state, modes, phases and per-frame codes
SUP_VALID, SUP_SUM_IOU, SUP_FAILURES, SUP_RESTARTS, SUP_TRACKED, SUP_SKIPPED, SUP_FIRST_FAILURE, SUP_HEAD = 0, 1, 2, 3, 4, 5, 6, 7
SUP_STATE_MODE, SUP_STATE_COUNTDOWN, SUP_STATE_SINCE, SUP_STATE_INTS = 0, 1, 2, 3
SUP_MODE_TRACK, SUP_MODE_WAIT = 0, 1
SUP_PLAN, SUP_JUDGE = 0, 1
SUP_CODE_INACTIVE, SUP_CODE_TRACKED, SUP_CODE_RESTART, SUP_CODE_FAILURE, SUP_CODE_SKIPPED = -1, 0, 1, 2, 3
PROTOCOLS = ("one_pass", "supervised", "multistart")
# include/ntmtrack.h NTK_MS_*: the multi-start protocol's table row, one per run
MS_FRAMES, MS_TRACKED, MS_SUM_IOU, MS_FAILED, MS_LOW, MS_PENDING, MS_HEAD = 0, 1, 2, 3, 4, 5, 6
# include/ntmtrack.h NTK_POLY_*: a polygon region is POLY_DOUBLES doubles, the leading finite pairs its vertices, NaN after them
POLY_MAX_POINTS, POLY_DOUBLES = 8, 16
# include/ntmtrack.h NTK_CLIPDEC_*: the per-clip row of ntk_track_decode_mask (validation from files decoded on the device)
CLIPDEC_DECODED, CLIPDEC_FAILED, CLIPDEC_MASKED, CLIPDEC_FIRST_FAILED, CLIPDEC_FIRST_STATUS, CLIPDEC_START_STATUS, CLIPDEC_HEAD = \
    0, 1, 2, 3, 4, 5, 6
ON_UNDECODED = ("raise", "skip")
# include/ntmtrack.h NTK_MASK_*: a mask is (x0, y0, w, h, first, count) over a flat array of counts; its overlap (|M n R|, |R|, |M|)
MASK_CELL_INTS, MASK_OVERLAP_DOUBLES, MASK_MAX_PIXELS = 6, 3, 1 << 30

Round = collections.namedtuple("Round", ["resets", "frame_index", "active", "clip_of"])


def _upload(array, dtype, device):
    """online._upload (host array -> device tensor through a pinned asynchronous copy: no synchronisation), imported at its first
    use: this module stays importable without torch."""
    from .online import _upload as upload
    return upload(array, dtype, device)

#: one clip of a validation set.  frames: [L,H,W,3] uint8 or float host array, or a callable returning one (called when the clip is
#: scheduled), or a list / tuple of L image files (paths, or the files' bytes): a FILE CLIP, read a round at a time and never held
#: whole (size may then be None: it is read from the first file's header).  regions: [L,4] ground truth (x, y, w, h) in pixels, row 0 starts the tracker; or [L,2P] polygons (x0, y0, x1, y1,
#: ...) of 3 <= P <= 8 vertices, rows with fewer padded with NaN, the tracker then starts from row 0's bounding rectangle; or a
#: MaskRegions (a segmentation mask per frame), the tracker then starts from the bounds of frame 0's set pixels.  init:
#: the region the tracker is started with when it is not that (the reference passes it normalised).  size: (H, W) where frames is a callable, so that
#: clips can be grouped by frame size without decoding them.
Clip = collections.namedtuple("Clip", ["frames", "regions", "init", "size"])
Clip.__new__.__defaults__ = (None, None)


def pad_polygons(regions):
    """[..., 2P] polygons, 3 <= P <= POLY_MAX_POINTS -> [..., POLY_DOUBLES] float64, padded with NaN."""
    a = np.asarray(regions, dtype=np.float64)
    k = a.shape[-1] if a.ndim else 0
    if k % 2 or not 6 <= k <= POLY_DOUBLES:
        raise ValueError("polygon regions have %d columns; 2P with 3 <= P <= %d" % (k, POLY_MAX_POINTS))
    out = np.full(a.shape[:-1] + (POLY_DOUBLES,), np.nan)
    out[..., :k] = a
    return out


def rect_polygons(rects):
    """[..., 4] rectangles (x, y, w, h) -> [..., POLY_DOUBLES] 4-gons (x, y), (x + w, y), (x + w, y + h), (x, y + h); a rectangle that
    is not finite with w > 0 and h > 0 (an absent object) becomes a region of NaNs (an absent object)."""
    r = np.asarray(rects, dtype=np.float64)
    out = np.full(r.shape[:-1] + (POLY_DOUBLES,), np.nan)
    with np.errstate(invalid="ignore"):
        x, y, x2, y2 = r[..., 0], r[..., 1], r[..., 0] + r[..., 2], r[..., 1] + r[..., 3]
        ok = np.isfinite(r).all(axis=-1) & (r[..., 2] > 0) & (r[..., 3] > 0)
    for i, v in enumerate((x, y, x2, y, x2, y2, x, y2)):
        out[..., i] = np.where(ok, v, np.nan)
    return out


def polygon_bounds(polys):
    """The host's ntk_track_poly_bounds: [..., POLY_DOUBLES] -> [..., 4] (min x, min y, max x - min x, max y - min y) over the
    leading finite pairs, NaN for a region that is not present (fewer than 3 vertices, an empty bounding rectangle, or a shoelace
    area of 0)."""
    polys = np.asarray(polys, dtype=np.float64)
    flat = polys.reshape(-1, POLY_DOUBLES)
    out = np.full((len(flat), 4), np.nan)
    for i, g in enumerate(flat):
        pts = g.reshape(-1, 2)
        n = 0
        while n < POLY_MAX_POINTS and np.isfinite(pts[n]).all():
            n += 1
        if n < 3:
            continue
        x, y = pts[:n, 0], pts[:n, 1]
        w, h = x.max() - x.min(), y.max() - y.min()
        dx, dy = x - x[0], y - y[0]
        with np.errstate(all="ignore"):
            twice = sum(dx[j] * dy[(j + 1) % n] - dx[(j + 1) % n] * dy[j] for j in range(n))
        if w > 0 and h > 0 and abs(twice) / 2 > 0:
            out[i] = (x.min(), y.min(), w, h)
    return out.reshape(polys.shape[:-1] + (4,))


class MaskRegions(object):
    """The ground truth of one clip as run-length coded masks (include/ntmtrack.h NTK_MASK_*): ``boxes`` int32 [L,4], frame i's
    mask box (x0, y0, w, h) in frame pixels; ``counts`` int32, the counts of all frames one after the other, as the toolkit
    writes them (even-indexed counts of a frame are runs of zeros, odd-indexed ones runs of ones, row-major over the box);
    ``offsets`` int64 [L+1], frame i's counts are counts[offsets[i]:offsets[i+1]] -- so the frames of a slot in a round are one
    slice.  A frame whose mask is not PRESENT (an empty box, a negative count, no pixel set) is an absent object."""

    def __init__(self, boxes, counts, offsets):
        self.boxes = np.ascontiguousarray(boxes, dtype=np.int32).reshape(-1, 4)
        self.counts = np.ascontiguousarray(counts, dtype=np.int32).reshape(-1)
        self.offsets = np.ascontiguousarray(offsets, dtype=np.int64).reshape(-1)
        if (len(self.offsets) != len(self.boxes) + 1 or self.offsets[0] != 0 or self.offsets[-1] != len(self.counts)
                or (np.diff(self.offsets) < 0).any()):
            raise ValueError("MaskRegions: %d boxes, %d counts and offsets %s" % (len(self.boxes), len(self.counts), self.offsets.tolist()))

    def __len__(self):
        return len(self.boxes)

    @classmethod
    def from_lists(cls, frames):
        """frames: per frame (x0, y0, w, h, counts), or None for an absent object (an empty box without counts)."""
        boxes = [(0, 0, 0, 0) if f is None else tuple(f[:4]) for f in frames]
        counts = [np.zeros(0, dtype=np.int32) if f is None else np.asarray(f[4], dtype=np.int32).reshape(-1) for f in frames]
        offsets = np.concatenate([[0], np.cumsum([len(c) for c in counts])])
        return cls(np.asarray(boxes, dtype=np.int32).reshape(-1, 4), np.concatenate(counts) if counts else counts, offsets)

    @classmethod
    def from_arrays(cls, masks):
        """Dense masks [L,H,W] (nonzero = object) -> the masks coded over their tight boxes; an all-zero frame is an absent
        object."""
        masks = np.asarray(masks)
        if masks.ndim != 3:
            raise ValueError("MaskRegions.from_arrays: masks %s; expected [L,H,W]" % (masks.shape,))
        frames = []
        for m in masks != 0:
            rows, cols = np.nonzero(m.any(axis=1))[0], np.nonzero(m.any(axis=0))[0]
            if not len(rows):
                frames.append(None)
                continue
            x0, y0, x1, y1 = cols[0], rows[0], cols[-1] + 1, rows[-1] + 1
            flat = m[y0:y1, x0:x1].reshape(-1)
            edges = np.nonzero(flat[1:] != flat[:-1])[0] + 1              # where a run starts
            runs = np.diff(np.concatenate([[0], edges, [len(flat)]]))
            if flat[0]:
                runs = np.concatenate([[0], runs])                        # the mask begins with a one
            if len(runs) % 2:
                runs = runs[:-1]                                          # trailing zeros: pixels the counts do not reach
            frames.append((x0, y0, x1 - x0, y1 - y0, runs))
        return cls.from_lists(frames)

    def frame(self, i):
        """-> (x0, y0, w, h, counts) of frame i."""
        x0, y0, w, h = (int(v) for v in self.boxes[i])
        return x0, y0, w, h, self.counts[self.offsets[i]:self.offsets[i + 1]]

    def ones_runs(self, i):
        """The runs of ones of frame i clipped to its box -> (w, starts, ends) with ends > starts, or None where the mask is not
        present."""
        _x0, _y0, w, h, c = self.frame(i)
        if w <= 0 or h <= 0 or w * h > MASK_MAX_PIXELS or (c < 0).any():
            return None
        ends = np.cumsum(c.astype(np.int64))
        s, e = np.minimum((ends - c)[1::2], w * h), np.minimum(ends[1::2], w * h)
        keep = e > s
        return (w, s[keep], e[keep]) if keep.any() else None

    def dense(self, i, H, W):
        """Frame i decoded -> bool [H,W] (the part of the box inside the frame); all False for an absent object."""
        out = np.zeros((H, W), dtype=bool)
        runs = self.ones_runs(i)
        if runs is None:
            return out
        x0, y0, w, h, _c = self.frame(i)
        _w, s, e = runs
        d = np.zeros(w * h + 1, dtype=np.int64)
        np.add.at(d, s, 1)
        np.add.at(d, e, -1)
        box = (np.cumsum(d)[:w * h] > 0).reshape(h, w)
        ya, yb, xa, xb = max(y0, 0), min(y0 + h, H), max(x0, 0), min(x0 + w, W)
        if yb > ya and xb > xa:
            out[ya:yb, xa:xb] = box[ya - y0:yb - y0, xa - x0:xb - x0]
        return out

    def take(self, indices):
        """-> MaskRegions of the frames ``indices``, in that order: the boxes re-ordered, the counts re-concatenated, the offsets
        rebuilt."""
        idx = np.asarray(indices, dtype=np.int64).reshape(-1)
        if len(idx) and (idx.min() < 0 or idx.max() >= len(self)):
            raise ValueError("MaskRegions.take: indices outside [0,%d)" % len(self))
        sizes = self.offsets[idx + 1] - self.offsets[idx]
        offsets = np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)
        # element k of the new counts: its frame j = the last one whose offset is <= k, the same place inside the old frame
        j = np.repeat(np.arange(len(idx)), sizes)
        counts = self.counts[self.offsets[idx][j] + (np.arange(offsets[-1]) - offsets[j])]
        return MaskRegions(self.boxes[idx], counts, offsets)

    def cells(self, lo, hi):
        """Frames [lo, hi) in the device layout -> (cells int32 [hi-lo, MASK_CELL_INTS] whose ``first`` counts from the start of
        the returned counts, the counts of those frames: one slice)."""
        a, b = int(self.offsets[lo]), int(self.offsets[hi])
        cells = np.empty((hi - lo, MASK_CELL_INTS), dtype=np.int32)
        cells[:, :4] = self.boxes[lo:hi]
        cells[:, 4] = self.offsets[lo:hi] - a
        cells[:, 5] = np.diff(self.offsets[lo:hi + 1])
        return cells, self.counts[a:b]


def mask_bounds(regions, i=None):
    """The host's ntk_track_mask_bounds: MaskRegions -> float64 [L,4] (or [4] of frame i): (min col, min row, max col + 1 - min col,
    max row + 1 - min row) over the set pixels in frame pixels, NaN for a mask that is not present.  What a clip's tracker starts
    from."""
    if i is not None:
        out = np.full(4, np.nan)
        runs = regions.ones_runs(i)
        if runs is not None:
            w, s, e = runs
            r0, r1 = s // w, (e - 1) // w
            one_row = bool((r0 == r1).all())                                # else a run crosses a row end: every column
            c_min, c_max = (int((s % w).min()), int(((e - 1) % w).max())) if one_row else (0, w - 1)
            out[:] = (int(regions.boxes[i, 0]) + c_min, int(regions.boxes[i, 1]) + int(r0.min()), c_max + 1 - c_min,
                      int(r1.max()) + 1 - int(r0.min()))
        return out
    return np.stack([mask_bounds(regions, k) for k in range(len(regions))]) if len(regions) else np.zeros((0, 4))


class MaskRound(object):
    """The mask ground truth of a round (or of one of its frames) on the device: ``cells`` int32 [T,B,MASK_CELL_INTS] (or [B,...])
    and ``rle`` int32 with ``n_rle`` counts as ntk_track_mask_* take them; ``rects`` float64 [T,B,4] and ``area`` [T,B] as
    ntk_track_mask_bounds left them; ``overlap`` float64 [..., MASK_OVERLAP_DOUBLES], set by whoever ran ntk_track_mask_overlaps
    on the tracked regions.  ``round[t]`` is frame t (views: nothing is copied)."""

    def __init__(self, cells, rle, n_rle, rects, area, overlap=None):
        self.cells, self.rle, self.n_rle, self.rects, self.area, self.overlap = cells, rle, int(n_rle), rects, area, overlap

    def __getitem__(self, t):
        return MaskRound(self.cells[t], self.rle, self.n_rle, self.rects[t], self.area[t],
                         None if self.overlap is None else self.overlap[t])

    def overlaps(self, regions, out=None):
        """One ntk_track_mask_overlaps of regions float64 [..., 4] (device) against these masks -> ``overlap`` (also kept)."""
        import torch
        from . import _lib
        n = self.cells.numel() // MASK_CELL_INTS
        if out is None:
            out = torch.empty(tuple(self.cells.shape[:-1]) + (MASK_OVERLAP_DOUBLES,), dtype=torch.float64, device=self.cells.device)
        if (regions.dtype != torch.float64 or regions.numel() != 4 * n or out.numel() != MASK_OVERLAP_DOUBLES * n
                or self.cells.dtype != torch.int32 or self.rle.dtype != torch.int32 or self.rle.numel() < max(self.n_rle, 1)):
            raise _lib.NtkError("MaskRound.overlaps: regions %s for %d masks" % (tuple(regions.shape), n))
        P = _lib.ptr
        _lib.check(_lib.lib().ntk_track_mask_overlaps(P(regions), P(self.cells), P(self.rle), self.n_rle, n, P(out), _lib.stream()),
                   "ntk_track_mask_overlaps")
        self.overlap = out
        return out


def upload_masks(per_cell, shape, device):
    """per_cell: ((index tuple into ``shape``), cells [k,6], counts) blocks, each filling k consecutive cells along the FIRST axis
    at the given index of the others -> MaskRound on the device: the cells with ``first`` rebased onto the concatenated counts,
    both through the pinned asynchronous upload, and ONE ntk_track_mask_bounds.  Cells no block names are absent objects."""
    import torch
    from . import _lib
    cells = np.zeros(tuple(shape) + (MASK_CELL_INTS,), dtype=np.int32)
    parts, n_rle = [], 0
    for index, c, counts in per_cell:
        c = c.copy()
        c[:, 4] += n_rle
        cells[(slice(0, len(c)),) + tuple(index)] = c
        parts.append(counts)
        n_rle += len(counts)
    if n_rle >= 2 ** 31:
        raise ValueError("the masks of a round hold %d counts; fewer than 2^31 fit" % n_rle)
    rle = np.concatenate(parts) if n_rle else np.zeros(1, dtype=np.int32)             # never an empty buffer
    d_cells, d_rle = _upload(cells, torch.int32, device), _upload(rle, torch.int32, device)
    rects = torch.empty(tuple(shape) + (4,), dtype=torch.float64, device=d_cells.device)
    area = torch.empty(tuple(shape), dtype=torch.float64, device=d_cells.device)
    P = _lib.ptr
    _lib.check(_lib.lib().ntk_track_mask_bounds(P(d_cells), P(d_rle), n_rle, cells.size // MASK_CELL_INTS, P(rects), P(area),
                                                _lib.stream()), "ntk_track_mask_bounds")
    return MaskRound(d_cells, d_rle, n_rle, rects, area)


class ClipSchedule(object):
    """Continuous batching of clips over B slots in rounds of T frames.  lengths[i]: frames of clip i INCLUDING its first one,
    which starts the tracker and is not tracked (so >= 2).  Clips are handed out in index order, at the start of a round, to the
    lowest free slot; a slot whose clip ends inside a round idles until the round ends.  With fewer clips than B the effective B
    (``self.B``) is the number of clips.

    Iterating yields Round(resets, frame_index, active, clip_of): ``resets`` a list of (slot, clip) started in this round;
    ``frame_index`` int64 [T,B], the frame of the slot's clip tracked at (t, b) (0 where inactive); ``active`` uint8 [T,B];
    ``clip_of`` int32 [B], -1 for a slot without a clip.  No two slots hold the same clip in a round."""

    def __init__(self, lengths, B, T):
        self.lengths = [int(n) for n in lengths]
        if int(B) < 1 or int(T) < 1:
            raise ValueError("ClipSchedule: B=%d T=%d" % (B, T))
        for i, n in enumerate(self.lengths):
            if n < 2:
                raise ValueError("ClipSchedule: clip %d has %d frame(s); a clip needs its first frame and one to track" % (i, n))
        self.B, self.T = max(1, min(int(B), len(self.lengths))), int(T)

    def __iter__(self):
        B, T, lengths = self.B, self.T, self.lengths
        clip, pos, upcoming = [-1] * B, [0] * B, 0
        while True:
            resets = []
            for s in range(B):
                if clip[s] < 0 and upcoming < len(lengths):
                    clip[s], pos[s] = upcoming, 1
                    resets.append((s, upcoming))
                    upcoming += 1
            if all(c < 0 for c in clip):
                return
            frame_index, active = np.zeros((T, B), dtype=np.int64), np.zeros((T, B), dtype=np.uint8)
            clip_of = np.asarray(clip, dtype=np.int32)
            for s in range(B):
                if clip[s] < 0:
                    continue
                n = min(T, lengths[clip[s]] - pos[s])
                frame_index[:n, s] = np.arange(pos[s], pos[s] + n)
                active[:n, s] = 1
                pos[s] += n
                if pos[s] == lengths[clip[s]]:
                    clip[s] = -1                    # free from the next round on
            yield Round(resets, frame_index, active, clip_of)


def regions_present(regions):
    """bool [L]: the frames of a clip whose ground truth is present, by the rule the score kernels use for its kind: a rectangle
    finite with w > 0 and h > 0, a polygon with a bounding rectangle (polygon_bounds), a mask with set pixels (mask_bounds)."""
    if isinstance(regions, MaskRegions):
        return np.isfinite(mask_bounds(regions)).all(axis=1)
    g = np.asarray(regions, dtype=np.float64)
    g = g if g.ndim == 2 and g.shape[1] != 4 else g.reshape(-1, 4)
    if g.shape[1] != 4:
        return np.isfinite(polygon_bounds(pad_polygons(g))).all(axis=1)
    with np.errstate(invalid="ignore"):
        return np.isfinite(g).all(axis=1) & (g[:, 2] > 0) & (g[:, 3] > 0)


class _DecodedOnce(object):
    """A callable clip behind its runs: ``frames()`` decodes the clip, or returns the decoded array while a run still holds a view
    of it.  The array is held weakly: the run views keep it alive through ``.base``, and it goes when the last of them does."""

    def __init__(self, decode):
        self.decode, self.held = decode, None

    def frames(self):
        import weakref
        a = None if self.held is None else self.held()
        if a is None:
            a = np.asarray(self.decode())
            a = a if a.dtype == np.uint8 else a.astype(np.float32, copy=False)      # what _ArraySource keeps: its views stay views
            if a.base is not None:
                a = a.copy()                            # a view of somebody else's memory cannot be the base of the run views
            self.held = weakref.ref(a)
        return a


def multistart_runs(clips, spacing=50, anchors=None):
    """The runs of the multi-start protocol (the rules: include/ntmtrack.h, NTK_MS_*) -> (run_clips, runs): ``runs``
    int64 [n_runs,4] = (clip, anchor, direction +1 / -1, length), ordered by clip, then by anchor; ``run_clips`` one ordinary Clip
    per run with the run's frames and regions in run order.

    The anchors of a clip of L >= 2 frames are {0, spacing, 2 spacing, ...} and L - 1, or ``anchors[i]`` where ``anchors`` is given
    (a list per clip).  An anchor a runs forward over a ... L - 1 when L - 1 - a >= a, else backward over a ... 0.  An anchor whose
    ground truth is absent (regions_present) moves along its own direction to the first frame where it is present (own rule); a
    run left with fewer than 2 frames is dropped, two runs with the same start and direction are one (the order is that of the
    anchors as given, which moving keeps within a direction).  A set without a run is a ValueError.

    Array frames become views, file lists re-ordered lists; a callable clip is decoded once for all of its runs that are alive at
    the same time (_DecodedOnce).  ``init`` goes only to the forward run from frame 0; ``size`` is copied."""
    if int(spacing) < 1:
        raise ValueError("multistart_runs: spacing=%d; at least 1" % spacing)
    clips = [_as_clip(c) for c in clips]
    if anchors is not None and len(anchors) != len(clips):
        raise ValueError("multistart_runs: %d anchor lists for %d clips" % (len(anchors), len(clips)))
    run_clips, runs = [], []
    for i, c in enumerate(clips):
        present = regions_present(c.regions)
        L = len(present)
        if L < 2:
            raise ValueError("multistart_runs: clip %d has %d frame(s); a clip needs 2" % (i, L))
        given = range(0, L, int(spacing)) if anchors is None else [int(a) for a in anchors[i]]
        if not all(0 <= a < L for a in given):
            raise ValueError("multistart_runs: clip %d: anchors %s outside [0,%d)" % (i, list(given), L))
        starts = []
        for a in sorted(set(given) | ({L - 1} if anchors is None else set())):
            step = 1 if L - 1 - a >= a else -1
            while 0 <= a < L and not present[a]:
                a += step
            if 0 <= a < L and (L - a if step > 0 else a + 1) >= 2 and (a, step) not in starts:
                starts.append((a, step))
        shared = _DecodedOnce(c.frames) if callable(c.frames) and starts else None
        is_mask = isinstance(c.regions, MaskRegions)
        for a, step in starts:
            order = np.arange(a, L) if step > 0 else np.arange(a, -1, -1)
            cut = slice(a, None) if step > 0 else slice(a, None, -1)
            if shared is not None:
                frames = lambda shared=shared, cut=cut: shared.frames()[cut]
            elif isinstance(c.frames, (list, tuple)):
                frames = [c.frames[k] for k in order]
            else:
                frames = np.asarray(c.frames)[cut]
            regions = c.regions.take(order) if is_mask else np.asarray(c.regions, dtype=np.float64).reshape(L, -1)[order]
            run_clips.append(Clip(frames, regions, c.init if (a, step) == (0, 1) else None, c.size))
            runs.append((i, a, step, len(order)))
    if not runs:
        raise ValueError("multistart_runs: the %d clip(s) yield no run" % len(clips))
    return run_clips, np.asarray(runs, dtype=np.int64).reshape(-1, 4)


def summarize(table, iou_thresholds, dist_thresholds):
    """The host arithmetic of OverlapScores.result(): table [n_clips, SCORE_HEAD + n_iou + n_dist] float64 -> dict (see result)."""
    table = np.asarray(table, dtype=np.float64)
    iou_thr, dist_thr = np.asarray(iou_thresholds, dtype=np.float64), np.asarray(dist_thresholds, dtype=np.float64)
    n_iou, n_dist = len(iou_thr), len(dist_thr)
    frames = table[:, SCORE_FRAMES]
    scored = frames > 0
    per = np.where(scored, frames, np.nan)[:, None]                     # a clip without scored frames: NaN means
    succ, prec = table[:, SCORE_HEAD:SCORE_HEAD + n_iou], table[:, SCORE_HEAD + n_iou:SCORE_HEAD + n_iou + n_dist]
    clips = {"frames": frames.astype(np.int64), "mean_overlap": table[:, SCORE_SUM_IOU] / per[:, 0],
             "mean_centre_error": table[:, SCORE_SUM_DIST] / per[:, 0], "lost": table[:, SCORE_LOST].astype(np.int64),
             "first_lost": table[:, SCORE_FIRST_LOST].astype(np.int64), "success": succ / per, "precision": prec / per}
    total = frames.sum()
    over = total if total > 0 else np.nan
    success_curve, precision_curve = succ.sum(axis=0) / over, prec.sum(axis=0) / over
    at20 = np.nonzero(dist_thr == 20.0)[0]
    return {"clips": clips, "iou_thresholds": iou_thr, "dist_thresholds": dist_thr,
            "frames": int(total), "clips_scored": int(scored.sum()), "clips_without_frames": int((~scored).sum()),
            "mean_overlap_frames": table[:, SCORE_SUM_IOU].sum() / over,
            "mean_overlap_clips": float(np.mean(clips["mean_overlap"][scored])) if scored.any() else np.nan,
            "mean_centre_error_frames": table[:, SCORE_SUM_DIST].sum() / over,
            "success_curve": success_curve, "success_auc": float(np.mean(success_curve)) if n_iou else np.nan,
            "precision_curve": precision_curve, "precision_20px": float(precision_curve[at20[0]]) if len(at20) else np.nan,
            "lost": int(table[:, SCORE_LOST].sum()),
            "clips_never_lost": int((scored & (table[:, SCORE_FIRST_LOST] < 0)).sum())}


def _scoring_call(who, entry, device, regions, gt, clip_of, active, frame_iou):
    """What OverlapScores.add and MultiStart.add share: the arguments of one scoring launch over a round, checked and on the device
    (tensors there are taken as they are, host arrays go up through the pinned asynchronous copy).  -> (the entry point's name for
    the kind of ground truth, regions [T,B,4], the ground truth's pointers -- for a MaskRound after its ONE ntk_track_mask_overlaps
    --, active [T,B] or None, clip_of [B], T, B, the frame_iou buffer or None, the tensors behind those pointers: held by the caller
    until it has launched)."""
    import torch
    from . import _lib

    def dev(x, dtype):
        if torch.is_tensor(x) and x.device.type == device.type:
            return x.to(dtype).contiguous()
        return _upload(x.cpu().numpy() if torch.is_tensor(x) else np.asarray(x), dtype, device)
    masks = gt if isinstance(gt, MaskRound) else None
    regions, gt = dev(regions, torch.float64), masks.rects if masks is not None else dev(gt, torch.float64)
    if regions.dim() == 2:
        regions, gt = regions.unsqueeze(0), gt.unsqueeze(0)
    poly = gt.dim() == 3 and gt.shape[2] == POLY_DOUBLES
    if (regions.dim() != 3 or regions.shape[2] != 4 or gt.dim() != 3 or gt.shape[:2] != regions.shape[:2]
            or gt.shape[2] not in (4, POLY_DOUBLES)):
        raise _lib.NtkError("%s: regions %s must be [T,B,4] and gt %s [T,B,4] or [T,B,%d]"
                            % (who, tuple(regions.shape), tuple(gt.shape), POLY_DOUBLES))
    T, B = regions.shape[:2]
    clip_of = dev(clip_of, torch.int32)
    mask = None if active is None else dev(active, torch.uint8).reshape(-1, B)
    if tuple(clip_of.shape) != (B,) or (mask is not None and tuple(mask.shape) != (T, B)):
        raise _lib.NtkError("%s: clip_of %s / active %s for [T,B] = [%d,%d]"
                            % (who, tuple(clip_of.shape), None if mask is None else tuple(mask.shape), T, B))
    out = torch.empty((T, B), dtype=torch.float64, device=device) if frame_iou else None
    P = _lib.ptr
    name = entry + ("_mask" if masks is not None else "_poly" if poly else "")
    truth = (P(gt),) if masks is None else (P(gt), P(masks.overlaps(regions)))
    return name, regions, truth, mask, clip_of, T, B, out, (gt, masks)


class OverlapScores(object):
    """The score table of n_clips clips ([n_clips, SCORE_HEAD + n_iou + n_dist] float64, ``self.table``) and the two threshold
    arrays, on the device.  ``add`` is one launch of ntk_track_overlap_scores and synchronises nothing; ``result`` is the one
    synchronising call."""

    def __init__(self, n_clips, iou_thresholds=None, dist_thresholds=None, device="cuda"):
        import torch
        self.iou_thresholds = np.asarray(np.linspace(0, 1, 21) if iou_thresholds is None else iou_thresholds, dtype=np.float64).reshape(-1)
        self.dist_thresholds = np.asarray(np.arange(0, 51.) if dist_thresholds is None else dist_thresholds, dtype=np.float64).reshape(-1)
        if int(n_clips) < 1 or max(len(self.iou_thresholds), len(self.dist_thresholds)) > SCORE_MAX_THRESHOLDS:
            raise ValueError("OverlapScores: n_clips=%d, %d and %d thresholds (at most %d each)"
                             % (n_clips, len(self.iou_thresholds), len(self.dist_thresholds), SCORE_MAX_THRESHOLDS))
        self.n_clips, self.device = int(n_clips), torch.device(device)
        self.table = torch.zeros((self.n_clips, SCORE_HEAD + len(self.iou_thresholds) + len(self.dist_thresholds)),
                                 dtype=torch.float64, device=self.device)
        self.table[:, SCORE_FIRST_LOST] = -1
        self._iou = torch.as_tensor(self.iou_thresholds).to(self.device)
        self._dist = torch.as_tensor(self.dist_thresholds).to(self.device)

    def add(self, regions, gt, clip_of, active=None, frame_iou=False):
        """regions, gt: [T,B,4] or [B,4] (x, y, w, h) pixels, or gt [T,B,16] / [B,16] polygons (then one launch of
        ntk_track_overlap_scores_poly), or gt a MaskRound of [T,B] / [B] masks (then one ntk_track_mask_overlaps of the regions
        against the masks and one ntk_track_overlap_scores_mask); clip_of [B]: the table row of slot b, no row twice (a row outside
        the table skips the slot); active [T,B] or [B], nullable.  Device tensors are taken as they are, host arrays go up through
        a pinned asynchronous copy.  frame_iou=True returns the per-frame IoUs [T,B] (NaN where a frame was not scored)."""
        from . import _lib
        P = _lib.ptr
        name, regions, truth, mask, clip_of, T, B, out, _held = _scoring_call("OverlapScores.add", "ntk_track_overlap_scores",
                                                                              self.device, regions, gt, clip_of, active, frame_iou)
        _lib.check(getattr(_lib.lib(), name)(P(regions), *truth, P(mask), P(clip_of), T, B, self.n_clips,
                                             P(self._iou) if len(self.iou_thresholds) else None, len(self.iou_thresholds),
                                             P(self._dist) if len(self.dist_thresholds) else None, len(self.dist_thresholds),
                                             P(self.table), P(out), _lib.stream()), name)
        return out

    def result(self):
        """Reads the table back (the one synchronisation).  -> dict: ``clips`` holds per clip ``frames``, ``mean_overlap``,
        ``mean_centre_error`` (px), ``lost``, ``first_lost`` (frames scored before the first lost one, -1 = never), ``success``
        [n_clips,n_iou] and ``precision`` [n_clips,n_dist] (rates); over the dataset ``frames``, ``mean_overlap_frames``
        (frame-weighted), ``mean_overlap_clips`` (clip-weighted), ``mean_centre_error_frames``, ``success_curve`` and
        ``success_auc`` (the mean of the success rates over the thresholds), ``precision_curve`` and ``precision_20px`` (NaN
        without a 20 px threshold), ``lost``, ``clips_never_lost``, ``clips_scored`` and ``clips_without_frames``.  A clip with
        no scored frame has NaN means, is left out of the clip-weighted figures and is counted in ``clips_without_frames``."""
        return summarize(self.table.cpu().numpy(), self.iou_thresholds, self.dist_thresholds)


def summarize_supervised(table):
    """The host arithmetic of Supervisor.result(): table [n_clips, SUP_HEAD] float64 -> dict.  ``clips`` holds per clip ``accuracy``
    (SUM_IOU / VALID: the mean overlap outside the burn-in after every start; NaN without a valid frame), ``valid``, ``failures``,
    ``restarts``, ``tracked`` (frames judged), ``skipped`` and ``first_failure`` (frames judged before the first failure, -1 =
    never); over the set ``accuracy_clips`` (the mean over the clips that have one), ``accuracy_frames`` (frame-weighted),
    ``failures``, ``restarts``, ``tracked``, ``skipped``, ``valid``, ``failures_per_100_frames`` (of the judged frames) and
    ``clips_never_failed``."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, SUP_HEAD)
    valid = table[:, SUP_VALID]
    has = valid > 0
    accuracy = table[:, SUP_SUM_IOU] / np.where(has, valid, np.nan)
    as_int = lambda c: table[:, c].astype(np.int64)
    clips = {"accuracy": accuracy, "valid": as_int(SUP_VALID), "failures": as_int(SUP_FAILURES), "restarts": as_int(SUP_RESTARTS),
             "tracked": as_int(SUP_TRACKED), "skipped": as_int(SUP_SKIPPED), "first_failure": as_int(SUP_FIRST_FAILURE)}
    tracked, total_valid = table[:, SUP_TRACKED].sum(), valid.sum()
    return {"clips": clips,
            "accuracy_clips": float(np.mean(accuracy[has])) if has.any() else np.nan,
            "accuracy_frames": table[:, SUP_SUM_IOU].sum() / (total_valid if total_valid > 0 else np.nan),
            "failures": int(table[:, SUP_FAILURES].sum()), "restarts": int(table[:, SUP_RESTARTS].sum()),
            "tracked": int(tracked), "skipped": int(table[:, SUP_SKIPPED].sum()), "valid": int(total_valid),
            "failures_per_100_frames": 100.0 * table[:, SUP_FAILURES].sum() / (tracked if tracked > 0 else np.nan),
            "clips_never_failed": int(((table[:, SUP_TRACKED] > 0) & (table[:, SUP_FIRST_FAILURE] < 0)).sum())}


class Supervisor(object):
    """The supervised protocol for B slots and n_clips clips on the device (the rules: include/ntmtrack.h, ntk_track_supervise): a
    slot whose overlap falls to ``failure_overlap`` or below has failed, sits ``skip`` frames out and is started again from the
    ground truth; a frame counts towards accuracy when more than ``burn_in`` frames were tracked since the last start.
    ``state`` int32 [B, SUP_STATE_INTS] and ``table`` float64 [n_clips, SUP_HEAD] live on the device; ``plan`` and ``judge`` are
    one launch each and synchronise nothing, ``result`` is the one synchronising call."""

    def __init__(self, B, n_clips, skip=5, burn_in=10, failure_overlap=0.0, device="cuda"):
        import torch
        self.B, self.n_clips = int(B), int(n_clips)
        self.skip, self.burn_in, self.failure_overlap = int(skip), int(burn_in), float(failure_overlap)
        if self.B < 1 or self.n_clips < 1 or self.skip < 1 or self.burn_in < 0 or not 0 <= self.failure_overlap < 1:
            raise ValueError("Supervisor: B=%d n_clips=%d skip=%d (>= 1) burn_in=%d (>= 0) failure_overlap=%g (in [0,1))"
                             % (self.B, self.n_clips, self.skip, self.burn_in, self.failure_overlap))
        self.device = torch.device(device)
        self.state = torch.zeros((self.B, SUP_STATE_INTS), dtype=torch.int32, device=self.device)      # (TRACK, 0, 0)
        self.table = torch.zeros((self.n_clips, SUP_HEAD), dtype=torch.float64, device=self.device)
        self.table[:, SUP_FIRST_FAILURE] = -1
        self.track = torch.zeros((self.B,), dtype=torch.uint8, device=self.device)
        self.restart = torch.zeros((self.B,), dtype=torch.uint8, device=self.device)
        self.codes = None                               # [T,B] int8 of the last track_clip

    def start(self, slots):
        """The slots take a new clip: their state rows become (TRACK, 0, 0).  An index fill from a pinned upload: no synchronisation."""
        import torch
        slots = [int(s) for s in slots]
        if not all(0 <= s < self.B for s in slots):
            raise ValueError("Supervisor.start: slots %s outside [0,%d)" % (slots, self.B))
        if slots:
            self.state.index_fill_(0, _upload(np.asarray(slots), torch.int64, self.device), 0)

    def _call(self, phase, regions, gt, active, clip_of, codes, frame_iou):
        import torch
        from . import _lib
        masks = gt if isinstance(gt, MaskRound) else None          # plan and judge on the masks' rects; judge reads their overlap
        if masks is not None:
            gt = masks.rects
            if phase == SUP_JUDGE and (not torch.is_tensor(masks.overlap) or masks.overlap.dtype != torch.float64
                                       or tuple(masks.overlap.shape) != (self.B, MASK_OVERLAP_DOUBLES)):
                raise _lib.NtkError("Supervisor: judge needs the masks' overlap, a float64 tensor of shape %s"
                                    % ((self.B, MASK_OVERLAP_DOUBLES),))
        poly = torch.is_tensor(gt) and gt.dim() == 2 and gt.shape[1] == POLY_DOUBLES
        for name, t, dtype, shape in (("regions", regions, torch.float64, (self.B, 4)),
                                      ("gt", gt, torch.float64, (self.B, POLY_DOUBLES if poly else 4)),
                                      ("active", active, torch.uint8, (self.B,)), ("clip_of", clip_of, torch.int32, (self.B,)),
                                      ("codes", codes, torch.int8, (self.B,)), ("frame_iou", frame_iou, torch.float64, (self.B,))):
            if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape):
                raise _lib.NtkError("Supervisor: %s must be a %s tensor of shape %s" % (name, dtype, shape))
        P = _lib.ptr
        fn = "ntk_track_supervise_mask" if masks is not None else "ntk_track_supervise_poly" if poly else "ntk_track_supervise"
        truth = (P(gt),) if masks is None else (P(gt), P(masks.overlap) if phase == SUP_JUDGE else None)
        _lib.check(getattr(_lib.lib(), fn)(phase, P(regions), *truth, P(active), P(clip_of), self.B, self.n_clips, self.skip,
                                           self.burn_in, self.failure_overlap, P(self.state), P(self.table), P(self.track),
                                           P(self.restart), P(codes), P(frame_iou), _lib.stream()), fn)

    def plan(self, gt_t, active_t, clip_of, codes=None, frame_iou=None):
        """Before the frame's pass.  gt_t float64 [B,4] (or [B,16] polygons: ntk_track_supervise_poly; or a frame of a MaskRound: ntk_track_supervise_mask), active_t uint8 [B] (nullable), clip_of int32 [B], on the device.
        -> (track, restart) uint8 [B]: the masks of the pass (the supervisor's own buffers, overwritten by the next plan).  codes
        int8 [B] and frame_iou float64 [B] (nullable) are filled for every slot."""
        self._call(SUP_PLAN, None, gt_t, active_t, clip_of, codes, frame_iou)
        return self.track, self.restart

    def judge(self, regions, gt_t, clip_of, codes=None, frame_iou=None):
        """After the pass: the tracked slots (the last plan's ``track``) are scored against gt_t; codes / frame_iou as given to
        plan are completed."""
        self._call(SUP_JUDGE, regions, gt_t, None, clip_of, codes, frame_iou)

    def result(self):
        """Reads the table back (the one synchronisation) -> summarize_supervised(table)."""
        return summarize_supervised(self.table.cpu().numpy())


def summarize_multistart(table, runs, curve, eao_interval, n_clips=None):
    """The host arithmetic of MultiStart.result(): table [n_runs, MS_HEAD] float64 of FINISHED runs, runs int64 [n_runs,4] (clip,
    anchor, direction, length: multistart_runs), curve [n_max] = Phi(1 ... n_max) (ntk_track_eao_curve), eao_interval (lo, hi)
    -> dict.  Of a run: N = FRAMES; N_F = TRACKED if it FAILED, else N (a streak open at the end is forgiven); sum = SUM_IOU if
    it failed, else PENDING.  ``per_run`` holds per run ``clip``, ``anchor``, ``direction``, ``frames`` (N), ``tracked`` (N_F),
    ``failed``, ``accuracy`` (sum / N_F, NaN for N_F = 0) and ``robustness`` (N_F / N, NaN for N = 0); ``clips`` per clip (n_clips
    of them, by default as many as the runs name) ``runs``, ``accuracy`` (sum of the sums / sum of N_F over its runs) and
    ``robustness`` (sum of N_F / sum of N), NaN where the denominator is 0; over the set ``accuracy`` and ``robustness`` by the same
    two formulas, ``eao`` (the mean of the curve's non-NaN points over n in [lo, hi]; NaN without one), ``eao_points`` (how many
    they were), ``eao_curve``, ``eao_interval``, ``failures``, ``runs`` (their number), ``runs_without_frames`` (N = 0: such a run takes part
    in nothing) and ``clips_without_runs``."""
    table = np.asarray(table, dtype=np.float64).reshape(-1, MS_HEAD)
    runs = np.asarray(runs, dtype=np.int64).reshape(-1, 4)
    curve = np.asarray(curve, dtype=np.float64).reshape(-1)
    lo, hi = int(eao_interval[0]), int(eao_interval[1])
    if len(runs) != len(table) or lo < 1 or hi < lo or hi > len(curve):
        raise ValueError("summarize_multistart: %d runs for %d table rows, eao_interval (%d, %d) on a curve of %d points"
                         % (len(runs), len(table), lo, hi, len(curve)))
    failed = table[:, MS_FAILED] != 0
    n = table[:, MS_FRAMES]
    n_f = np.where(failed, table[:, MS_TRACKED], n)
    total = np.where(failed, table[:, MS_SUM_IOU], table[:, MS_PENDING])
    has = n > 0
    n_f, total, failed = np.where(has, n_f, 0.0), np.where(has, total, 0.0), failed & has
    over = lambda a, b: a / np.where(b > 0, b, np.nan)
    n_clips = (int(runs[:, 0].max()) + 1 if len(runs) else 0) if n_clips is None else int(n_clips)
    per_clip = lambda v: np.bincount(runs[:, 0], weights=v, minlength=n_clips)
    runs_of = np.bincount(runs[:, 0], minlength=n_clips)
    window = curve[lo - 1:hi]
    used = ~np.isnan(window)
    return {"per_run": {"clip": runs[:, 0].copy(), "anchor": runs[:, 1].copy(), "direction": runs[:, 2].copy(),
                        "frames": n.astype(np.int64), "tracked": n_f.astype(np.int64), "failed": failed,
                        "accuracy": over(total, n_f), "robustness": over(n_f, n)},
            "clips": {"runs": runs_of, "accuracy": over(per_clip(total), per_clip(n_f)), "robustness": over(per_clip(n_f), per_clip(n))},
            "accuracy": float(over(total.sum(), n_f.sum())), "robustness": float(over(n_f.sum(), n.sum())),
            "eao": float(window[used].mean()) if used.any() else np.nan, "eao_points": int(used.sum()), "eao_curve": curve,
            "eao_interval": (lo, hi), "failures": int(failed.sum()), "runs": len(runs),
            "runs_without_frames": int((~has).sum()), "clips_without_runs": int((runs_of == 0).sum())}


class MultiStart(object):
    """The multi-start protocol for n_runs runs on the device (the rules: include/ntmtrack.h, ntk_track_multistart): ``table``
    float64 [n_runs, MS_HEAD], one row per run, which holds ALL of the protocol's state -- there is nothing per slot and nothing
    to start --, and ``trace`` float64 [trace_first[n_runs]], every scored frame's overlap, run r's from trace_first[r] on.
    ``trace_first`` int64 [n_runs + 1] (a run of L frames takes L - 1 entries) is uploaded once.  ``add`` is one launch and
    synchronises nothing; ``result`` launches the EAO reduction and is the one synchronising call."""

    def __init__(self, n_runs, trace_first, failure_overlap=0.1, patience=10, device="cuda"):
        import torch
        self.n_runs, self.failure_overlap, self.patience = int(n_runs), float(failure_overlap), int(patience)
        first = np.ascontiguousarray(trace_first, dtype=np.int64).reshape(-1)
        if (self.n_runs < 1 or len(first) != self.n_runs + 1 or first[0] != 0 or (np.diff(first) < 0).any() or self.patience < 0
                or not 0 <= self.failure_overlap < 1):
            raise ValueError("MultiStart: n_runs=%d, %d ascending trace_first entries from 0 (n_runs + 1), patience=%d (>= 0), "
                             "failure_overlap=%g (in [0,1))" % (self.n_runs, len(first), self.patience, self.failure_overlap))
        self.device = torch.device(device)
        self.trace_first = first
        self._first = _upload(first, torch.int64, self.device)
        self.table = torch.zeros((self.n_runs, MS_HEAD), dtype=torch.float64, device=self.device)
        self.trace = torch.zeros((max(int(first[-1]), 1),), dtype=torch.float64, device=self.device)      # never an empty buffer

    def add(self, regions, gt, clip_of, active=None, frame_iou=False):
        """OverlapScores.add's arguments (clip_of [B]: the RUN of slot b) -> one ntk_track_multistart, _poly or (after the
        MaskRound's one ntk_track_mask_overlaps) _mask."""
        from . import _lib
        P = _lib.ptr
        name, regions, truth, mask, clip_of, T, B, out, _held = _scoring_call("MultiStart.add", "ntk_track_multistart", self.device,
                                                                              regions, gt, clip_of, active, frame_iou)
        _lib.check(getattr(_lib.lib(), name)(P(regions), *truth, P(mask), P(clip_of), T, B, self.n_runs, self.failure_overlap,
                                             self.patience, P(self.table), P(self._first), P(self.trace), P(out), _lib.stream()), name)
        return out

    def curve(self, n_max):
        """One ntk_track_eao_curve over the runs as they stand -> Phi(1 ... n_max), float64 [n_max] on the device (no
        synchronisation; the prefix sums go to a buffer of the trace's size that lives for this call)."""
        import torch
        from . import _lib
        P = _lib.ptr
        prefix = torch.empty_like(self.trace)
        curve = torch.empty((int(n_max),), dtype=torch.float64, device=self.device)
        _lib.check(_lib.lib().ntk_track_eao_curve(P(self.table), P(self._first), P(self.trace), self.n_runs, int(n_max), P(prefix),
                                                  P(curve), _lib.stream()), "ntk_track_eao_curve")
        return curve

    def result(self, eao_interval=(115, 755), runs=None, n_clips=None):
        """Launches the EAO reduction (n_max = hi) and reads the table and the curve back in ONE copy (the one synchronisation)
        -> summarize_multistart.  runs: multistart_runs' (by default every run is its own clip, started at frame 0)."""
        import torch
        hi = int(eao_interval[1])
        if int(eao_interval[0]) < 1 or hi < int(eao_interval[0]):
            raise ValueError("MultiStart.result: eao_interval=%s; 1 <= lo <= hi" % (tuple(eao_interval),))
        host = torch.cat([self.table.reshape(-1), self.curve(hi)]).cpu().numpy()
        if runs is None:
            runs = np.stack([np.arange(self.n_runs), np.zeros(self.n_runs), np.ones(self.n_runs), np.diff(self.trace_first) + 1], axis=1)
        return summarize_multistart(host[:self.n_runs * MS_HEAD], runs, host[self.n_runs * MS_HEAD:], eao_interval, n_clips)


def _as_clip(c):
    if isinstance(c, Clip):
        return c
    if isinstance(c, dict):
        return Clip(c["frames"], c["regions"], c.get("init"), c.get("size"))
    if isinstance(c, (tuple, list)):
        return Clip(*c)
    return Clip(c.frames, c.regions, getattr(c, "init", None), getattr(c, "size", None))


class _SizeClass(object):
    def __init__(self, size, members, schedule):
        self.size, self.members, self.schedule = size, members, schedule      # members: the caller's clip indices, in order;
        self.tracker = self.supervisor = None                                 # schedule() -> the ClipSchedule of their rounds
        self.source = None              # where the rounds' frames come from: _ArraySource, _HostFileSource or _DeviceFileSource

    def ids(self, rnd):
        """int32 [B]: the caller's clip index of every slot of the round, -1 for a slot without a clip."""
        return np.where(rnd.clip_of >= 0, np.asarray(self.members, dtype=np.int64)[np.maximum(rnd.clip_of, 0)], -1).astype(np.int32)


RoundInput = collections.namedtuple("RoundInput", ["firsts", "frames", "active", "d_ids", "tracked"])


class _Source(object):
    """Where a size class's frames come from, one round at a time.  ``round(rnd, ids)`` -> RoundInput: firsts, the starting
    images of the slots reset in the round, in reset order, as make_tracker and reset take them; frames [T,B,H,W,3], a host array
    or a device tensor, as track_clip takes them; active uint8 [T,B] and d_ids int32 [B] on the device; tracked, the [T,B] mask
    regions() reads: the schedule's, on the host, or `active` itself where the device turned frames off.  ``consumed()``: the
    round's tracker and scoring launches are enqueued.  ``close()`` stops the source's own threads."""

    def consumed(self):
        pass

    def close(self):
        pass


class _ArraySource(_Source):
    """The frames of a size class whose clips are arrays or callables.  ``held``: clip index -> decoded frames, from the round
    that resets the clip to the round that hands out its last frame."""

    def __init__(self, cls, clips, lengths, device):
        self.cls, self.clips, self.lengths, self.device, self.held = cls, clips, lengths, device, {}

    def clip_frames(self, i):
        if i not in self.held:
            f = self.clips[i].frames
            a = np.asarray(f() if callable(f) else f)
            if a.ndim != 4 or a.shape[3] != 3 or a.shape[0] != self.lengths[i]:
                raise ValueError("clip %d: frames %s for %d regions; expected [L,H,W,3]" % (i, a.shape, self.lengths[i]))
            self.held[i] = a if a.dtype == np.uint8 else a.astype(np.float32, copy=False)
        return self.held[i]

    def host_round(self, rnd, ids):
        """The host half (NumPy only) -> (firsts [n_resets,H,W,3] or None, frames [T,B,H,W,3]): uint8 where every clip involved
        is, else float32; zero frames (the crop kernel still reads them) where a cell is inactive."""
        T, B = rnd.active.shape
        firsts = None
        if rnd.resets:
            firsts = [self.clip_frames(self.cls.members[c])[0] for _s, c in rnd.resets]
            firsts = np.stack(firsts).astype(np.uint8 if all(f.dtype == np.uint8 for f in firsts) else np.float32, copy=False)
        held = [None if i < 0 else self.clip_frames(int(i)) for i in ids]
        u8 = all(h is None or h.dtype == np.uint8 for h in held)
        frames = np.zeros((T, B) + tuple(self.cls.size) + (3,), dtype=np.uint8 if u8 else np.float32)
        for b in range(B):
            n = int(rnd.active[:, b].sum())
            if n:
                at = rnd.frame_index[:n, b]
                frames[:n, b] = held[b][at[0]:at[-1] + 1]
                if at[-1] + 1 == self.lengths[int(ids[b])]:
                    del self.held[int(ids[b])]          # the clip has ended
        return firsts, frames

    def round(self, rnd, ids):
        import torch
        firsts, frames = self.host_round(rnd, ids)
        return RoundInput(firsts, frames, _upload(rnd.active, torch.uint8, self.device), _upload(ids, torch.int32, self.device),
                          rnd.active)


class _FileDecoding(object):
    """What the file sources of ONE Validation share: the pool of reader threads, the decode stream, the per-clip decode table
    of all clips (ntk_track_decode_mask's) and the counts of files decoded on either side."""

    def __init__(self, decode, prefetch, workers, n_clips, device):
        self.decode, self.prefetch, self.workers, self.n_clips, self.device = decode, prefetch, workers, n_clips, device
        self.pool = self.stream = self.table = None
        self.frames_on_device = self.frames_on_host = 0

    def reader_pool(self):
        if self.pool is None and self.workers > 1:
            from concurrent.futures import ThreadPoolExecutor
            self.pool = ThreadPoolExecutor(max_workers=self.workers)
        return self.pool

    def decode_stream(self, tracking):
        """The decode stream, made behind the tracking stream's work at its first use, with the decode table."""
        import torch
        if self.stream is None:
            self.stream = torch.cuda.Stream(self.device)
            self.table = torch.zeros((self.n_clips, CLIPDEC_HEAD), dtype=torch.int64, device=self.device)
            self.table[:, CLIPDEC_FIRST_FAILED] = -1
            self.stream.wait_stream(tracking)
        return self.stream

    def close(self):
        if self.pool is not None:
            self.pool.shutdown(wait=True)
            self.pool = None


class _HostFileSource(_Source):
    """The frames of a size class of file clips, decoded by Pillow: a data.InputPrefetcher (made with the first round) stages
    round r + 1 while round r runs; the pinned block goes up as it is, as track_clip would upload it."""

    def __init__(self, cls, clips, shared):
        self.cls, self.shared, self.prefetcher = cls, shared, None
        self.files = [clips[i].frames for i in cls.members]

    def round_files(self, rnd):
        """-> data.RoundFiles of a round: the file of every active cell and the starting frames of the resets."""
        from .data import RoundFiles
        T, B = rnd.active.shape
        cells = [(int(t), int(b), self.files[int(rnd.clip_of[b])][int(rnd.frame_index[t, b])]) for t, b in zip(*np.nonzero(rnd.active))]
        starts = [(int(s), self.files[c][0]) for s, c in rnd.resets]
        return RoundFiles(self.cls.size, T, B, cells, starts)

    def staged_round(self):
        """The next staged round, in the schedule's order."""
        from . import data
        sh = self.shared
        if self.prefetcher is None:
            pool = sh.reader_pool()
            specs = (self.round_files(rnd) for rnd in self.cls.schedule())
            stage = lambda spec, staging: data.stage_round(spec, staging, pool, grow=False, decode=sh.decode)
            self.prefetcher = data.InputPrefetcher(specs, depth=sh.prefetch, workers=1, stage=stage, decode=sh.decode)
        try:
            return next(self.prefetcher)
        except StopIteration:
            raise RuntimeError("Validation: the prefetcher ended before the schedule did")

    def round(self, rnd, ids):
        import torch
        staged, dev = self.staged_round(), self.shared.device
        frames, firsts = staged.host_frames()
        self.shared.frames_on_host += staged.packed.n
        firsts = firsts.copy()                          # the caller's to keep: the pinned set is refilled
        frames = _upload(frames, torch.uint8, dev)
        staged.uploaded = torch.cuda.Event()            # the prefetcher refills the set only after this copy has run
        staged.uploaded.record()
        return RoundInput(firsts, frames, _upload(rnd.active, torch.uint8, dev), _upload(ids, torch.int32, dev), rnd.active)

    def close(self):
        if self.prefetcher is not None:
            self.prefetcher.close()


class _DeviceFileSource(_HostFileSource):
    """The same files decoded on the device: ONE ntk_jpeg_decode_batch per round on the shared decode stream, a round ahead of
    the tracker, and ntk_track_decode_mask on the tracking stream.  The two streams are ordered by events alone: "set k decoded"
    and "set k consumed" (the tracking stream has read the set's device buffers: the decode stream may write them again)."""

    def __init__(self, cls, clips, shared):
        _HostFileSource.__init__(self, cls, clips, shared)
        self.dead = None                # uint8 [B] on the device: the slots whose clip started from an undecodable frame
        self.was_consumed, self.current = {}, None      # id(staging set) -> its "consumed" event; the set of the round under way

    def round(self, rnd, ids):
        """-> frames [T,B,H,W,3] and starting frames [n_resets,H,W,3] as uint8 views of the set's device pixel buffer (cells
        without a file hold whatever the buffer held: never read into a result) and the masked active."""
        from . import _lib, data
        import torch
        sh, dev = self.shared, self.shared.device
        T, B = rnd.active.shape
        H, W = self.cls.size
        staged = self.staged_round()
        d_ids = _upload(ids, torch.int32, dev)
        tracking = torch.cuda.current_stream(dev)
        stream = sh.decode_stream(tracking)
        if self.dead is None:
            self.dead = torch.zeros((B,), dtype=torch.uint8, device=dev)
        self.current = id(staged.packed.staging)
        staged.uploaded, decoded = torch.cuda.Event(), torch.cuda.Event()
        with torch.cuda.stream(stream):
            if self.current in self.was_consumed:
                stream.wait_event(self.was_consumed[self.current])
            pix, _table, status = data.decode_packed(staged.packed, dev, uploaded=staged.uploaded)
            decoded.record()
        # allocated under the decode stream, read on the tracking stream
        pix.record_stream(tracking)
        status.record_stream(tracking)
        tracking.wait_event(decoded)
        on_device = sum(staged.packed.jpeg.on_device)
        sh.frames_on_device, sh.frames_on_host = sh.frames_on_device + on_device, sh.frames_on_host + staged.packed.n - on_device
        active = _upload(rnd.active, torch.uint8, dev)
        cell_index = _upload(staged.cell_index, torch.int32, dev)
        start_index = _upload(staged.start_index, torch.int32, dev)
        P = _lib.ptr
        _lib.check(_lib.lib().ntk_track_decode_mask(P(status), staged.packed.n, P(cell_index), P(start_index), P(d_ids), T, B,
                                                    sh.n_clips, P(self.dead), P(active), P(sh.table), _lib.stream()),
                   "ntk_track_decode_mask")
        frame, n = H * W * 3, len(rnd.resets)
        return RoundInput(pix[T * B * frame:(T * B + n) * frame].view(n, H, W, 3), pix[:T * B * frame].view(T, B, H, W, 3),
                          active, d_ids, active)

    def consumed(self):
        import torch
        event = self.was_consumed[self.current] = torch.cuda.Event()
        event.record()


class Validation(object):
    """Validates a tracker over clips: ``make_tracker(first_images [B,H,W,3], regions [B,4])`` -> a BatchNTMTracker or
    BatchDNCTracker (one per frame size; both share the online contract), ``clips`` a sequence of Clip (or objects / dicts with
    ``frames`` and ``regions``).  ``step()`` runs one round -- reset for the slots that take a new clip, one track_clip over
    frames [T,B,H,W,3] with the round's mask, one scores.add -- and returns False when no round was left.  After the first round
    of a frame size (which builds the tracker, its plans and workspaces) a round makes no host synchronisation.  ``scores`` is
    the OverlapScores, rows in the caller's clip order; ``regions()`` the tracked regions per clip when return_regions was set.

    ``protocol="supervised"`` runs the supervised protocol instead (Supervisor; ``skip``, ``burn_in``, ``failure_overlap``): the
    same schedule and the same resets, a round is one track_clip with the supervisor, which restarts a lost slot from the ground
    truth inside the pass.  ``supervisor`` then holds the table (``scores`` stays empty), ``codes()`` the per-frame codes per clip
    beside ``regions()``, whose skipped frames hold NaN.  Still no host synchronisation after the first round of a frame size.

    ``protocol="multistart"`` runs the multi-start (anchor-based) protocol of the VOT sets from 2020 on (``spacing``, ``anchors``,
    ``failure_overlap``, 0.1 unless given, ``patience``, ``eao_interval``): the clips are expanded into their runs (multistart_runs;
    ``runs``, ``source_clips``), the runs are scheduled exactly as clips are -- ``clips``, ``regions()`` and every table are per
    RUN, in run order -- and a round's scoring launch is ONE ``multistart.add`` (MultiStart) in place of scores.add (``scores``
    stays empty).  The schedule is static: a run that has failed is still tracked to its scheduled end, which costs the frames
    behind every failure.  Still no host synchronisation after the first round of a frame size.

    Clips with polygon regions ([L,2P]) are scored against the polygons in both protocols; their trackers start, and restart, from
    the polygons' bounding rectangles.  Rectangle clips in the same run are scored as 4-gons.  The polygons go up through the same
    pinned asynchronous copy, so a round still makes no host synchronisation.

    Clips whose regions are MaskRegions (segmentation masks) are scored against the masks in both protocols, straight from the
    run-length counts: per round the cells [T,B,6] and the concatenated counts go up through the same pinned copy, ONE
    ntk_track_mask_bounds gives the rectangles the trackers start and restart from, and the one-pass protocol adds ONE
    ntk_track_mask_overlaps and ONE ntk_track_overlap_scores_mask (the supervised one: track_clip with a MaskRound).  A run holds
    either only mask clips or none (ValueError); a run without mask clips makes exactly the calls it made before.

    File clips (Clip.frames a list of paths or bytes) are read a round at a time: a background data.InputPrefetcher reads round
    r + 1 with ``workers`` pool threads (data.default_workers() when None) into one of ``prefetch`` pinned sets while round r
    runs.  ``decode="host"``: Pillow decodes on those threads and the round runs as it does from arrays.  ``decode="device"``:
    the round's files are decoded by ONE ntk_jpeg_decode_batch on a decode stream of this Validation's own, a round ahead of the
    tracker; ntk_track_decode_mask turns off every frame the decoder could not deliver (and every frame of a clip whose starting
    frame it could not), the tracker and the scores take the device tensors and the masked ``active``.  The two streams are
    ordered by events alone ("set k decoded", "set k consumed"); the only host wait is the prefetcher's, for the uploads from
    the pinned set it is about to refill.  ``finish()`` reads the per-clip decode table once: ``on_undecoded="raise"`` raises
    NtkError naming the first undecodable file, ``"skip"`` leaves it at the report (``decode_report``, and ``"decode"`` in
    validate's result).  A frame size holds either only file clips or none; array and callable clips run the code they always
    ran, whatever ``decode`` says."""

    def __init__(self, make_tracker, clips, B, T, iou_thresholds=None, dist_thresholds=None, return_regions=False, device="cuda",
                 protocol="one_pass", skip=5, burn_in=10, failure_overlap=None, decode="host", prefetch=2, workers=None,
                 on_undecoded="raise", spacing=50, anchors=None, patience=10, eao_interval=(115, 755)):
        import torch
        from . import data
        if protocol not in PROTOCOLS:
            raise ValueError("Validation: protocol %r; one of %s" % (protocol, ", ".join(PROTOCOLS)))
        if failure_overlap is None:                     # the supervised protocol's 0, the multi-start protocol's 0.1
            failure_overlap = 0.1 if protocol == "multistart" else 0.0
        self.runs = self.source_clips = self.multistart = None
        if protocol == "multistart":
            lo, hi = (int(v) for v in eao_interval)
            if int(spacing) < 1 or int(patience) < 0 or not 0 <= float(failure_overlap) < 1 or lo < 1 or hi < lo:
                raise ValueError("Validation: spacing=%d (>= 1) patience=%d (>= 0) failure_overlap=%g (in [0,1)) eao_interval=(%d, %d) "
                                 "(1 <= lo <= hi)" % (spacing, patience, failure_overlap, lo, hi))
            self.eao_interval = (lo, hi)
            self.source_clips = [_as_clip(c) for c in clips]
            clips, self.runs = multistart_runs(self.source_clips, spacing, anchors)      # from here on a run is a clip
        data._check_decode(decode)
        if on_undecoded not in ON_UNDECODED:
            raise ValueError("Validation: on_undecoded %r; one of %s" % (on_undecoded, ", ".join(ON_UNDECODED)))
        if int(prefetch) < 1:
            raise ValueError("Validation: prefetch=%d; at least 1" % prefetch)
        self.decode, self.prefetch, self.on_undecoded = decode, int(prefetch), on_undecoded
        self.workers = data.default_workers() if workers is None else max(1, int(workers))
        self.protocol = protocol
        self.make_tracker, self.device = make_tracker, torch.device(device)
        self.clips = [_as_clip(c) for c in clips]
        if not self.clips:
            raise ValueError("Validation: no clips")
        self.B, self.T = int(B), int(T)
        is_mask = [isinstance(c.regions, MaskRegions) for c in self.clips]
        self.masks = any(is_mask)
        if self.masks and not all(is_mask):
            raise ValueError("Validation: clips %s have mask regions and clips %s have not: a run holds either only mask clips or none"
                             % ([i for i, m in enumerate(is_mask) if m], [i for i, m in enumerate(is_mask) if not m]))
        if self.masks:
            # ground truth per clip: the MaskRegions themselves; a tracker starts from the bounds of its clip's first mask
            self.polygons = False
            self._gt = [c.regions for c in self.clips]
            self._first = [mask_bounds(g, 0) if len(g) else None for g in self._gt]
        else:
            # ground truth per clip: [L,4], or, as soon as one clip has polygons, [L,16] for every clip (a rectangle clip as 4-gons)
            given = [np.asarray(c.regions, dtype=np.float64) for c in self.clips]
            given = [g if g.ndim == 2 and g.shape[1] != 4 else g.reshape(-1, 4) for g in given]
            self.polygons = any(g.shape[1] != 4 for g in given)
            self._gt = [(rect_polygons(g) if g.shape[1] == 4 else pad_polygons(g)) for g in given] if self.polygons else given
            self._first = [g[0] if g.shape[1] == 4 else polygon_bounds(pad_polygons(g[0])) for g in given]
        self._is_file = [isinstance(c.frames, (list, tuple)) for c in self.clips]
        lengths = [len(g) for g in self._gt]
        for i, c in enumerate(self.clips):
            if self._is_file[i] and len(c.frames) != lengths[i]:
                raise ValueError("clip %d: %d files for %d regions" % (i, len(c.frames), lengths[i]))
        classes = collections.OrderedDict()
        for i, c in enumerate(self.clips):
            classes.setdefault(self._size(i), []).append(i)
        self.classes = [_SizeClass(size, members, lambda m=members: ClipSchedule([lengths[i] for i in m], self.B, self.T))
                        for size, members in classes.items()]
        self._files = _FileDecoding(decode, self.prefetch, self.workers, len(self.clips), self.device)
        for cls in self.classes:
            if not any(self._is_file[i] for i in cls.members):
                cls.source = _ArraySource(cls, self.clips, lengths, self.device)
            elif all(self._is_file[i] for i in cls.members):
                cls.source = (_DeviceFileSource if decode == "device" else _HostFileSource)(cls, self.clips, self._files)
            else:
                raise ValueError("Validation: the %dx%d clips are file clips and others (clips %s): a frame size holds either only "
                                 "file clips or none" % (cls.size + (cls.members,)))
        self.has_files = any(self._is_file)
        self.decode_report = None                       # set by finish() of a run that had file clips
        self.scores = OverlapScores(len(self.clips), iou_thresholds, dist_thresholds, device=self.device)
        self._sup_args = (skip, burn_in, failure_overlap) if protocol == "supervised" else None
        self.supervisor = None                          # made with the first round: it needs the schedule's effective B
        if protocol == "multistart":                    # one table row and one stretch of the trace per run
            first = np.concatenate([[0], np.cumsum([n - 1 for n in lengths])])
            self.multistart = MultiStart(len(self.clips), first, failure_overlap, patience, device=self.device)
        self._keep = [] if return_regions else None     # (device regions [T,B,4], frame_index, active, clip ids) per round
        self._rounds = self._all_rounds()

    # ---- clips
    def _size(self, i):
        c = self.clips[i]
        if c.size is not None:
            return (int(c.size[0]), int(c.size[1]))
        if self._is_file[i]:                            # the header of the first file
            import io
            from PIL import Image
            f = c.frames[0]
            with Image.open(io.BytesIO(bytes(f)) if isinstance(f, (bytes, bytearray, memoryview)) else f) as im:
                return (int(im.size[1]), int(im.size[0]))
        if callable(c.frames):
            return tuple(np.asarray(c.frames()).shape[1:3])    # no size given: decoded for its shape alone and dropped again (pass
                                                               # size= to avoid the second decoding when the clip is scheduled)
        return tuple(np.asarray(c.frames).shape[1:3])

    def _init_region(self, i):
        c = self.clips[i]
        return self._first[i] if c.init is None else np.asarray(c.init, dtype=np.float64).reshape(4)

    # ---- rounds
    def _all_rounds(self):
        for cls in self.classes:
            for rnd in cls.schedule():
                yield cls, rnd

    def step(self):
        nxt = next(self._rounds, None)
        if nxt is None:
            return False
        self._run(*nxt)
        return True

    def _run(self, cls, rnd):
        import torch
        T, B = rnd.active.shape
        ids = cls.ids(rnd)
        inp = cls.source.round(rnd, ids)                # the round's frames, from wherever the class's clips keep them
        # (1) the slots that take a new clip
        if rnd.resets:
            slots = [s for s, _c in rnd.resets]
            regions = np.stack([self._init_region(cls.members[c]) for _s, c in rnd.resets])
            if cls.tracker is None:
                assert slots == list(range(B))          # the first round of a schedule fills every slot, in order
                cls.tracker = self.make_tracker(inp.firsts, regions)
                if self._sup_args is not None:          # one state per frame size (its own B), one table for all
                    cls.supervisor = Supervisor(B, len(self.clips), *self._sup_args, device=self.device)
                    if self.supervisor is None:
                        self.supervisor = cls.supervisor
                    else:
                        cls.supervisor.table = self.supervisor.table
            else:
                cls.tracker.reset(slots, inp.firsts, regions)
            if cls.supervisor is not None:
                cls.supervisor.start(slots)
        # (2) the ground truth of the round: NaN boxes (absent masks) where inactive
        if self.masks:
            d_gt = self._round_masks(rnd, ids)
        else:
            gt = np.full((T, B, POLY_DOUBLES if self.polygons else 4), np.nan, dtype=np.float64)
            for b in range(B):
                n = int(rnd.active[:, b].sum())
                if n:
                    at = rnd.frame_index[:n, b]
                    gt[:n, b] = self._gt[int(ids[b])][at[0]:at[-1] + 1]
            d_gt = _upload(gt, torch.float64, self.device)
        # (3) one pass over the round, (4) one scoring launch
        if cls.supervisor is not None:
            out = cls.tracker.track_clip(inp.frames, active=inp.active, supervisor=cls.supervisor, gt=d_gt, clip_of=inp.d_ids)
        else:
            out = cls.tracker.track_clip(inp.frames, active=inp.active)
            (self.scores if self.multistart is None else self.multistart).add(out, d_gt, inp.d_ids, active=inp.active)
        cls.source.consumed()                           # the round's launches are enqueued
        if self._keep is not None:
            self._keep.append((out, rnd.frame_index, inp.tracked, ids, None if cls.supervisor is None else cls.supervisor.codes))

    def _round_masks(self, rnd, ids):
        """The masks of a round -> MaskRound: a slot's frames are one slice of its clip's counts; two uploads, one
        ntk_track_mask_bounds."""
        blocks = []
        for b in range(rnd.active.shape[1]):
            n = int(rnd.active[:, b].sum())
            if n:
                at = rnd.frame_index[:n, b]
                blocks.append(((b,),) + self._gt[int(ids[b])].cells(int(at[0]), int(at[-1]) + 1))
        return upload_masks(blocks, rnd.active.shape, self.device)

    def close(self):
        """Stops the sources' threads and the reader pool (finish() calls it; a run that is abandoned should)."""
        for cls in self.classes:
            if cls.source is not None:
                cls.source.close()
        self._files.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _decode_report(self):
        """The per-clip decode table, read once -> the ``decode`` part of the result (see validate)."""
        n = len(self.clips)
        table = np.zeros((n, CLIPDEC_HEAD), dtype=np.int64)
        table[:, CLIPDEC_FIRST_FAILED] = -1
        if self._files.table is not None:
            table = self._files.table.cpu().numpy()
        else:                                           # decode="host": a file that could not be decoded raised at its round
            for i in range(n):
                table[i, CLIPDEC_DECODED] = len(self._gt[i]) - 1 if self._is_file[i] else 0
        failed_files = []
        for i in np.nonzero((table[:, CLIPDEC_START_STATUS] != 0) | (table[:, CLIPDEC_FIRST_FAILED] >= 0))[0]:
            start = table[i, CLIPDEC_START_STATUS] != 0
            k = 0 if start else 1 + int(table[i, CLIPDEC_FIRST_FAILED])
            f = self.clips[i].frames[k]
            name = "<clip %d, frame %d>" % (i, k) if isinstance(f, (bytes, bytearray, memoryview)) else str(f)
            failed_files.append((int(i), k, name, int(table[i, CLIPDEC_START_STATUS if start else CLIPDEC_FIRST_STATUS])))
        col = lambda c: table[:, c].copy()
        return {"clips": {"decoded": col(CLIPDEC_DECODED), "failed": col(CLIPDEC_FAILED), "masked": col(CLIPDEC_MASKED),
                          "first_failed": col(CLIPDEC_FIRST_FAILED), "first_status": col(CLIPDEC_FIRST_STATUS),
                          "start_status": col(CLIPDEC_START_STATUS)},
                "decoded": int(table[:, CLIPDEC_DECODED].sum()), "failed": int(table[:, CLIPDEC_FAILED].sum()),
                "masked": int(table[:, CLIPDEC_MASKED].sum()),
                "clips_affected": len(failed_files), "frames_on_device": self._files.frames_on_device,
                "frames_on_host": self._files.frames_on_host,
                "failed_files": [name for _i, _k, name, _s in failed_files], "_first": failed_files[:1]}

    def finish(self):
        """Runs the remaining rounds; then asks every tracker that can tell (BatchDNCTracker.check) whether a launch failed.  A
        run with file clips then reads the decode table (once; ``decode_report``) and, with on_undecoded="raise", raises NtkError
        naming the first undecodable file of the first affected clip."""
        try:
            while self.step():
                pass
        finally:
            self.close()
        for cls in self.classes:
            if cls.tracker is not None and hasattr(cls.tracker, "check"):
                cls.tracker.check()
        if self.has_files and self.decode_report is None:
            report = self._decode_report()
            first = report.pop("_first")
            self.decode_report = report
            if first and self.on_undecoded == "raise":
                from . import _lib, data
                i, k, name, status = first[0]
                raise _lib.NtkError("device JPEG decode of %s (clip %d, frame %d) failed: %s (status %d); %d clip(s) affected"
                                    % (name, i, k, data.JPEG_STATUS.get(status, "unknown"), status, report["clips_affected"]))
        return self

    def regions(self):
        """The tracked regions per clip, a list of [L-1,4] float64 host arrays in the caller's clip order (synchronises)."""
        if self._keep is None:
            raise ValueError("Validation: made without return_regions=True")
        out = [np.full((len(g) - 1, 4), np.nan) for g in self._gt]
        for host, codes, frame_index, ids, cells in self._kept(regions=True):
            for t, b in cells:
                if codes is None or codes[t, b] != SUP_CODE_SKIPPED:
                    out[int(ids[b])][frame_index[t, b] - 1] = host[t, b]
        return out

    def _kept(self, regions):
        """Per kept round -> (the tracked regions [T,B,4] when `regions` is set, the supervisor's codes [T,B] or None, frame_index,
        clip ids, the tracked cells (t, b)): the device tensors as host arrays (synchronises)."""
        for dev, frame_index, tracked, ids, codes in self._keep:
            host = dev.cpu().numpy() if regions else None
            tracked = tracked if isinstance(tracked, np.ndarray) else tracked.cpu().numpy()    # a mask the device decided
            yield host, None if codes is None else codes.cpu().numpy(), frame_index, ids, list(zip(*np.nonzero(tracked)))

    def codes(self):
        """protocol="supervised": what each clip's slot did on each tracked frame, a list of [L-1] int8 host arrays beside
        ``regions()`` (SUP_CODE_*: 0 tracked, 1 restarted from the ground truth, 2 failure, 3 sat out; the region of a restart
        frame is the ground truth it was started with, that of a skipped frame NaN) -- together what a VOT trajectory file holds.
        Synchronises."""
        if self._keep is None or self.protocol != "supervised":
            raise ValueError("Validation: codes() needs protocol=\"supervised\" and return_regions=True")
        out = [np.full((len(g) - 1,), SUP_CODE_INACTIVE, dtype=np.int8) for g in self._gt]
        for _host, codes, frame_index, ids, cells in self._kept(regions=False):
            for t, b in cells:
                out[int(ids[b])][frame_index[t, b] - 1] = codes[t, b]
        return out


def validate(make_tracker, clips, B, T, return_regions=False, **kw):
    """Validation(...) run to its end -> scores.result(), or (result, regions per clip) with return_regions=True.  With
    protocol="supervised" (and skip=, burn_in=, failure_overlap=) the result is the supervisor's (summarize_supervised) and
    return_regions=True gives (result, regions per clip, codes per clip).  With protocol="multistart" (and spacing=, anchors=,
    failure_overlap=, patience=, eao_interval=) the result is summarize_multistart's and the regions are per RUN, in run order.
    decode=, prefetch=, workers=, on_undecoded= go to
    Validation; a run that had file clips gains ``result["decode"]``: ``clips`` (per clip ``decoded``, ``failed``, ``masked``,
    ``first_failed``, ``first_status``, ``start_status``: the NTK_CLIPDEC_* row), the totals ``decoded``, ``failed``, ``masked``
    and ``clips_affected``, ``frames_on_device`` / ``frames_on_host`` (files the device / Pillow decoded) and ``failed_files``
    (per affected clip the file that failed first).  Results of runs without file clips keep their keys."""
    v = Validation(make_tracker, clips, B, T, return_regions=return_regions, **kw).finish()
    supervised = v.protocol == "supervised"
    if v.multistart is not None:
        res = v.multistart.result(v.eao_interval, v.runs, len(v.source_clips))
    else:
        res = (v.supervisor if supervised else v.scores).result()
    if v.decode_report is not None:
        res["decode"] = v.decode_report
    if not return_regions:
        return res
    return (res, v.regions()) + ((v.codes(),) if supervised else ())


def write_trajectory(path, first_region, regions, codes=None):
    """Writes the VOT toolkit's trajectory file of one clip.  Line 1 is ``1``, the initialisation frame (the toolkit's format has
    the code there and not the region: ``first_region``, the four numbers the tracker was started with, is checked and not
    written).  Then one line per tracked frame, from ``regions`` [L-1,4] and ``codes`` [L-1] as Validation.regions() and
    Validation.codes() return them: ``1`` on a restart frame, ``2`` on a failure frame, ``0`` on a frame that was sat out, any other
    frame ``x,y,w,h`` with four decimals.  ``codes=None`` is the one-pass run: every line after the first is a region."""
    first = np.asarray(first_region, dtype=np.float64).reshape(-1)
    regions = np.asarray(regions, dtype=np.float64).reshape(-1, 4)
    if first.shape != (4,) or not np.isfinite(first).all():
        raise ValueError("write_trajectory: first_region %s; four finite numbers" % (first.tolist(),))
    if codes is not None and len(codes) != len(regions):
        raise ValueError("write_trajectory: %d codes for %d regions" % (len(codes), len(regions)))
    special = {SUP_CODE_RESTART: "1", SUP_CODE_FAILURE: "2", SUP_CODE_SKIPPED: "0"}
    lines = ["1"]
    for t, r in enumerate(regions):
        code = None if codes is None else special.get(int(codes[t]))
        lines.append(code if code is not None else "%.4f,%.4f,%.4f,%.4f" % tuple(r))
    with open(path, "w") as f:
        f.write("\n".join(lines) + "\n")
