"""The ground truth of validation clips, by kind: a rectangle per frame ([L,4]), a polygon per frame ([L,2P], 3 <= P <= 8: VOT
regions) or a segmentation mask per frame (MaskRegions: the run-length coded masks of the VOT sets from 2020 on).  A leaf of the
package: NumPy alone at import (torch and the library are imported by the functions that reach the device), imported by data,
scoring, evaluate and online.

  Clip               one clip of a validation set: frames, regions, init, size
  pad_polygons, rect_polygons, polygon_bounds        polygons in the device layout (include/ntmtrack.h NTK_POLY_*) and the host's
                     ntk_track_poly_bounds
  MaskRegions, mask_bounds       a clip's masks as the toolkit writes them (NTK_MASK_*) and the host's ntk_track_mask_bounds
  RectTruth, PolyTruth, MaskTruth    a clip's ground truth on the host, one class per kind with one interface (as_truth picks it):
                     len, first() (what the tracker starts from), present(), take(order), round(...) -> the round's on the device
  RectRound, PolyRound, MaskRound    a round's ground truth on the device (or one frame of it), one class per kind with one
                     interface (as_round_truth picks it): suffix (of the entry points that score the kind), rects (what a restart
                     starts from), [t], scoring_pointers / plan_pointers / judge_pointers, after_pass
  upload_masks       mask blocks -> MaskRound: two uploads and ONE ntk_track_mask_bounds

The score kernels (track_scores.hip) are one template family over the kind of ground truth; these classes are its mirror: a
caller names no kind, it asks the object.
"""
import collections

import numpy as np

# include/ntmtrack.h NTK_POLY_*: a polygon region is POLY_DOUBLES doubles, the leading finite pairs its vertices, NaN after them
POLY_MAX_POINTS, POLY_DOUBLES = 8, 16
# include/ntmtrack.h NTK_MASK_*: a mask is (x0, y0, w, h, first, count) over a flat array of counts; its overlap (|M n R|, |R|, |M|)
MASK_CELL_INTS, MASK_OVERLAP_DOUBLES, MASK_MAX_PIXELS = 6, 3, 1 << 30

#: one clip of a validation set.  frames: [L,H,W,3] uint8 or float host array, or a callable returning one (called when the clip is
#: scheduled), or a list / tuple of L image files (paths, or the files' bytes): a FILE CLIP, read a round at a time and never held
#: whole (size may then be None: it is read from the first file's header).  regions: [L,4] ground truth (x, y, w, h) in pixels,
#: row 0 starts the tracker; or [L,2P] polygons (x0, y0, x1, y1, ...) of 3 <= P <= 8 vertices, rows with fewer padded with NaN,
#: the tracker then starts from row 0's bounding rectangle; or a MaskRegions (a segmentation mask per frame), the tracker then
#: starts from the bounds of frame 0's set pixels.  init: the region the tracker is started with when it is not that (the
#: reference passes it normalised).  size: (H, W) where frames is a callable, so that clips can be grouped by frame size without
#: decoding them.
Clip = collections.namedtuple("Clip", ["frames", "regions", "init", "size"])
Clip.__new__.__defaults__ = (None, None)


def _as_clip(c):
    if isinstance(c, Clip):
        return c
    if isinstance(c, dict):
        return Clip(c["frames"], c["regions"], c.get("init"), c.get("size"))
    if isinstance(c, (tuple, list)):
        return Clip(*c)
    return Clip(c.frames, c.regions, getattr(c, "init", None), getattr(c, "size", None))


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


# ---- a clip's ground truth on the host: one class per kind ----------------------------------------------------------------------

class RectTruth(object):
    """A rectangle per frame: ``regions`` float64 [L,4] (x, y, w, h) in pixels.  The interface of the three kinds: ``len``;
    ``first()`` the [4] rectangle a tracker starts from; ``present()`` bool [L], by the rule the score kernels use for the kind;
    ``take(order)`` the same kind with the frames in another order; ``round(rnd, ids, truths, device)`` (of the class) the
    ground truth of a round on the device, NaN rectangles (absent objects) where a cell is inactive: ``rnd`` a Round of the
    schedule, whose ``slices()`` name the frames of every slot, ``ids`` [B] the slots' indices into ``truths``."""
    width = 4

    def __init__(self, regions):
        self.regions = np.asarray(regions, dtype=np.float64).reshape(-1, self.width)

    def __len__(self):
        return len(self.regions)

    def first(self):
        return self.regions[0]

    def present(self):
        g = self.regions
        with np.errstate(invalid="ignore"):
            return np.isfinite(g).all(axis=1) & (g[:, 2] > 0) & (g[:, 3] > 0)

    def take(self, order):
        return type(self)(self.regions[order])

    def as_polygons(self):
        """The rectangles as 4-gons (a set in which one clip has polygons is scored as polygons); the start stays row 0."""
        return PolyTruth(rect_polygons(self.regions), first=self.first())

    @classmethod
    def round(cls, rnd, ids, truths, device):
        import torch
        from . import _lib
        gt = np.full(tuple(rnd.active.shape) + (cls.width,), np.nan, dtype=np.float64)
        for b, lo, hi in rnd.slices():
            gt[:hi - lo, b] = truths[int(ids[b])].regions[lo:hi]
        return cls.Round(_lib.upload(gt, torch.float64, device))


class PolyTruth(RectTruth):
    """A polygon per frame: ``regions`` float64 [L,POLY_DOUBLES], from [L,2P] padded with NaN.  The tracker starts from row 0's
    bounding rectangle (or ``first``, where the polygons were made from rectangles)."""
    width = POLY_DOUBLES

    def __init__(self, regions, first=None):
        self.regions, self._first = pad_polygons(regions).reshape(-1, POLY_DOUBLES), first

    def first(self):
        return polygon_bounds(self.regions[0]) if self._first is None else self._first

    def present(self):
        return np.isfinite(polygon_bounds(self.regions)).all(axis=1)

    def as_polygons(self):
        return self


class MaskTruth(object):
    """A segmentation mask per frame: ``regions`` a MaskRegions.  The tracker starts from the bounds of frame 0's set pixels."""

    def __init__(self, regions):
        self.regions = regions

    def __len__(self):
        return len(self.regions)

    def first(self):
        return mask_bounds(self.regions, 0) if len(self.regions) else None

    def present(self):
        return np.isfinite(mask_bounds(self.regions)).all(axis=1)

    def take(self, order):
        return MaskTruth(self.regions.take(order))

    @classmethod
    def round(cls, rnd, ids, truths, device):
        """A slot's frames are one slice of its clip's counts; two uploads, one ntk_track_mask_bounds."""
        blocks = (((b,),) + truths[int(ids[b])].regions.cells(lo, hi) for b, lo, hi in rnd.slices())
        return upload_masks(blocks, rnd.active.shape, device)


def as_truth(regions):
    """A clip's regions as given -- [L,4], [L,2P] or a MaskRegions -> RectTruth, PolyTruth or MaskTruth."""
    if isinstance(regions, MaskRegions):
        return MaskTruth(regions)
    g = np.asarray(regions, dtype=np.float64)
    return PolyTruth(g) if g.ndim == 2 and g.shape[1] != 4 else RectTruth(g)


def regions_present(regions):
    """bool [L]: the frames of a clip whose ground truth is present, by the rule the score kernels use for its kind: a rectangle
    finite with w > 0 and h > 0, a polygon with a bounding rectangle (polygon_bounds), a mask with set pixels (mask_bounds)."""
    return as_truth(regions).present()


# ---- a round's ground truth on the device: one class per kind ------------------------------------------------------------------

class RectRound(object):
    """The rectangles of a round on the device, ``gt`` float64 [T,B,4], or of one of its frames, [B,4].  The interface of the
    three kinds: ``suffix`` of the entry points that score the kind; ``shape`` (T, B) or (B,); ``rects`` [..., 4], what a restart
    starts from (here the ground truth itself: the same storage); ``round[t]`` frame t (views: nothing is copied);
    ``scoring_pointers(regions)`` what a [T,B] scoring entry point takes after ``regions``; ``plan_pointers()`` and
    ``judge_pointers()`` what ntk_track_supervise* takes there in its two phases; ``after_pass(regions)`` what a supervised
    frame runs between its pass and judge."""
    suffix = ""

    def __init__(self, gt):
        self.gt, self.shape = gt, tuple(gt.shape[:-1])

    @property
    def rects(self):
        return self.gt

    def __getitem__(self, t):
        return type(self)(self.gt[t])

    def scoring_pointers(self, regions):
        from . import _lib
        return (_lib.ptr(self.gt),)

    def plan_pointers(self):
        return self.scoring_pointers(None)

    judge_pointers = plan_pointers

    def after_pass(self, regions):
        pass


class PolyRound(RectRound):
    """The polygons of a round on the device, ``gt`` float64 [T,B,POLY_DOUBLES] or [B,POLY_DOUBLES].  ``rects`` are the polygons'
    bounding rectangles: ONE ntk_track_poly_bounds over all of ``gt`` at the first use, so a protocol that restarts nothing
    never launches it."""
    suffix = "_poly"
    _rects = None

    @property
    def rects(self):
        if self._rects is None:
            import torch
            from . import _lib
            self._rects = torch.empty(self.shape + (4,), dtype=torch.float64, device=self.gt.device)
            _lib.check(_lib.lib().ntk_track_poly_bounds(_lib.ptr(self.gt), self.gt.numel() // POLY_DOUBLES, _lib.ptr(self._rects),
                                                        _lib.stream()), "ntk_track_poly_bounds")
        return self._rects


class MaskRound(object):
    """The mask ground truth of a round (or of one of its frames) on the device: ``cells`` int32 [T,B,MASK_CELL_INTS] (or [B,...])
    and ``rle`` int32 with ``n_rle`` counts as ntk_track_mask_* take them; ``rects`` float64 [T,B,4] and ``area`` [T,B] as
    ntk_track_mask_bounds left them; ``overlap`` float64 [..., MASK_OVERLAP_DOUBLES], set by whoever ran ntk_track_mask_overlaps
    on the tracked regions.  ``round[t]`` is frame t (views: nothing is copied).  RectRound's interface: the entry points take
    the rectangles and the overlap, which scoring_pointers computes for the round and after_pass for a frame."""
    suffix = "_mask"

    def __init__(self, cells, rle, n_rle, rects, area, overlap=None):
        self.cells, self.rle, self.n_rle, self.rects, self.area, self.overlap = cells, rle, int(n_rle), rects, area, overlap
        self.shape = tuple(cells.shape[:-1])

    def __getitem__(self, t):
        """Frame t.  Its ``overlap`` is a view of the round's, which is made with the first frame taken: what after_pass leaves
        in the frames is the round's ``overlap`` afterwards."""
        if self.overlap is None:
            import torch
            self.overlap = torch.empty(self.shape + (MASK_OVERLAP_DOUBLES,), dtype=torch.float64, device=self.cells.device)
        return MaskRound(self.cells[t], self.rle, self.n_rle, self.rects[t], self.area[t], self.overlap[t])

    def overlaps(self, regions, out=None):
        """One ntk_track_mask_overlaps of regions float64 [..., 4] (device) against these masks -> ``overlap`` (also kept)."""
        import torch
        from . import _lib
        n = self.cells.numel() // MASK_CELL_INTS
        if out is None:
            out = torch.empty(self.shape + (MASK_OVERLAP_DOUBLES,), dtype=torch.float64, device=self.cells.device)
        if (regions.dtype != torch.float64 or regions.numel() != 4 * n or out.numel() != MASK_OVERLAP_DOUBLES * n
                or self.cells.dtype != torch.int32 or self.rle.dtype != torch.int32 or self.rle.numel() < max(self.n_rle, 1)):
            raise _lib.NtkError("MaskRound.overlaps: regions %s for %d masks" % (tuple(regions.shape), n))
        P = _lib.ptr
        _lib.check(_lib.lib().ntk_track_mask_overlaps(P(regions), P(self.cells), P(self.rle), self.n_rle, n, P(out), _lib.stream()),
                   "ntk_track_mask_overlaps")
        self.overlap = out
        return out

    def scoring_pointers(self, regions):
        from . import _lib
        return _lib.ptr(self.rects), _lib.ptr(self.overlaps(regions))

    def plan_pointers(self):
        from . import _lib
        return _lib.ptr(self.rects), None

    def judge_pointers(self):
        import torch
        from . import _lib
        want = self.shape + (MASK_OVERLAP_DOUBLES,)
        if not torch.is_tensor(self.overlap) or self.overlap.dtype != torch.float64 or tuple(self.overlap.shape) != want:
            raise _lib.NtkError("Supervisor: judge needs the masks' overlap, a float64 tensor of shape %s" % (want,))
        return _lib.ptr(self.rects), _lib.ptr(self.overlap)

    def after_pass(self, regions):
        self.overlaps(regions, out=self.overlap)


RectTruth.Round, PolyTruth.Round = RectRound, PolyRound


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
    d_cells, d_rle = _lib.upload(cells, torch.int32, device), _lib.upload(rle, torch.int32, device)
    rects = torch.empty(tuple(shape) + (4,), dtype=torch.float64, device=d_cells.device)
    area = torch.empty(tuple(shape), dtype=torch.float64, device=d_cells.device)
    P = _lib.ptr
    _lib.check(_lib.lib().ntk_track_mask_bounds(P(d_cells), P(d_rle), n_rle, cells.size // MASK_CELL_INTS, P(rects), P(area),
                                                _lib.stream()), "ntk_track_mask_bounds")
    return MaskRound(d_cells, d_rle, n_rle, rects, area)


def as_round_truth(gt, device, who, shape=None, upload=False):
    """What the callers of the score tables, of the supervisor and of track_clip pass as a round's (or a frame's) ground truth ->
    RectRound, PolyRound or MaskRound, checked.  A float64 [T,B,4], [B,4], [T,B,POLY_DOUBLES] or [B,POLY_DOUBLES] device tensor
    is wrapped as it is (never copied); with ``upload`` a host array (or a tensor of another type) goes up through the pinned
    asynchronous copy.  ``shape``: the (T, B) or (B,) the caller needs, checked when given."""
    import torch
    from . import _lib
    if not isinstance(gt, (RectRound, MaskRound)):
        if upload:
            gt = _lib.on_device(gt, torch.float64, device)
        if not (torch.is_tensor(gt) and gt.dtype == torch.float64 and gt.is_contiguous() and gt.dim() in (2, 3)
                and gt.shape[-1] in (4, POLY_DOUBLES)):
            raise _lib.NtkError("%s: gt must be a contiguous float64 device tensor [T,B,4] or [T,B,%d] (or a frame of one: [B,4], "
                                "[B,%d]) or a MaskRound, not %s" % (who, POLY_DOUBLES, POLY_DOUBLES, tuple(gt.shape) if
                                                                    torch.is_tensor(gt) else type(gt).__name__))
        gt = (PolyRound if gt.shape[-1] == POLY_DOUBLES else RectRound)(gt)
    elif isinstance(gt, MaskRound) and not (gt.rects.dtype == torch.float64 and gt.rects.is_contiguous() and gt.cells.is_contiguous()
                                            and tuple(gt.rects.shape) == gt.shape + (4,)):
        raise _lib.NtkError("%s: a MaskRound of %s masks needs contiguous cells and contiguous float64 rects %s on the device"
                            % (who, gt.shape, gt.shape + (4,)))
    if shape is not None and gt.shape != tuple(shape):
        raise _lib.NtkError("%s: the ground truth is of %s cells; expected %s" % (who, gt.shape, tuple(shape)))
    return gt
