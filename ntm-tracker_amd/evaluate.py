"""Validation over clips on the device: the reference's validate_tracker.py:26-38 (one NTMTracker per clip, one frame at a time,
nothing scored) as continuous batching over B slots of a BatchNTMTracker / BatchDNCTracker, with the scores of every clip
accumulated in one device table that is read back once, at the end.  This module is the driver; the ground truth by kind
(rectangles, polygons, masks) lives in regions, the tables by protocol in scoring, and every name of theirs that callers know as
``evaluate.X`` is re-exported below.

  ClipSchedule   which clip sits in which slot in which round (host arithmetic only: no torch, no device); a Round's
                 ``slices()`` name the frames of every slot, for the frames and the ground truth alike
  Validation     the driver: per round the resets, ONE track_clip and ONE scoring launch, no host synchronisation after the
                 first round of a frame size.  The frames of a round come from the frame size's source: _ArraySource (arrays and
                 callables), _HostFileSource (image files read a round at a time, a round ahead: data.stage_round,
                 data.InputPrefetcher) or _DeviceFileSource (the files decoded on the device on a second stream,
                 ntk_jpeg_decode_batch, ntk_track_decode_mask turning off the frames that could not be decoded); its ground truth
                 from the clips' RectTruth / PolyTruth / MaskTruth; how it is run and scored from the protocol (_OnePass for
                 "one_pass" and "multistart", _Supervised), chosen once
  multistart_runs    the multi-start protocol's runs of a set of clips (host arithmetic only): a run is a clip whose frames are
                 read in another order
  validate       runs a Validation to the end; protocol="one_pass" (the default), "supervised" or "multistart"
  write_trajectory   the toolkit's trajectory file of one clip, from regions() and codes()

A polygon clip is scored as the toolkit scores it -- the polygon against the tracker's rectangle -- while the tracker is started
and restarted from the polygon's bounding rectangle, as the reference's vot.VOT("rectangle") hands it over.  A run without a
polygon clip makes exactly the rectangle calls.  A mask clip is scored straight from the run-length counts against the pixel set
of the tracker's rectangle, while the tracker is started and restarted from the bounds of the set pixels.  A run holds either only
mask clips or none.
"""
import collections

import numpy as np

from .regions import (MASK_CELL_INTS, MASK_MAX_PIXELS, MASK_OVERLAP_DOUBLES, POLY_DOUBLES, POLY_MAX_POINTS,   # noqa: F401
                      Clip, MaskRegions, MaskRound, MaskTruth, PolyRound, PolyTruth, RectRound, RectTruth, _as_clip,
                      as_round_truth, as_truth, mask_bounds, pad_polygons, polygon_bounds, rect_polygons, regions_present,
                      upload_masks)
from .scoring import (MS_FAILED, MS_FRAMES, MS_HEAD, MS_LOW, MS_PENDING, MS_SUM_IOU, MS_TRACKED, SCORE_FIRST_LOST,   # noqa: F401
                      SCORE_FRAMES, SCORE_HEAD, SCORE_LOST, SCORE_MAX_THRESHOLDS, SCORE_SUM_DIST, SCORE_SUM_IOU,
                      SUP_CODE_FAILURE, SUP_CODE_INACTIVE, SUP_CODE_RESTART, SUP_CODE_SKIPPED, SUP_CODE_TRACKED, SUP_FAILURES,
                      SUP_FIRST_FAILURE, SUP_HEAD, SUP_JUDGE, SUP_MODE_TRACK, SUP_MODE_WAIT, SUP_PLAN, SUP_RESTARTS, SUP_SKIPPED,
                      SUP_STATE_COUNTDOWN, SUP_STATE_INTS, SUP_STATE_MODE, SUP_STATE_SINCE, SUP_SUM_IOU, SUP_TRACKED, SUP_VALID,
                      MultiStart, OverlapScores, Supervisor, summarize, summarize_multistart, summarize_supervised)

PROTOCOLS = ("one_pass", "supervised", "multistart")
# include/ntmtrack.h NTK_CLIPDEC_*: the per-clip row of ntk_track_decode_mask (validation from files decoded on the device)
CLIPDEC_DECODED, CLIPDEC_FAILED, CLIPDEC_MASKED, CLIPDEC_FIRST_FAILED, CLIPDEC_FIRST_STATUS, CLIPDEC_START_STATUS, CLIPDEC_HEAD = \
    0, 1, 2, 3, 4, 5, 6
ON_UNDECODED = ("raise", "skip")


class Round(collections.namedtuple("Round", ["resets", "frame_index", "active", "clip_of"])):
    """One round of a ClipSchedule (see there)."""
    __slots__ = ()

    def slices(self):
        """(b, lo, hi) for every slot b with active frames: at t = 0 ... hi - lo - 1 it tracks frames lo ... hi - 1 of its clip."""
        for b in range(self.active.shape[1]):
            n = int(self.active[:, b].sum())
            if n:
                lo = int(self.frame_index[0, b])
                yield b, lo, lo + n


def _upload(array, dtype, device):
    """_lib.upload (host array -> device tensor through a pinned asynchronous copy: no synchronisation), imported at its first
    use: this module stays importable without torch."""
    from ._lib import upload
    return upload(array, dtype, device)


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
    per run with the run's frames and regions in run order (polygons in the padded [L,16] layout).

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
        truth = as_truth(c.regions)
        present = truth.present()
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
        for a, step in starts:
            order = np.arange(a, L) if step > 0 else np.arange(a, -1, -1)
            cut = slice(a, None) if step > 0 else slice(a, None, -1)
            if shared is not None:
                frames = lambda shared=shared, cut=cut: shared.frames()[cut]
            elif isinstance(c.frames, (list, tuple)):
                frames = [c.frames[k] for k in order]
            else:
                frames = np.asarray(c.frames)[cut]
            run_clips.append(Clip(frames, truth.take(order).regions, c.init if (a, step) == (0, 1) else None, c.size))
            runs.append((i, a, step, len(order)))
    if not runs:
        raise ValueError("multistart_runs: the %d clip(s) yield no run" % len(clips))
    return run_clips, np.asarray(runs, dtype=np.int64).reshape(-1, 4)


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
        for b, lo, hi in rnd.slices():
            frames[:hi - lo, b] = held[b][lo:hi]
            if hi == self.lengths[int(ids[b])]:
                del self.held[int(ids[b])]              # the clip has ended
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


class _FileSource(_Source):
    """What the two sources of a size class of file clips share: a data.InputPrefetcher (made with the first round) stages round
    r + 1 while round r runs."""

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

    def close(self):
        if self.prefetcher is not None:
            self.prefetcher.close()


class _HostFileSource(_FileSource):
    """The files decoded by Pillow on the prefetcher's threads; the pinned block goes up as it is, as track_clip would upload
    it."""

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


class _DeviceFileSource(_FileSource):
    """The same files decoded on the device: ONE ntk_jpeg_decode_batch per round on the shared decode stream, a round ahead of
    the tracker, and ntk_track_decode_mask on the tracking stream.  The two streams are ordered by events alone: "set k decoded"
    and "set k consumed" (the tracking stream has read the set's device buffers: the decode stream may write them again)."""

    def __init__(self, cls, clips, shared):
        _FileSource.__init__(self, cls, clips, shared)
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


class _OnePass(object):
    """The protocols that track a round and then score it: one track_clip, one ``table.add`` (an OverlapScores for "one_pass", a
    MultiStart for "multistart"), nothing per slot.  ``run`` -> (the tracked regions [T,B,4], the per-frame codes: none)."""
    supervisor = None

    def __init__(self, table, *result_args):
        self.table, self.result_args = table, result_args

    def started(self, cls, slots, B):
        pass

    def run(self, cls, inp, truth):
        out = cls.tracker.track_clip(inp.frames, active=inp.active)
        self.table.add(out, truth, inp.d_ids, active=inp.active)
        return out, None

    def result(self):
        return self.table.result(*self.result_args)


class _Supervised(object):
    """protocol="supervised": a round is one track_clip with the size class's Supervisor, which is made with the class's first
    round (it needs the schedule's effective B): one state per frame size, one table for all -- that of ``supervisor``, the
    first one made."""

    def __init__(self, n_clips, skip, burn_in, failure_overlap, device):
        self.args, self.device, self.supervisor = (n_clips, skip, burn_in, failure_overlap), device, None

    def started(self, cls, slots, B):
        if cls.supervisor is None:
            cls.supervisor = Supervisor(B, *self.args, device=self.device)
            if self.supervisor is None:
                self.supervisor = cls.supervisor
            else:
                cls.supervisor.table = self.supervisor.table
        cls.supervisor.start(slots)

    def run(self, cls, inp, truth):
        out = cls.tracker.track_clip(inp.frames, active=inp.active, supervisor=cls.supervisor, gt=truth, clip_of=inp.d_ids)
        return out, cls.supervisor.codes

    def result(self):
        return self.supervisor.result()


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
        # the ground truth per clip, of ONE kind for the set: masks for every clip or for none; as soon as one clip has polygons,
        # polygons for every clip (a rectangle clip as 4-gons, started from its rectangle as before)
        truths = [as_truth(c.regions) for c in self.clips]
        is_mask = [type(t) is MaskTruth for t in truths]
        self.masks = any(is_mask)
        if self.masks and not all(is_mask):
            raise ValueError("Validation: clips %s have mask regions and clips %s have not: a run holds either only mask clips or none"
                             % ([i for i, m in enumerate(is_mask) if m], [i for i, m in enumerate(is_mask) if not m]))
        self.polygons = any(type(t) is PolyTruth for t in truths)
        self._truth = [t.as_polygons() for t in truths] if self.polygons else truths
        self._gt = [t.regions for t in self._truth]     # what they hold: [L,4] or [L,16] arrays, or the MaskRegions
        self._is_file = [isinstance(c.frames, (list, tuple)) for c in self.clips]
        lengths = [len(t) for t in self._truth]
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
        if protocol == "supervised":
            self._protocol = _Supervised(len(self.clips), skip, burn_in, failure_overlap, self.device)
        elif protocol == "multistart":                  # one table row and one stretch of the trace per run
            first = np.concatenate([[0], np.cumsum([n - 1 for n in lengths])])
            self.multistart = MultiStart(len(self.clips), first, failure_overlap, patience, device=self.device)
            self._protocol = _OnePass(self.multistart, self.eao_interval, self.runs, len(self.source_clips))
        else:
            self._protocol = _OnePass(self.scores)
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
        return self._truth[i].first() if c.init is None else np.asarray(c.init, dtype=np.float64).reshape(4)

    @property
    def supervisor(self):
        """protocol="supervised": the Supervisor whose table the run fills (made with the first round), else None."""
        return self._protocol.supervisor

    def result(self):
        """The protocol's result: OverlapScores.result(), Supervisor.result() or MultiStart.result() over the runs."""
        return self._protocol.result()

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
        B = rnd.active.shape[1]
        ids = cls.ids(rnd)
        inp = cls.source.round(rnd, ids)                # the round's frames, from wherever the class's clips keep them
        # (1) the slots that take a new clip
        if rnd.resets:
            slots = [s for s, _c in rnd.resets]
            regions = np.stack([self._init_region(cls.members[c]) for _s, c in rnd.resets])
            if cls.tracker is None:
                assert slots == list(range(B))          # the first round of a schedule fills every slot, in order
                cls.tracker = self.make_tracker(inp.firsts, regions)
            else:
                cls.tracker.reset(slots, inp.firsts, regions)
            self._protocol.started(cls, slots, B)
        # (2) the ground truth of the round: NaN boxes (absent masks) where inactive
        truth = type(self._truth[0]).round(rnd, ids, self._truth, self.device)
        # (3) one pass over the round and (4) one scoring launch, as the protocol has it
        out, codes = self._protocol.run(cls, inp, truth)
        cls.source.consumed()                           # the round's launches are enqueued
        if self._keep is not None:
            self._keep.append((out, rnd.frame_index, inp.tracked, ids, codes))

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
    res = v.result()
    if v.decode_report is not None:
        res["decode"] = v.decode_report
    if not return_regions:
        return res
    return (res, v.regions()) + ((v.codes(),) if v.protocol == "supervised" else ())


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
