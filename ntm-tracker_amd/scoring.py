"""The score tables of validation on the device, one per protocol, and the host arithmetic of their read-outs.  NumPy alone at
import: torch and the library are imported by the functions that reach the device.

  OverlapScores  the one-pass protocol: the per-clip table (ntk_track_overlap_scores) and its one synchronising read-out
  Supervisor     the supervised protocol (a lost tracker is restarted from the ground truth): per-slot state and per-clip table
                 on the device (ntk_track_supervise), decided frame by frame without a read-back
  MultiStart     the multi-start protocol's run table and overlap trace (ntk_track_multistart) and the EAO reduction
                 (ntk_track_eao_curve)
  summarize, summarize_supervised, summarize_multistart     table -> result dict

The ground truth a table scores against is a regions.RectRound, PolyRound or MaskRound (what the callers pass -- tensors, host
arrays, a MaskRound -- goes through regions.as_round_truth): it names the entry point's suffix and hands over its pointers, so
nothing here asks for its kind.

The overlap is the VOT / OTB one on real-valued rectangles.  The reference's own bb_iou (test_tracker.py:59-83) is never called
there, uses a +1 pixel convention and does not clamp an empty intersection: it is not the model here.
"""
import numpy as np

from .regions import as_round_truth

# row layout of the score table: include/ntmtrack.h NTK_SCORE_*
SCORE_FRAMES, SCORE_SUM_IOU, SCORE_SUM_DIST, SCORE_LOST, SCORE_FIRST_LOST, SCORE_HEAD = 0, 1, 2, 3, 4, 5
SCORE_MAX_THRESHOLDS = 256

# include/ntmtrack.h NTK_SUP_*: the supervised protocol's table row, slot state, modes, phases and per-frame codes
SUP_VALID, SUP_SUM_IOU, SUP_FAILURES, SUP_RESTARTS, SUP_TRACKED, SUP_SKIPPED, SUP_FIRST_FAILURE, SUP_HEAD = 0, 1, 2, 3, 4, 5, 6, 7
SUP_STATE_MODE, SUP_STATE_COUNTDOWN, SUP_STATE_SINCE, SUP_STATE_INTS = 0, 1, 2, 3
SUP_MODE_TRACK, SUP_MODE_WAIT = 0, 1
SUP_PLAN, SUP_JUDGE = 0, 1
SUP_CODE_INACTIVE, SUP_CODE_TRACKED, SUP_CODE_RESTART, SUP_CODE_FAILURE, SUP_CODE_SKIPPED = -1, 0, 1, 2, 3
# include/ntmtrack.h NTK_MS_*: the multi-start protocol's table row, one per run
MS_FRAMES, MS_TRACKED, MS_SUM_IOU, MS_FAILED, MS_LOW, MS_PENDING, MS_HEAD = 0, 1, 2, 3, 4, 5, 6


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


def _scoring_call(who, device, regions, gt, clip_of, active, frame_iou):
    """What OverlapScores.add and MultiStart.add share: the arguments of one scoring launch over a round, checked and on the device
    (tensors there are taken as they are, host arrays go up through the pinned asynchronous copy).  -> (regions [T,B,4] or [B,4],
    the ground truth as a RectRound, PolyRound or MaskRound, active [T,B] or None, clip_of [B], T, B, the frame_iou buffer or
    None)."""
    import torch
    from . import _lib
    regions = _lib.on_device(regions, torch.float64, device)
    truth = as_round_truth(gt, device, who, upload=True)
    if regions.dim() not in (2, 3) or regions.shape[-1] != 4 or truth.shape != tuple(regions.shape[:-1]):
        raise _lib.NtkError("%s: regions %s must be [T,B,4] (or [B,4]) and the ground truth, of %s cells, of the same [T,B]"
                            % (who, tuple(regions.shape), truth.shape))
    T, B = (1,) * (3 - regions.dim()) + truth.shape
    clip_of = _lib.on_device(clip_of, torch.int32, device)
    mask = None if active is None else _lib.on_device(active, torch.uint8, device).reshape(-1, B)
    if tuple(clip_of.shape) != (B,) or (mask is not None and tuple(mask.shape) != (T, B)):
        raise _lib.NtkError("%s: clip_of %s / active %s for [T,B] = [%d,%d]"
                            % (who, tuple(clip_of.shape), None if mask is None else tuple(mask.shape), T, B))
    out = torch.empty((T, B), dtype=torch.float64, device=device) if frame_iou else None
    return regions, truth, mask, clip_of, T, B, out


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
        regions, truth, mask, clip_of, T, B, out = _scoring_call("OverlapScores.add", self.device, regions, gt, clip_of, active,
                                                                 frame_iou)
        name = "ntk_track_overlap_scores" + truth.suffix
        _lib.check(getattr(_lib.lib(), name)(P(regions), *truth.scoring_pointers(regions), P(mask), P(clip_of), T, B, self.n_clips,
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
        from . import _lib
        slots = [int(s) for s in slots]
        if not all(0 <= s < self.B for s in slots):
            raise ValueError("Supervisor.start: slots %s outside [0,%d)" % (slots, self.B))
        if slots:
            self.state.index_fill_(0, _lib.upload(np.asarray(slots), torch.int64, self.device), 0)

    def _call(self, phase, regions, truth, pointers, active, clip_of, codes, frame_iou):
        import torch
        from . import _lib
        for name, t, dtype, shape in (("regions", regions, torch.float64, (self.B, 4)), ("active", active, torch.uint8, (self.B,)),
                                      ("clip_of", clip_of, torch.int32, (self.B,)), ("codes", codes, torch.int8, (self.B,)),
                                      ("frame_iou", frame_iou, torch.float64, (self.B,))):
            if t is not None and (not torch.is_tensor(t) or t.dtype != dtype or tuple(t.shape) != shape):
                raise _lib.NtkError("Supervisor: %s must be a %s tensor of shape %s" % (name, dtype, shape))
        P = _lib.ptr
        fn = "ntk_track_supervise" + truth.suffix
        _lib.check(getattr(_lib.lib(), fn)(phase, P(regions), *pointers, P(active), P(clip_of), self.B, self.n_clips, self.skip,
                                           self.burn_in, self.failure_overlap, P(self.state), P(self.table), P(self.track),
                                           P(self.restart), P(codes), P(frame_iou), _lib.stream()), fn)

    def plan(self, gt_t, active_t, clip_of, codes=None, frame_iou=None):
        """Before the frame's pass.  gt_t float64 [B,4] (or [B,16] polygons: ntk_track_supervise_poly; or a frame of a MaskRound:
        ntk_track_supervise_mask), active_t uint8 [B] (nullable), clip_of int32 [B], on the device.
        -> (track, restart) uint8 [B]: the masks of the pass (the supervisor's own buffers, overwritten by the next plan).  codes
        int8 [B] and frame_iou float64 [B] (nullable) are filled for every slot."""
        truth = as_round_truth(gt_t, self.device, "Supervisor", shape=(self.B,))
        self._call(SUP_PLAN, None, truth, truth.plan_pointers(), active_t, clip_of, codes, frame_iou)
        return self.track, self.restart

    def judge(self, regions, gt_t, clip_of, codes=None, frame_iou=None):
        """After the pass: the tracked slots (the last plan's ``track``) are scored against gt_t; codes / frame_iou as given to
        plan are completed."""
        truth = as_round_truth(gt_t, self.device, "Supervisor", shape=(self.B,))
        self._call(SUP_JUDGE, regions, truth, truth.judge_pointers(), None, clip_of, codes, frame_iou)

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
        from . import _lib
        self.n_runs, self.failure_overlap, self.patience = int(n_runs), float(failure_overlap), int(patience)
        first = np.ascontiguousarray(trace_first, dtype=np.int64).reshape(-1)
        if (self.n_runs < 1 or len(first) != self.n_runs + 1 or first[0] != 0 or (np.diff(first) < 0).any() or self.patience < 0
                or not 0 <= self.failure_overlap < 1):
            raise ValueError("MultiStart: n_runs=%d, %d ascending trace_first entries from 0 (n_runs + 1), patience=%d (>= 0), "
                             "failure_overlap=%g (in [0,1))" % (self.n_runs, len(first), self.patience, self.failure_overlap))
        self.device = torch.device(device)
        self.trace_first = first
        self._first = _lib.upload(first, torch.int64, self.device)
        self.table = torch.zeros((self.n_runs, MS_HEAD), dtype=torch.float64, device=self.device)
        self.trace = torch.zeros((max(int(first[-1]), 1),), dtype=torch.float64, device=self.device)      # never an empty buffer

    def add(self, regions, gt, clip_of, active=None, frame_iou=False):
        """OverlapScores.add's arguments (clip_of [B]: the RUN of slot b) -> one ntk_track_multistart, _poly or (after the
        MaskRound's one ntk_track_mask_overlaps) _mask."""
        from . import _lib
        P = _lib.ptr
        regions, truth, mask, clip_of, T, B, out = _scoring_call("MultiStart.add", self.device, regions, gt, clip_of, active,
                                                                 frame_iou)
        name = "ntk_track_multistart" + truth.suffix
        _lib.check(getattr(_lib.lib(), name)(P(regions), *truth.scoring_pointers(regions), P(mask), P(clip_of), T, B, self.n_runs,
                                             self.failure_overlap, self.patience, P(self.table), P(self._first), P(self.trace),
                                             P(out), _lib.stream()), name)
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
