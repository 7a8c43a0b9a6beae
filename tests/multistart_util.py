"""NumPy restatement of the multi-start protocol's rules (include/ntmtrack.h, NTK_MS_*), written from the rules
in plain Python on top of evaluate_util.frame_score: ``anchors`` (which runs a clip has), ``walk`` (the run table and the trace
of rounds of frames) and ``curve_exact`` (the EAO curve in exact rational arithmetic).

walk keeps no running state: after every round a run's table row is recomputed from the whole list of its overlaps so far, by
the definitions -- the first ordinal f whose frames f ... f + patience are all low, the trailing streak, sums added in frame
order -- so that nothing of the kernel's incremental bookkeeping is shared."""
from fractions import Fraction

import numpy as np

import evaluate_util as U

FRAMES, TRACKED, SUM_IOU, FAILED, LOW, PENDING, HEAD = 0, 1, 2, 3, 4, 5, 6


def anchors(present, spacing=50, given=None):
    """present: bool [L], the frames with ground truth -> the runs of the clip as a list of (start, direction, length), in order.
    The anchors are 0, spacing, 2 spacing, ... and L - 1 (or ``given``); forward when at least as many frames lie ahead as behind;
    an absent anchor moves along its direction to the first present frame; fewer than 2 frames: dropped; same start and direction:
    one run."""
    L = len(present)
    marks = sorted(set(given)) if given is not None else sorted(set(list(range(0, L, spacing)) + [L - 1]))
    out = []
    for a in marks:
        ahead, behind = L - 1 - a, a
        d = 1 if ahead >= behind else -1
        frames = list(range(a, L)) if d == 1 else list(range(a, -1, -1))
        while frames and not present[frames[0]]:
            frames = frames[1:]
        if len(frames) < 2:
            continue
        run = (frames[0], d, len(frames))
        if run not in out:
            out.append(run)
    return out


def frame_overlaps(pred, gt, active=None, score=U.frame_score):
    """[T,B] float64: the overlap of every scored frame, NaN where a frame is not scored (``score`` returns None)."""
    T, B = np.asarray(pred).shape[:2]
    out = np.full((T, B), np.nan)
    for t in range(T):
        for b in range(B):
            s = score(pred[t][b], gt[t][b], True if active is None else bool(active[t][b]))
            if s is not None:
                out[t, b] = s[0]
    return out


def in_order_sum(values):
    s = np.float64(0.0)
    for v in values:
        s = s + np.float64(v)
    return s


def run_row(overlaps, failure_overlap, patience):
    """The table row of a run from all of its scored frames' overlaps, in frame order."""
    n = len(overlaps)
    low = [o <= failure_overlap for o in overlaps]
    fails = [f for f in range(n - patience) if all(low[f:f + patience + 1])]
    row = np.zeros(HEAD)
    row[FRAMES] = n
    if fails:
        f = fails[0]
        row[TRACKED], row[FAILED], row[SUM_IOU] = f, 1, in_order_sum(overlaps[:f])
        row[PENDING] = row[SUM_IOU]
        return row
    streak = 0
    while streak < n and low[n - 1 - streak]:
        streak += 1
    row[TRACKED], row[LOW] = n - streak, streak
    row[SUM_IOU], row[PENDING] = in_order_sum(overlaps[:n - streak]), in_order_sum(overlaps)
    return row


def walk(rounds, n_runs, trace_first, failure_overlap=0.1, patience=10):
    """rounds: a list of (overlaps [T,B] with NaN where a frame is not scored, run_of [B]) -> (table [n_runs, HEAD], trace
    [trace_first[n_runs]], zeros where nothing was written).  A slot whose run is outside [0, n_runs) is skipped."""
    seen = [[] for _ in range(n_runs)]
    for overlaps, run_of in rounds:
        T, B = overlaps.shape
        for b in range(B):
            r = int(run_of[b])
            if 0 <= r < n_runs:
                seen[r].extend(overlaps[t, b] for t in range(T) if not np.isnan(overlaps[t, b]))
    table, trace = np.zeros((n_runs, HEAD)), np.zeros(int(trace_first[n_runs]))
    for r, o in enumerate(seen):
        table[r] = run_row(o, failure_overlap, patience)
        assert len(o) <= trace_first[r + 1] - trace_first[r]
        trace[trace_first[r]:trace_first[r] + len(o)] = o
    return table, trace


def finished(table):
    """-> (N, N_F, failed) of finished runs: an open streak is forgiven."""
    failed = table[:, FAILED] != 0
    return table[:, FRAMES].astype(int), np.where(failed, table[:, TRACKED], table[:, FRAMES]).astype(int), failed


def curve_exact(table, trace_first, trace, n_max):
    """Phi(1 ... n_max) as float64 [n_max], every sum and quotient in exact rational arithmetic over the float64 overlaps and
    rounded once; NaN where S_n is empty."""
    N, N_F, failed = finished(table)
    out = np.full(n_max, np.nan)
    prefix = []                                                     # per run: P(k) for k = 0 ... N_F
    for r in range(len(table)):
        p = [Fraction(0)]
        for i in range(N_F[r]):
            p.append(p[-1] + Fraction(float(trace[trace_first[r] + i])))
        prefix.append(p)
    for n in range(1, n_max + 1):
        members = [r for r in range(len(table)) if N[r] > 0 and (failed[r] or N[r] >= n)]
        if members:
            out[n - 1] = float(sum(prefix[r][min(n, N_F[r])] / n for r in members) / len(members))
    return out
