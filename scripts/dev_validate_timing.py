"""Time validation over clips: evaluate.validate (continuous batching, scores kept on the device, one read-back at the end)
against the two ways the public API allowed before it, both written here from that API alone (dev tool).

  dev_validate_timing.py [--B 16 64] [--clips-per-slot 2] [--T 8] [--passes 3] [--size 360 640] [--commit ID] [--out FILE]
  dev_validate_timing.py --protocols one_pass supervised [...]      the two protocols of evaluate.validate on clips without failures

  recipe   the continuous-batching loop a caller had to write: B slots, BatchNTMTracker.reset for the slots whose clip ended, one
           track_clip with a mask per round, `out.cpu()` and a NumPy scorer per round
  singles  one online.NTMTracker per clip, frame by frame (validate_tracker.py:26-38), every region scored on the host

Synthetic 640 x 360 uint8 clips held as HOST arrays for all three forms (a validation set comes from disk), clip lengths uniform in
[8, 24], the shapes of profiles/online_batch.txt's cell and trunk with random weights.  --protocols: the ground truth of every
clip is replaced by what the tracker itself returns on it (one untimed one-pass run), so that every overlap is 1 and the supervised
protocol restarts nothing: what is timed is its per-frame bookkeeping on top of the same passes (profiles/validate_supervised.txt;
`--protocols one_pass` alone runs on a commit that has no protocol argument yet).  Wall-clock time from the first call to the
last result on the host, the device idle before and after; the forms alternate pass by pass, pass 0 warms up, the figure is the
median of the others.  objects.frames/s counts tracked frames (a clip of L frames has L - 1).  profiles/validate.txt holds the output."""
import argparse
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from oracle import ntm_oracle as O
from ntmtrack import evaluate, online
from ntmtrack.ntm import NTMCell
from ntmtrack.vgg import VGG16Conv43

ap = argparse.ArgumentParser()
ap.add_argument("--B", nargs="+", type=int, default=[16, 64])
ap.add_argument("--clips-per-slot", type=int, default=2)
ap.add_argument("--T", type=int, default=8, help="frames per round")
ap.add_argument("--passes", type=int, default=3, help="timed passes per form after one warm-up pass")
ap.add_argument("--size", nargs=2, type=int, default=[360, 640], metavar=("H", "W"))
ap.add_argument("--commit", default="unknown")
ap.add_argument("--protocols", nargs="+", choices=["one_pass", "supervised"], default=None,
                help="time these protocols of evaluate.validate on clips without failures instead of the three forms")
ap.add_argument("--out", default=None, help="append the report to this file as well")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("dev_validate_timing.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")
H, W = args.size
T = args.T
IOU_THR, DIST_THR = np.linspace(0, 1, 21), np.arange(0, 51.)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: sorted(v)[len(v) // 2]
rng = np.random.default_rng(0)
vgg = VGG16Conv43(O.init_vgg_weights(rng), device=dev)
cell = NTMCell(2, mem_size=128, mem_dim=20, controller_hidden_size=200, controller_num_layers=1, write_head_size=1,
               read_head_size=4, input_dim=514, device=dev, init_scale=0.05, seed=1)


def make_clips(n, seed):
    r = np.random.default_rng(seed)
    clips = []
    for _ in range(n):
        L = int(r.integers(8, 25))
        wh = r.uniform(40, 120, size=2)
        start = np.concatenate([r.uniform(0, 1, size=2) * (np.array([W, H]) - wh), wh])
        regions = start + np.cumsum(r.uniform(-2, 2, size=(L, 4)), axis=0)
        clips.append(evaluate.Clip(r.integers(0, 256, size=(L, H, W, 3), dtype=np.uint8), regions))
    return clips


def host_scores(table, rows, pred, gt):
    """NumPy scorer of the two older forms: pred, gt [n,4] (x, y, w, h) -> adds to table[rows] (frames, sum IoU, sum distance,
    lost, success counts, precision counts)."""
    pw, ph = np.maximum(pred[:, 2], 0), np.maximum(pred[:, 3], 0)
    ix = np.minimum(pred[:, 0] + pw, gt[:, 0] + gt[:, 2]) - np.maximum(pred[:, 0], gt[:, 0])
    iy = np.minimum(pred[:, 1] + ph, gt[:, 1] + gt[:, 3]) - np.maximum(pred[:, 1], gt[:, 1])
    inter = np.where((ix > 0) & (iy > 0), ix * iy, 0.0)
    iou = np.clip(inter / (pw * ph + gt[:, 2] * gt[:, 3] - inter), 0, 1)
    dist = np.hypot(pred[:, 0] + pw / 2 - gt[:, 0] - gt[:, 2] / 2, pred[:, 1] + ph / 2 - gt[:, 1] - gt[:, 3] / 2)
    cols = np.concatenate([np.ones_like(iou)[:, None], iou[:, None], dist[:, None], (iou == 0)[:, None],
                           iou[:, None] > IOU_THR[None], dist[:, None] <= DIST_THR[None]], axis=1).astype(np.float64)
    np.add.at(table, rows, cols)


def run_validate(clips, B):
    make = lambda images, regions: online.BatchNTMTracker(images, regions, cell, vgg, device=dev)
    return evaluate.validate(make, clips, B, T, device=dev)["mean_overlap_frames"]


def run_recipe(clips, B):
    """INTEGRATION.md's three steps as they stood: reset, track_clip with a mask, out.cpu() and a host scorer per round."""
    table = np.zeros((len(clips), 4 + len(IOU_THR) + len(DIST_THR)))
    B = min(B, len(clips))
    slot_clip, slot_pos, upcoming, trk = [-1] * B, [0] * B, 0, None
    while True:
        new = []
        for s in range(B):
            if slot_clip[s] < 0 and upcoming < len(clips):
                slot_clip[s], slot_pos[s] = upcoming, 1
                new.append(s)
                upcoming += 1
        if all(c < 0 for c in slot_clip):
            break
        if new:
            images = np.stack([clips[slot_clip[s]].frames[0] for s in new])
            regions = np.stack([clips[slot_clip[s]].regions[0] for s in new])
            if trk is None:
                trk = online.BatchNTMTracker(images, regions, cell, vgg, device=dev)
            else:
                trk.reset(new, images, regions)
        frames, mask = np.zeros((T, B, H, W, 3), dtype=np.uint8), np.zeros((T, B), dtype=np.uint8)
        gt, rows = np.zeros((T, B, 4)), np.zeros((T, B), dtype=np.int64)
        for s in range(B):
            c = slot_clip[s]
            if c < 0:
                continue
            n = min(T, len(clips[c].regions) - slot_pos[s])
            frames[:n, s], gt[:n, s] = clips[c].frames[slot_pos[s]:slot_pos[s] + n], clips[c].regions[slot_pos[s]:slot_pos[s] + n]
            mask[:n, s], rows[:, s] = 1, c
            slot_pos[s] += n
            if slot_pos[s] == len(clips[c].regions):
                slot_clip[s] = -1
        out = trk.track_clip(frames, active=mask).cpu().numpy()          # the synchronisation of every round
        on = mask.astype(bool)
        host_scores(table, rows[on], out[on], gt[on])
    return table[:, 1].sum() / table[:, 0].sum()


def run_singles(clips, _B):
    table = np.zeros((len(clips), 4 + len(IOU_THR) + len(DIST_THR)))
    for i, c in enumerate(clips):
        trk = online.NTMTracker(c.frames[0], tuple(c.regions[0]), cell, vgg, device=dev)
        pred = np.array([tuple(trk.track(c.frames[t])) for t in range(1, len(c.regions))])
        host_scores(table, np.full(len(pred), i), pred, c.regions[1:])
    return table[:, 1].sum() / table[:, 0].sum()


def run_protocols():
    make = lambda images, regions: online.BatchNTMTracker(images, regions, cell, vgg, device=dev)

    def run(name, clips, B):
        if name == "one_pass":                       # no protocol argument: the call a commit without one understands
            return evaluate.validate(make, clips, B, T, device=dev)["mean_overlap_frames"]
        res = evaluate.validate(make, clips, B, T, device=dev, protocol="supervised")
        assert res["failures"] == 0 and res["restarts"] == 0, "the clips were meant to have no failure"
        return res["accuracy_frames"]
    say("box: %s | torch %s | commit %s | frames %dx%d uint8 on the host | rounds of %d frames | %d timed passes after 1 warm-up"
        % (torch.cuda.get_device_name(0), torch.__version__, args.commit, W, H, T, args.passes))
    say("%3s %5s %7s %6s | %s" % ("B", "clips", "obj.fr", "passes", " | ".join("%-10s %8s %9s %9s %7s" % (n, "s", "obj.fr/s", "ms/pass", "spread")
                                                                             for n in args.protocols)))
    for B in args.B:
        clips = make_clips(args.clips_per_slot * B, 100 + B)
        _res, tracked_regions = evaluate.validate(make, clips, B, T, return_regions=True, device=dev)
        clips = [evaluate.Clip(c.frames, np.concatenate([c.regions[:1], r])) for c, r in zip(clips, tracked_regions)]
        assert all(np.isfinite(c.regions).all() and (c.regions[:, 2:] > 0).all() for c in clips)
        tracked = sum(len(c.regions) - 1 for c in clips)
        passes = T * sum(1 for _r in evaluate.ClipSchedule([len(c.regions) for c in clips], B, T))    # frame passes of the tracker
        times, values = {n: [] for n in args.protocols}, {}
        for it in range(args.passes + 1):
            for name in args.protocols:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                values[name] = run(name, clips, B)
                torch.cuda.synchronize()
                if it > 0:
                    times[name].append(time.perf_counter() - t0)
        say("%3d %5d %7d %6d | %s" % (B, len(clips), tracked, passes, " | ".join(
            "%-10s %8.3f %9.0f %9.3f %7.3f" % (n, med(times[n]), tracked / med(times[n]), 1e3 * med(times[n]) / passes,
                                              max(times[n]) - min(times[n])) for n in args.protocols)))
        say("          mean overlap (one_pass) / accuracy (supervised: the frames after the burn-in): %s"
            % ", ".join("%s %.6f" % (n, values[n]) for n in args.protocols))
        del clips
    say("s: wall-clock seconds of one whole validation, median of the timed passes; ms/pass: s over the tracker's frame passes "
        "(rounds x T, each one crop, one trunk pass, one sequence for B slots); spread: max - min of the timed passes (s).")


if args.protocols:
    run_protocols()
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)

FORMS = (("validate", run_validate), ("recipe", run_recipe), ("singles", run_singles))
say("box: %s | torch %s | commit %s | frames %dx%d uint8 on the host | rounds of %d frames | %d timed passes after 1 warm-up"
    % (torch.cuda.get_device_name(0), torch.__version__, args.commit, W, H, T, args.passes))
say("%3s %5s %7s | %s" % ("B", "clips", "obj.fr", " | ".join("%-8s %9s %9s %7s" % (n, "s", "obj.fr/s", "spread") for n, _f in FORMS)))
for B in args.B:
    clips = make_clips(args.clips_per_slot * B, 100 + B)
    tracked = sum(len(c.regions) - 1 for c in clips)
    times, values = {n: [] for n, _f in FORMS}, {}
    for it in range(args.passes + 1):
        for name, fn in FORMS:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            values[name] = fn(clips, B)
            torch.cuda.synchronize()
            if it > 0:
                times[name].append(time.perf_counter() - t0)
    say("%3d %5d %7d | %s" % (B, len(clips), tracked, " | ".join(
        "%-8s %9.3f %9.0f %7.3f" % (n, med(times[n]), tracked / med(times[n]), max(times[n]) - min(times[n])) for n, _f in FORMS)))
    say("          mean overlap of the three forms (the same clips; the forms differ by fp32 rounding of the trunk forms): %s"
        % ", ".join("%s %.6f" % (n, values[n]) for n, _f in FORMS))
    del clips
say("s: wall-clock seconds of one whole validation, median of the timed passes; spread: max - min of those passes (s).")
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
