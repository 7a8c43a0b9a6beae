"""Time evaluate.validate over the same synthetic clips once with polygon ground truth and once with the polygons' masks (dev tool).

  dev_validate_masks_timing.py [--B 16 64] [--clips-per-slot 2] [--T 8] [--passes 3] [--size 360 640] [--commit ID] [--out FILE]

Synthetic 640 x 360 uint8 clips held as HOST arrays, clip lengths uniform in [8, 24], the ground truth a rectangle of 40 .. 120 px
a side turned by 20 degrees that drifts a few pixels per frame; the mask of a frame is the set of pixels whose centre lies inside
the frame's polygon (evaluate.MaskRegions.from_arrays codes it over its tight box).  The shapes of profiles/online_batch.txt's
cell and trunk with random weights.  Both protocols; the arms (polygon, mask) alternate pass by pass, pass 0 warms up, the figure
is the median of the others.  Wall-clock time from the call to the result on the host, the device idle before and after.
objects.frames/s counts tracked frames (a clip of L frames has L - 1).  profiles/validate_masks.txt holds the output."""
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
ap.add_argument("--passes", type=int, default=3, help="timed passes per arm after one warm-up pass")
ap.add_argument("--size", nargs=2, type=int, default=[360, 640], metavar=("H", "W"))
ap.add_argument("--commit", default="unknown")
ap.add_argument("--out", default=None, help="append the report to this file as well")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("dev_validate_masks_timing.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")
H, W = args.size
T = args.T
TURN = np.radians(20.0)
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: sorted(v)[len(v) // 2]
rng = np.random.default_rng(0)
vgg = VGG16Conv43(O.init_vgg_weights(rng), device=dev)
cell = NTMCell(2, mem_size=128, mem_dim=20, controller_hidden_size=200, controller_num_layers=1, write_head_size=1,
               read_head_size=4, input_dim=514, device=dev, init_scale=0.05, seed=1)


def turned(r):
    cx, cy, c, s = r[0] + r[2] / 2, r[1] + r[3] / 2, np.cos(TURN), np.sin(TURN)
    return np.array([(cx + dx * c - dy * s, cy + dx * s + dy * c)
                     for dx, dy in ((-r[2] / 2, -r[3] / 2), (r[2] / 2, -r[3] / 2), (r[2] / 2, r[3] / 2), (-r[2] / 2, r[3] / 2))])


def raster(quad):
    """The pixels of the frame whose centre lies inside the convex polygon."""
    y, x = np.mgrid[:H, :W]
    x, y = x + 0.5, y + 0.5
    inside = np.ones((H, W), dtype=bool)
    for i in range(len(quad)):
        (ax, ay), (bx, by) = quad[i], quad[(i + 1) % len(quad)]
        inside &= (bx - ax) * (y - ay) - (by - ay) * (x - ax) >= 0
    return inside


def make_clips(n, seed):
    """-> (polygon clips, mask clips) over the same frames."""
    r = np.random.default_rng(seed)
    polys, masks = [], []
    for _ in range(n):
        L = int(r.integers(8, 25))
        wh = r.uniform(40, 120, size=2)
        start = np.concatenate([r.uniform(0.15, 0.85, size=2) * (np.array([W, H]) - wh), wh])
        boxes = start + np.cumsum(r.uniform(-2, 2, size=(L, 4)), axis=0)
        quads = np.stack([turned(b) for b in boxes])
        frames = r.integers(0, 256, size=(L, H, W, 3), dtype=np.uint8)
        polys.append(evaluate.Clip(frames, quads.reshape(L, 8)))
        masks.append(evaluate.Clip(frames, evaluate.MaskRegions.from_arrays(np.stack([raster(q) for q in quads]))))
    return polys, masks


def round_counts(clips, B):
    """The counts of every round's upload: n_rle per round, as MaskTruth.round concatenates them."""
    out = []
    for rnd in evaluate.ClipSchedule([len(c.regions) for c in clips], B, T):
        n_rle = 0
        for b in range(rnd.active.shape[1]):
            n = int(rnd.active[:, b].sum())
            if n:
                off = clips[int(rnd.clip_of[b])].regions.offsets
                n_rle += int(off[rnd.frame_index[n - 1, b] + 1] - off[rnd.frame_index[0, b]])
        out.append(n_rle)
    return out


make = lambda images, regions: online.BatchNTMTracker(images, regions, cell, vgg, device=dev)


def run(protocol, clips, B):
    res = evaluate.validate(make, clips, B, T, device=dev, protocol=protocol)
    return res["mean_overlap_frames"] if protocol == "one_pass" else (res["accuracy_frames"], res["failures"], res["restarts"])


say("box: %s | torch %s | commit %s | frames %dx%d uint8 on the host | rounds of %d frames | %d timed passes after 1 warm-up"
    % (torch.cuda.get_device_name(0), torch.__version__, args.commit, W, H, T, args.passes))
for B in args.B:
    polys, masks = make_clips(args.clips_per_slot * B, 100 + B)
    tracked = sum(len(c.regions) - 1 for c in polys)
    passes = T * sum(1 for _r in evaluate.ClipSchedule([len(c.regions) for c in polys], B, T))
    per_mask = np.concatenate([np.diff(c.regions.offsets) for c in masks])
    n_rle = round_counts(masks, B)
    say("B %d: %d clips, %d tracked frames, %d frame passes | counts per mask: mean %.1f, min %d, max %d | n_rle of a round "
        "(T x B = %d masks): median %d, max %d" % (B, len(polys), tracked, passes, per_mask.mean(), per_mask.min(), per_mask.max(),
                                                    T * B, med(n_rle), max(n_rle)))
    for protocol in ("one_pass", "supervised"):
        arms = (("polygon", polys), ("mask", masks))
        times, values = {n: [] for n, _c in arms}, {}
        for it in range(args.passes + 1):
            for name, clips in arms:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                values[name] = run(protocol, clips, B)
                torch.cuda.synchronize()
                if it > 0:
                    times[name].append(time.perf_counter() - t0)
        say("  %-10s | %s | mask / polygon %.3f" % (protocol, " | ".join(
            "%-7s %7.3f s %8.0f obj.fr/s %7.3f ms/pass, timed passes %s" % (
                n, med(times[n]), tracked / med(times[n]), 1e3 * med(times[n]) / passes, " ".join("%.3f" % t for t in times[n]))
            for n, _c in arms), med(times["mask"]) / med(times["polygon"])))
        say("  %-10s   result (one_pass: mean overlap; supervised: accuracy, failures, restarts): %s"
            % ("", ", ".join("%s %s" % (n, values[n]) for n, _c in arms)))
    del polys, masks
say("s: wall-clock seconds of one whole validation, median of the timed passes; ms/pass: s over the tracker's frame passes "
    "(rounds x T, each one crop, one trunk pass, one sequence for B slots).")
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
