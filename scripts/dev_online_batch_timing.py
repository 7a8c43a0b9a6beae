"""Time online tracking of B objects: a Python loop over B online.NTMTracker instances (one object per call, the host in
the loop of every frame) against one online.BatchNTMTracker.track_clip (dev tool).

  dev_online_batch_timing.py [--B 1 4 16 64] [--frames 20] [--passes 5] [--size 360 640] [--commit ID] [--out FILE]

640 x 360 uint8 frames resident on the device for BOTH forms (the single tracker converts its frame to fp32 per call, as it
always does), benchmark cell with random weights, 20 frames per clip; for every B, F = 1 (B objects in one video) and F = B
(one object in each of B clips).  HIP events around a whole clip; the first pass of every form warms up, the figure is the
median of the others.  The batched form is timed a second time with events between its pieces (crop / trunk /
serialise + sequence / box update).  profiles/online_batch.txt holds the output, with the spread between repeated processes."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from oracle import ntm_oracle as O
from ntmtrack import online
from ntmtrack.ntm import NTMCell
from ntmtrack.vgg import VGG16Conv43

ap = argparse.ArgumentParser()
ap.add_argument("--B", nargs="+", type=int, default=[1, 4, 16, 64])
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--passes", type=int, default=5, help="timed passes per form after one warm-up pass")
ap.add_argument("--size", nargs=2, type=int, default=[360, 640], metavar=("H", "W"))
ap.add_argument("--commit", default="unknown")
ap.add_argument("--out", default=None, help="append the report to this file as well")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("dev_online_batch_timing.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")
H, W = args.size
T = args.frames
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def ev():
    return torch.cuda.Event(enable_timing=True)


med = lambda v: sorted(v)[len(v) // 2]
rng = np.random.default_rng(0)
vgg = VGG16Conv43(O.init_vgg_weights(rng), device=dev)
cell = NTMCell(2, mem_size=128, mem_dim=20, controller_hidden_size=200, controller_num_layers=1, write_head_size=1,
               read_head_size=4, input_dim=514, device=dev, init_scale=0.05, seed=1)
say("box: %s | torch %s | commit %s | frames %dx%d uint8 | %d frames per clip | %d timed passes after 1 warm-up"
    % (torch.cuda.get_device_name(0), torch.__version__, args.commit, W, H, T, args.passes))
say("%3s %3s | %28s | %28s | %6s | %s" % ("B", "F", "loop of NTMTracker", "BatchNTMTracker.track_clip", "ratio",
                                           "batched split, ms per frame"))
say("%3s %3s | %9s %9s %8s | %9s %9s %8s | %6s | %s" % ("", "", "ms/frame", "obj.fr/s", "spread", "ms/frame", "obj.fr/s", "spread",
                                                        "", "crop / trunk / serialise+sequence / box update"))


def regions_for(B):
    r = np.random.default_rng(100 + B)
    wh = r.uniform(40, 120, size=(B, 2))
    xy = r.uniform(0, 1, size=(B, 2)) * (np.array([W, H]) - wh)
    return np.concatenate([xy, wh], axis=1)


def single_pass(clip, frame_of, regions):
    """B single trackers, frame by frame as validate_tracker.py drives them; -> ms per frame (all B objects)."""
    trks = [online.NTMTracker(clip[0, f], tuple(r), cell, vgg, device=dev) for r, f in zip(regions, frame_of)]
    torch.cuda.synchronize()
    e0, e1 = ev(), ev()
    e0.record()
    for t in range(1, T + 1):
        for trk, f in zip(trks, frame_of):
            trk.track(clip[t, f])
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / T


def batch_pass(clip, frame_of, regions):
    trk = online.BatchNTMTracker(clip[0], regions, cell, vgg, frame_of=frame_of, device=dev)
    torch.cuda.synchronize()
    e0, e1 = ev(), ev()
    e0.record()
    out = trk.track_clip(clip[1:])
    e1.record()
    torch.cuda.synchronize()
    assert out.shape == (T, len(regions), 4)
    return e0.elapsed_time(e1) / T


def batch_split_pass(clip, frame_of, regions):
    """The same launches with events between the pieces -> ms per frame of each piece."""
    trk = online.BatchNTMTracker(clip[0], regions, cell, vgg, frame_of=frame_of, device=dev)
    torch.cuda.synchronize()
    evs = []
    for t in range(1, T + 1):
        e = [ev() for _ in range(5)]
        e[0].record()
        crops = trk._crop(clip[t], trk.frame_of, trk.cropbox32, out=trk._crops)
        e[1].record()
        fmap = trk._trunk(crops)
        e[2].record()
        logits = trk._sequence(trk._serialize(fmap, None, X=trk._X), None)
        e[3].record()
        trk._update_boxes(logits, None)
        e[4].record()
        evs.append(e)
    torch.cuda.synchronize()
    return [sum(e[i].elapsed_time(e[i + 1]) for e in evs) / T for i in range(4)]


for B in args.B:
    regions = regions_for(B)
    for F in sorted({1, B}):
        clip = torch.randint(0, 256, (T + 1, F, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(B))
        frame_of = [0] * B if F == 1 else list(range(B))
        single, batch = [], []
        for it in range(args.passes + 1):                   # the two forms alternate, pass by pass; pass 0 warms up
            s, b = single_pass(clip, frame_of, regions), batch_pass(clip, frame_of, regions)
            if it > 0:
                single.append(s)
                batch.append(b)
        split = batch_split_pass(clip, frame_of, regions)
        ms, mb = med(single), med(batch)
        say("%3d %3d | %9.3f %9.0f %8.3f | %9.3f %9.0f %8.3f | %5.2fx | %.3f / %.3f / %.3f / %.3f"
            % (B, F, ms, 1e3 * B / ms, max(single) - min(single), mb, 1e3 * B / mb, max(batch) - min(batch), ms / mb, *split))
        del clip
say("ms/frame: one frame of all B objects, median of the timed passes; spread: max - min of those passes (ms); ratio: loop / batched.")
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
