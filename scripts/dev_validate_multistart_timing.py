"""Time evaluate.validate(protocol="multistart") against the one-pass validation of the same run clips, and ntk_track_eao_curve
on synthetic finished runs (dev tool).

  dev_validate_multistart_timing.py [--B 16] [--clips 16] [--T 8] [--passes 9] [--size 360 640] [--curve-runs 500 20000]
                                    [--curve-frames 250 5000] [--commit ID] [--out FILE]

Part 1: synthetic 640 x 360 uint8 clips held as HOST arrays, clip lengths uniform in [60, 140], the ground truth a box of 40 .. 120
px a side that drifts a few pixels per frame; anchors 50 frames apart (the default), so a clip has 3 to 4 runs.  The shapes of
profiles/online_batch.txt's cell and trunk with random weights.  The two arms run the same run clips on the same schedule and
differ in the round's scoring launch alone (ntk_track_multistart / ntk_track_overlap_scores) and in the one reduction at the
end; they alternate pass by pass, pass 0 warms up, the figure is the median of the others and all are printed.  Wall-clock time
from the call to the result on the host, the device idle before and after.

Part 2: a table and a trace of finished runs made on the device (run lengths uniform in [frames / 2, frames], three runs in ten
failed at a uniform ordinal, overlaps uniform in [0, 1)), ntk_track_eao_curve with n_max = 755 between two device events, one
warm-up launch, the median of the others.  profiles/validate_multistart.txt holds the output."""
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
ap.add_argument("--B", type=int, default=16)
ap.add_argument("--clips", type=int, default=16)
ap.add_argument("--T", type=int, default=8, help="frames per round")
ap.add_argument("--passes", type=int, default=9, help="timed passes per arm after one warm-up pass")
ap.add_argument("--size", nargs=2, type=int, default=[360, 640], metavar=("H", "W"))
ap.add_argument("--curve-runs", nargs="+", type=int, default=[500, 20000])
ap.add_argument("--curve-frames", nargs="+", type=int, default=[250, 5000], help="the longest run of each --curve-runs set")
ap.add_argument("--commit", default="unknown")
ap.add_argument("--out", default=None, help="append the report to this file as well")
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("dev_validate_multistart_timing.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")
H, W = args.size
T, B = args.T, args.B
N_MAX = 755
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: sorted(v)[len(v) // 2]
rng = np.random.default_rng(0)
vgg = VGG16Conv43(O.init_vgg_weights(rng), device=dev)
cell = NTMCell(2, mem_size=128, mem_dim=20, controller_hidden_size=200, controller_num_layers=1, write_head_size=1,
               read_head_size=4, input_dim=514, device=dev, init_scale=0.05, seed=1)
make = lambda images, regions: online.BatchNTMTracker(images, regions, cell, vgg, device=dev)

say("box: %s | torch %s | commit %s | frames %dx%d uint8 on the host | B %d, rounds of %d frames | %d timed passes after 1 warm-up"
    % (torch.cuda.get_device_name(0), torch.__version__, args.commit, W, H, B, T, args.passes))

# ---- part 1: the validator
clips = []
for _ in range(args.clips):
    L = int(rng.integers(60, 141))
    wh = rng.uniform(40, 120, size=2)
    start = np.concatenate([rng.uniform(0.15, 0.85, size=2) * (np.array([W, H]) - wh), wh])
    clips.append(evaluate.Clip(rng.integers(0, 256, size=(L, H, W, 3), dtype=np.uint8),
                               start + np.cumsum(rng.uniform(-2, 2, size=(L, 4)), axis=0)))
run_clips, runs = evaluate.multistart_runs(clips)
tracked = int((runs[:, 3] - 1).sum())
rounds = sum(1 for _r in evaluate.ClipSchedule(runs[:, 3].tolist(), B, T))
say("%d clips of %d..%d frames -> %d runs (%d backward), %d tracked frames, %d rounds = %d frame passes"
    % (len(clips), min(len(c.regions) for c in clips), max(len(c.regions) for c in clips), len(runs), int((runs[:, 2] < 0).sum()),
       tracked, rounds, rounds * T))
arms = (("one_pass", lambda: evaluate.validate(make, run_clips, B, T, device=dev)["mean_overlap_frames"]),
        ("multistart", lambda: (lambda r: (r["accuracy"], r["robustness"], r["eao"], r["failures"]))(
            evaluate.validate(make, clips, B, T, device=dev, protocol="multistart"))))
times, values = {n: [] for n, _f in arms}, {}
for it in range(args.passes + 1):
    for name, fn in arms:
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        values[name] = fn()
        torch.cuda.synchronize()
        if it > 0:
            times[name].append(time.perf_counter() - t0)
for name, _f in arms:
    say("  %-10s %7.3f s %7.1f rounds/s %8.0f obj.fr/s, timed passes %s"
        % (name, med(times[name]), rounds / med(times[name]), tracked / med(times[name]), " ".join("%.3f" % t for t in times[name])))
say("  multistart / one_pass %.3f | results: one_pass mean overlap %.4f; multistart (accuracy, robustness, EAO, failures) %s"
    % (med(times["multistart"]) / med(times["one_pass"]), values["one_pass"], values["multistart"]))
del clips, run_clips

# ---- part 2: the EAO reduction
for n_runs, longest in zip(args.curve_runs, args.curve_frames):
    lengths = rng.integers(longest // 2, longest + 1, size=n_runs)
    first = np.concatenate([[0], np.cumsum(lengths)])
    ms = evaluate.MultiStart(n_runs, first, device=dev)
    ms.trace.uniform_(0, 1)
    failed = rng.random(n_runs) < 0.3
    table = np.zeros((n_runs, evaluate.MS_HEAD))
    table[:, evaluate.MS_FRAMES], table[:, evaluate.MS_FAILED] = lengths, failed
    table[:, evaluate.MS_TRACKED] = np.where(failed, (rng.random(n_runs) * lengths).astype(np.int64), lengths)
    ms.table.copy_(torch.from_numpy(table).to(dev))
    ms_times = []
    for it in range(args.passes + 1):
        t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        t0.record()
        curve = ms.curve(N_MAX)
        t1.record()
        torch.cuda.synchronize()
        if it > 0:
            ms_times.append(t0.elapsed_time(t1))
    say("ntk_track_eao_curve: %d runs of %d..%d scored frames, %.3g trace entries (%.1f MB trace + as much prefix), n_max %d: "
        "%.3f ms (median; both kernels and the two buffers' allocation), timed launches %s | mean of the curve %.4f"
        % (n_runs, lengths.min(), lengths.max(), first[-1], first[-1] * 8 / 1e6, N_MAX, med(ms_times),
           " ".join("%.3f" % t for t in ms_times), float(curve.mean())))
    del ms, curve
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
