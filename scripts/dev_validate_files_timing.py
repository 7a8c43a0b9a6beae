"""Time validation from image files (dev tool): a seeded synthetic VOT tree written by Pillow (quality 90, 4:2:0, no restart
markers), validated in three forms.

  dev_validate_files_timing.py [--B 16 64] [--T 8 24] [--clips-per-slot 4] [--passes 3] [--size 360 640] [--big 16 8]
                               [--forms a b c] [--root DIR] [--tree DIR] [--commit ID] [--out FILE]
  dev_validate_files_timing.py --rss-form a|b|c --tree DIR [--B 64] [--T 24]      peak resident set of one validation

  a  data.vot_clips(root): every scheduled clip decoded whole by Pillow on one thread into float32 (the only form a commit
     without frames="files" has; --root DIR imports the package from a checkout of such a commit, with --forms a)
  b  data.vot_clips(root, frames="files"), decode="host": a round's files decoded by Pillow on the pool threads, a round ahead
  c  the same clips, decode="device": a round's files decoded by ntk_jpeg_decode_batch on the decode stream, a round ahead

Clip lengths uniform in [8, 24] (profiles/validate.txt's), --clips-per-slot clips per slot, NTM 128 x 20 with random weights and
the fp32 trunk.  The first B * clips-per-slot sequences of one tree serve every B.  --big B T adds one arm on a second tree of
frames of twice the size on both axes.  Wall-clock time of one whole evaluate.validate to its result on the host, the device idle
before and after; the forms alternate pass by pass, pass 0 warms up, the figure is the median of the others with max - min beside
it.  --rss-form: ONE validation of one form at the largest B and T given, then the peak resident set of the process
(resource.getrusage; ru_maxrss is a high-water mark of the process and survives exec, so each form is started from a shell, in a
process of its own, not from this script).  profiles/validate_files.txt holds the output."""
import argparse
import os
import resource
import sys
import tempfile
import time

ap = argparse.ArgumentParser()
ap.add_argument("--B", nargs="+", type=int, default=[16, 64])
ap.add_argument("--T", nargs="+", type=int, default=[8, 24], help="frames per round")
ap.add_argument("--clips-per-slot", type=int, default=4)
ap.add_argument("--passes", type=int, default=3, help="timed passes per form after one warm-up pass")
ap.add_argument("--size", nargs=2, type=int, default=[360, 640], metavar=("H", "W"))
ap.add_argument("--big", nargs=2, type=int, default=None, metavar=("B", "T"), help="one arm at twice the frame size on both axes")
ap.add_argument("--forms", nargs="+", choices=["a", "b", "c"], default=["a", "b", "c"])
ap.add_argument("--root", default=os.path.dirname(os.path.dirname(os.path.abspath(__file__))), help="the checkout to import from")
ap.add_argument("--tree", default=None, help="write the VOT trees here and keep them (default: a temporary folder)")
ap.add_argument("--rss-form", choices=["a", "b", "c"], default=None, help="one validation of this form, then the process's peak resident set")
ap.add_argument("--commit", default="unknown")
ap.add_argument("--out", default=None, help="append the report to this file as well")
args = ap.parse_args()

sys.path.insert(0, os.path.abspath(args.root))
import numpy as np
import torch

from oracle import ntm_oracle as O
from ntmtrack import data, evaluate, online
from ntmtrack.ntm import NTMCell
from ntmtrack.vgg import VGG16Conv43

if not torch.cuda.is_available():
    sys.exit("dev_validate_files_timing.py measures on the GPU; none is visible")
dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


med = lambda v: sorted(v)[len(v) // 2]


def write_tree(root, n_clips, H, W, seed):
    """n_clips sequences <root>/sNNNN/{groundtruth.txt, %08d.jpg}: a smooth pattern under noise, shifted a little from frame to
    frame (every file different, of a photograph's size at quality 90); boxes that drift a few pixels per frame."""
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    rng = np.random.default_rng(seed)
    y, x = np.mgrid[0:H, 0:W]
    bases = []
    for k in range(8):
        ph = rng.uniform(0, 6.28, size=3)
        img = np.stack([127.5 + 90 * np.sin(ph[c] + x * (0.021 + 0.01 * c + 0.003 * k) + y * (0.017 + 0.006 * c)) for c in range(3)], axis=-1)
        bases.append(np.clip(img + rng.normal(0, 12, size=img.shape), 0, 255).astype(np.uint8))
    jobs, names = [], []
    for i in range(n_clips):
        name = "s%04d" % i
        names.append(name)
        os.makedirs(os.path.join(root, name))
        L = int(rng.integers(8, 25))
        wh = rng.uniform(40, 120, size=2) * (W / 640.0)
        start = np.concatenate([rng.uniform(0, 1, size=2) * (np.array([W, H]) - wh), wh])
        regions = start + np.cumsum(rng.uniform(-2, 2, size=(L, 4)), axis=0)
        with open(os.path.join(root, name, "groundtruth.txt"), "w") as f:
            f.write("".join("%.3f,%.3f,%.3f,%.3f\n" % tuple(r) for r in regions))
        jobs += [(os.path.join(root, name, "%08d.jpg" % (k + 1)), (i + k) % 8, 3 * k + i % 5, 2 * k) for k in range(L)]
    with open(os.path.join(root, "list.txt"), "w") as f:
        f.write("\n".join(names) + "\n")

    def write(job):
        path, base, dx, dy = job
        Image.fromarray(np.roll(bases[base], (dy, dx), axis=(0, 1))).save(path, "JPEG", quality=90, subsampling=2)
        return os.path.getsize(path)
    with ThreadPoolExecutor(max_workers=data.default_workers()) as pool:
        sizes = list(pool.map(write, jobs))
    return len(jobs), sum(sizes)


rng = np.random.default_rng(0)
vgg = VGG16Conv43(O.init_vgg_weights(rng), device=dev)
cell = NTMCell(2, mem_size=128, mem_dim=20, controller_hidden_size=200, controller_num_layers=1, write_head_size=1,
               read_head_size=4, input_dim=514, device=dev, init_scale=0.05, seed=1)
make = lambda images, regions: online.BatchNTMTracker(images, regions, cell, vgg, device=dev)


def clips_of(form, root, n):
    names = ["s%04d" % i for i in range(n)]
    return data.vot_clips(root, names) if form == "a" else data.vot_clips(root, names, frames="files")


def run(form, clips, B, T):
    kw = {} if form == "a" else {"decode": "host" if form == "b" else "device"}
    return evaluate.validate(make, clips, B, T, device=dev, **kw)


holder = None
if args.tree is None:
    holder = tempfile.TemporaryDirectory(prefix="ntmtrack_vot_")
    args.tree = holder.name
H, W = args.size
arms = [(os.path.join(args.tree, "%dx%d" % (W, H)), H, W, B, T) for B in args.B for T in args.T]
if args.big:
    arms.append((os.path.join(args.tree, "%dx%d" % (2 * W, 2 * H)), 2 * H, 2 * W, args.big[0], args.big[1]))
for root, h, w in sorted(set(a[:3] for a in arms)):
    if not os.path.isdir(root):
        n = args.clips_per_slot * max(a[3] for a in arms if a[0] == root)
        t0 = time.perf_counter()
        files, nbytes = write_tree(root, n, h, w, seed=h)
        say("tree %s: %d sequences, %d files, %.1f KB a file, written in %.1f s" % (os.path.basename(root), n, files, nbytes / files / 1e3,
                                                                                   time.perf_counter() - t0))
if args.rss_form:                                       # one validation of one form; the peak resident set of this process
    root, h, w, B, T = max((a for a in arms if a[1] == H), key=lambda a: (a[3], a[4]))
    before = resource.getrusage(resource.RUSAGE_SELF).ru_maxrss
    res = run(args.rss_form, clips_of(args.rss_form, root, args.clips_per_slot * B), B, T)
    torch.cuda.synchronize()
    say("peak resident set, form %s, one validation at %dx%d, B = %d, T = %d, %d clips: %.2f GB (%.2f GB before it: the package, the "
        "runtime, the cell and the trunk); mean overlap %.6f" % (args.rss_form, w, h, B, T, args.clips_per_slot * B,
                                                               resource.getrusage(resource.RUSAGE_SELF).ru_maxrss / 1e6, before / 1e6,
                                                               res["mean_overlap_frames"]))
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")
    sys.exit(0)
say("box: %s | torch %s | commit %s | package from %s | forms %s | %d clips per slot | %d timed passes after 1 warm-up | %d pool threads"
    % (torch.cuda.get_device_name(0), torch.__version__, args.commit, os.path.relpath(os.path.abspath(args.root)), " ".join(args.forms),
       args.clips_per_slot, args.passes, data.default_workers()))
say("%9s %3s %3s %5s %7s | %s" % ("frames", "B", "T", "clips", "obj.fr", " | ".join("%s %8s %9s %7s" % (f, "s", "obj.fr/s", "spread") for f in args.forms)))
for root, h, w, B, T in arms:
    n = args.clips_per_slot * B
    sets = {f: clips_of(f, root, n) for f in args.forms}
    tracked = sum(len(c.regions) - 1 for c in sets[args.forms[0]])
    times, values = {f: [] for f in args.forms}, {}
    for it in range(args.passes + 1):
        for f in args.forms:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            values[f] = run(f, sets[f], B, T)
            torch.cuda.synchronize()
            if it > 0:
                times[f].append(time.perf_counter() - t0)
    say("%9s %3d %3d %5d %7d | %s" % ("%dx%d" % (w, h), B, T, n, tracked, " | ".join(
        "%s %8.3f %9.0f %7.3f" % (f, med(times[f]), tracked / med(times[f]), max(times[f]) - min(times[f])) for f in args.forms)))
    say("          mean overlap: %s%s" % (", ".join("%s %.6f" % (f, values[f]["mean_overlap_frames"]) for f in args.forms),
                                          "".join("; %s decoded %d on the device, %d on the host" % (f, values[f]["decode"]["frames_on_device"],
                                                                                                   values[f]["decode"]["frames_on_host"])
                                                  for f in args.forms if "decode" in values[f])))
say("s: wall-clock seconds of one whole validation, median of the timed passes; spread: max - min of those passes (s); obj.fr: tracked frames.")
if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
