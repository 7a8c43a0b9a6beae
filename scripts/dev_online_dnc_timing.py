"""Time online DNC tracking of B objects: the loop the public API allowed before online.BatchDNCTracker -- B independent Python
loops over DNC.run_sequence(X, prev_state) with online.crop_and_resize, the trunk, the online serialiser and host box
arithmetic -- against one online.BatchDNCTracker.track_clip (dev tool).

  dev_online_dnc_timing.py [--cores c2 c5] [--B 1 16 64] [--repeats 5] [--frames 20] [--size 360 640] [--commit ID] [--out FILE]
  dev_online_dnc_timing.py --child loop|batch --core c2|c5 --B n          (one measurement, one JSON line; what the driver starts)

Every measurement is a process of its own (one warm-up clip, one timed clip); for every (core, B) the two forms alternate,
`repeats` processes each, and the figure is the median, the spread max - min over those processes.  640 x 360 uint8 frames
resident on the device for both forms, B objects in one video, 20 frames per clip, random weights.  Cores: c2 = benchmark
config 2 (memory 256 x 64), c5 = config 5 (512 x 128); 4 read heads, 1 write head, 200 hidden units.  The batched child also
times the same clip with every other tracker inactive on every frame and reports what ntk_dnc_state_keep moved.
profiles/online_dnc.txt holds the output."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

CORES = {"c2": dict(memory_size=256, word_size=64), "c5": dict(memory_size=512, word_size=128)}
HBM_BYTES_PER_S = 8e12

ap = argparse.ArgumentParser()
ap.add_argument("--cores", nargs="+", default=["c2", "c5"], choices=sorted(CORES))
ap.add_argument("--B", nargs="+", type=int, default=[1, 16, 64])
ap.add_argument("--repeats", type=int, default=5, help="processes per form and (core, B)")
ap.add_argument("--frames", type=int, default=20)
ap.add_argument("--size", nargs=2, type=int, default=[360, 640], metavar=("H", "W"))
ap.add_argument("--commit", default="unknown")
ap.add_argument("--out", default=None, help="append the report to this file as well")
ap.add_argument("--child", choices=["loop", "batch"], default=None)
ap.add_argument("--core", default="c2", choices=sorted(CORES))
args = ap.parse_args()
H, W = args.size
T = args.frames


def regions_for(B):
    import numpy as np
    r = np.random.default_rng(100 + B)
    wh = r.uniform(40, 120, size=(B, 2))
    xy = r.uniform(0, 1, size=(B, 2)) * (np.array([W, H]) - wh)
    return np.concatenate([xy, wh], axis=1)


def child():
    import numpy as np
    import torch
    from oracle import ntm_oracle as O
    from ntmtrack import _lib, geometry as G, online
    from ntmtrack.dnc import DNC
    from ntmtrack.vgg import VGG16Conv43
    if not torch.cuda.is_available():
        sys.exit("dev_online_dnc_timing.py measures on the GPU; none is visible")
    dev = torch.device("cuda:0")
    B = args.B[0]
    vgg = VGG16Conv43(O.init_vgg_weights(np.random.default_rng(0)), device=dev)
    core = DNC(dict(CORES[args.core], num_reads=4, num_writes=1), {"hidden_size": 200}, 2, 20, input_dim=514, device=dev, seed=1)
    core.WxT.mul_(0.05)                                    # trunk features are O(10): keep the gates off saturation
    clip = torch.randint(0, 256, (T + 1, 1, H, W, 3), dtype=torch.uint8, device=dev, generator=torch.Generator(dev).manual_seed(B))
    regions = regions_for(B)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    P = _lib.ptr

    class Loop(object):
        """One object on the public API as it was before the batched tracker: the state is a DNCState handed from call to call."""

        def __init__(self, image, region):
            self.size = (image.shape[1], image.shape[0])
            self._boxes(region)
            self.state = None
            self._frame(image, True)

        def _boxes(self, region):
            x1, y1, w, h = region
            self.nb = G.normalize_bbox(self.size, (y1, x1, y1 + h, x1 + w))
            self.cb = G.calculate_cropbox(self.nb, 8, 6)
            self.tr = G.calculate_transformation(self.cb)

        def _frame(self, image, first):
            crop = online.crop_and_resize(image.to(torch.float32), self.cb)
            fmap = vgg(crop.unsqueeze(0), latency=True)
            gts0 = None
            if first:
                gt = G.generate_gt(G.apply_transformation(self.nb, self.tr), 8, 6)
                gts0 = torch.as_tensor(gt.reshape(1, -1), dtype=torch.float32).to(dev).contiguous()
            X = torch.empty((1, 65, core.ldx), device=dev)
            _lib.check(_lib.lib().ntk_gather_serialize_online(P(fmap), None if gts0 is None else P(gts0), P(X), 1, 1, 28, 28, 512,
                                                              core.ldx, 6, 2, 8, _lib.stream()), "ntk_gather_serialize_online")
            out, self.state = core.run_sequence(X[:, :, :core.D].transpose(0, 1), self.state)
            return out[-1, 0]

        def track(self, image):
            off = torch.tanh(self._frame(image, False)).cpu().numpy()
            y1, x1, y2, x2 = G.apply_transformation(G.offset_bbox([.125, .125, .875, .875], off), np.linalg.inv(self.tr))
            w, h = self.size
            region = (x1 * w, y1 * h, (x2 - x1) * w, (y2 - y1) * h)
            self._boxes(region)
            return region

    def loop_clip():
        trks = [Loop(clip[0, 0], tuple(r)) for r in regions]
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        for t in range(1, T + 1):
            for trk in trks:
                trk.track(clip[t, 0])
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / T

    def batch_clip(active=None):
        trk = online.BatchDNCTracker(clip[0], regions, core, vgg, device=dev)
        torch.cuda.synchronize()
        e0, e1 = ev(), ev()
        e0.record()
        trk.track_clip(clip[1:], active=active)
        e1.record()
        torch.cuda.synchronize()
        trk.check()
        return e0.elapsed_time(e1) / T, trk

    res = {"form": args.child, "core": args.core, "B": B, "box": torch.cuda.get_device_name(0), "torch": torch.__version__}
    if args.child == "loop":
        loop_clip()
        res["ms_per_frame"] = loop_clip()
    else:
        batch_clip()
        res["ms_per_frame"], trk = batch_clip()
        # every other tracker inactive on every frame (alternating from frame to frame): two keep launches per frame
        mask = (torch.arange(B, device=dev)[None, :] + torch.arange(T, device=dev)[:, None]) % 2
        mask = mask.to(torch.uint8).contiguous()
        batch_clip(mask)
        res["ms_per_masked_frame"], trk = batch_clip(mask)
        row_bytes = 4 * sum(trk.state.row_floats())
        inactive = float((mask == 0).sum()) / T
        res["state_bytes_per_object"] = row_bytes
        res["keep_bytes_per_masked_frame"] = 2 * 2 * inactive * row_bytes          # two launches, each reads and writes the row
    res["family"] = core.last_cluster_form or "seq"
    res["k"] = core.last_cluster_k
    print("RESULT " + json.dumps(res), flush=True)


def driver():
    lines = []

    def say(s):
        print(s, flush=True)
        lines.append(s)

    def run(form, core, B):
        cmd = [sys.executable, os.path.abspath(__file__), "--child", form, "--core", core, "--B", str(B), "--frames", str(T),
               "--size", str(H), str(W)]
        out = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.STDOUT, text=True, timeout=600)
        got = [l for l in out.stdout.splitlines() if l.startswith("RESULT ")]
        if out.returncode != 0 or not got:
            sys.exit("child %s failed (%d):\n%s" % (" ".join(cmd[2:]), out.returncode, out.stdout[-4000:]))
        res = json.loads(got[-1][7:])
        print("  %s %s B=%d: %.3f ms per frame (%s k=%d)" % (form, core, B, res["ms_per_frame"], res["family"], res["k"]), flush=True)
        return res

    med = lambda v: sorted(v)[len(v) // 2]
    spread = lambda v: max(v) - min(v)
    first = True
    for core in args.cores:
        for B in args.B:
            loop, batch = [], []
            for _ in range(args.repeats):                        # the two forms alternate, process by process
                loop.append(run("loop", core, B))
                batch.append(run("batch", core, B))
            if first:
                say("box: %s | torch %s | commit %s | frames %dx%d uint8 | %d frames per clip | %d processes per form, each 1 warm-up "
                    "clip + 1 timed clip" % (batch[0]["box"], batch[0]["torch"], args.commit, W, H, T, args.repeats))
                say("%4s %3s | %30s | %30s | %6s | %28s | %s" % ("core", "B", "loop over DNC.run_sequence", "BatchDNCTracker.track_clip",
                                                                "ratio", "masked clip (half inactive)", "ntk_dnc_state_keep per masked frame"))
                say("%4s %3s | %9s %8s %11s | %9s %8s %11s | %6s | %9s %8s %9s | %s"
                    % ("", "", "ms/frame", "spread", "family", "ms/frame", "spread", "family", "", "ms/frame", "spread", "extra ms",
                       "MB moved, time at 8 TB/s, share of the extra"))
                first = False
            l, b, m = [r["ms_per_frame"] for r in loop], [r["ms_per_frame"] for r in batch], [r["ms_per_masked_frame"] for r in batch]
            fam = lambda r: "%s k=%d" % (r[0]["family"], r[0]["k"])
            moved = batch[0]["keep_bytes_per_masked_frame"]
            extra = med(m) - med(b)
            ideal_ms = 1e3 * moved / HBM_BYTES_PER_S
            say("%4s %3d | %9.3f %8.3f %11s | %9.3f %8.3f %11s | %5.2fx | %9.3f %8.3f %9.3f | %.2f MB, %.4f ms, %s"
                % (core, B, med(l), spread(l), fam(loop), med(b), spread(b), fam(batch), med(l) / med(b), med(m), spread(m), extra,
                   moved / 1e6, ideal_ms, ("%.0f %%" % (100 * ideal_ms / extra)) if extra > 0 else "extra <= 0"))
    say("ms/frame: one frame of all B objects; median over the processes of a form, spread: max - min over them; ratio: loop / batched;")
    say("extra ms: masked - unmasked batched frame (two ntk_dnc_state_keep launches); MB moved: bytes read + written by both launches.")
    if args.out:
        with open(args.out, "a") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    child() if args.child else driver()
