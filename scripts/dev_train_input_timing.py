"""Measurements of profiles/train_input.txt: the input path per 640-frame batch (the per-frame get_input against get_input_batch with
pack="full" / "rect") on synthetic 1280x720 JPEG frames written to a temporary directory, and train.fit's seconds per step with
and without the prefetcher.  Usage: python scripts/dev_train_input_timing.py   (N_FRAMES=... for another batch size)"""
import os
import sys
import tempfile
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from ntmtrack import data, tracker, train
from ntmtrack.geometry import discrete_gauss
from oracle import ntm_oracle as O

N = int(os.environ.get("N_FRAMES", "640"))
B, T = 32, 20
dev = torch.device("cuda:0")


def say(s):
    print(s, flush=True)


def median(xs):
    return float(np.median(xs))


tmp = tempfile.mkdtemp(prefix="ntk_frames_")
from PIL import Image
rng = np.random.default_rng(0)
t0 = time.perf_counter()
base = rng.integers(0, 256, size=(90, 160, 3), dtype=np.uint8)
nseq = N // T
seqs = []
hm = discrete_gauss((.5, .5), (8, 8), 1.0)
ARMS = os.environ.get("ARMS", "all")      # "device": only the device-decode arms (profiles/train_input_device_decode.txt)
SAVE_KW = {}                              # extra Image.save keywords of the frame set being written
SET_TAG = [""]


def write_seq(s):
    rng = np.random.default_rng(100 + s)
    d = os.path.join(tmp, "train_seq%03d%s_0" % (s, SET_TAG[0]))
    os.makedirs(d)
    stems = []
    for t in range(T):
        # a smooth image plus noise: JPEG of realistic size; the object (0.3 x 0.2 of the frame) drifts
        img = np.asarray(Image.fromarray(np.roll(base, (s * 7 + t, s * 3 + 2 * t), axis=(0, 1))).resize((1280, 720), Image.BILINEAR)).astype(np.int16)
        img = np.clip(img + rng.integers(-12, 13, size=img.shape), 0, 255).astype(np.uint8)
        jpg = os.path.join(d, "%06d.JPEG" % t)
        Image.fromarray(img).save(jpg, quality=90, **SAVE_KW)
        cy, cx, h, w = 0.4 + 0.01 * t, 0.45 + 0.005 * t, 0.3, 0.2
        k = 8.0 / 6.0          # cropbox_grid / bbox_grid of preprocess.py: the crop is the object scaled about its centre
        y1, x1, y2, x2 = cy - h * k / 2, cx - w * k / 2, cy + h * k / 2, cx + w * k / 2
        stem = os.path.join(d, "%06d" % t)
        hm.astype(np.float64).tofile(stem + ".bin")
        with open(stem + ".txt", "w") as f:
            f.write("%r,%r,%r,%r,0.3,0.3,0.6,0.6,%s,%r,%r" % (y1, x1, y2, x2, jpg, 0.0 if t == 0 else 0.01, 0.0 if t == 0 else -0.01))
        stems.append("%06d" % t)
    return (d, stems)


from concurrent.futures import ThreadPoolExecutor
with ThreadPoolExecutor(max_workers=data.default_workers()) as wp:
    seqs = list(wp.map(write_seq, range(nseq)))
say("wrote %d JPEG frames 1280x720 in %.1f s (mean %.0f kB)" % (nseq * T, time.perf_counter() - t0,
                                                               np.mean([os.path.getsize(os.path.join(s[0], "000000.JPEG")) for s in seqs]) / 1e3))
names = [os.path.join(d, st) for d, stems in seqs for st in stems]
n = len(names)
say("workers = %d (affinity %d)" % (data.default_workers(), len(os.sched_getaffinity(0))))

# ---- a second frame set: the same images written with a restart marker after every MCU row
SAVE_KW["restart_marker_rows"] = 1
SET_TAG[0] = "r"
with ThreadPoolExecutor(max_workers=data.default_workers()) as wp:
    seqs_rst = list(wp.map(write_seq, range(nseq)))
names_rst = [os.path.join(d, st) for d, stems in seqs_rst for st in stems]


def device_decode_arm(tag, names):
    """decode="device" per batch: host parse + unstuff on the decoder threads, bytes uploaded, the decode call (entropy + inverse
    DCT + colour kernels) and the crop kernel by event pairs, the whole call, against the host-decode call on the same frames."""
    pool = ThreadPoolExecutor(max_workers=data.default_workers())
    st = data.Staging()
    stage_times = []
    for rep in range(3):
        t0 = time.perf_counter()
        staged = data.stage_batch(names, None, pool, "rect", st, decode="device")
        stage_times.append(time.perf_counter() - t0)
    t0 = time.perf_counter()
    raw = list(pool.map(lambda nm: open(data.load_frame_record(nm)["image_path"], "rb").read(), names))
    t_read = time.perf_counter() - t0
    packed, j = staged.packed, staged.packed.jpeg
    up_bytes = j.stream_bytes + packed.n * data.JPEG_DESC_BYTES + 4 * j.n_segments + packed.table.numel() * 8
    ev = lambda: torch.cuda.Event(enable_timing=True)
    decs, crops = [], []
    mean = data._vgg_mean(dev)
    out = torch.empty((packed.n, 224, 224, 3), device=dev)
    L = data._lib.lib()
    for rep in range(13):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        pix, tab, status = data.decode_packed(packed, dev)                  # uploads + the three decode launches
        e1.record()
        box = packed.boxes.to(dev, non_blocking=True)
        data._lib.check(L.ntk_frames_crop_batch(data._lib.ptr(pix), packed.nbytes, data._lib.ptr(tab), data._lib.ptr(box), data._lib.ptr(mean),
                                                data._lib.ptr(out), packed.n, 3, 720, 1280, 224, 224, 0, 0.0, data._lib.stream()), "crop")
        e2.record()
        torch.cuda.synchronize()
        if rep >= 3:
            decs.append(e0.elapsed_time(e1))
            crops.append(e1.elapsed_time(e2))
    assert not status.cpu().numpy().any()
    walls = {}
    for decode in ("host", "device", "host", "device"):
        t0 = time.perf_counter()
        got = data.get_input_batch(names, device=dev, staging=st, decode=decode)
        torch.cuda.synchronize()
        walls.setdefault(decode, []).append(time.perf_counter() - t0)
        if decode == "host":
            ref = got[0]
    same = bool(torch.equal(got[0], ref)) and bool(torch.equal(out, ref))
    say("device decode [%s]: %d frames, %d on the device; restart segments per frame %.1f; file read %.3f s; stage (read + parse + unstuff, "
        "%d threads) %.3f s (median of 3; first %.3f); uploaded %.1f MB (streams %.1f MB) against %.1f MB of host-decoded rectangles; "
        "workspace %.1f MB; upload + decode kernels %.3f ms (event pairs, median of 10 after 3 warm-ups; min %.3f max %.3f); crop kernel "
        "%.3f ms; whole get_input_batch call: device %.3f s, host %.3f s (second of two calls each, alternating); bits equal: %s"
        % (tag, packed.n, sum(j.on_device), (j.n_segments - packed.n) / packed.n, t_read, data.default_workers(), median(stage_times),
           stage_times[0], up_bytes / 1e6, j.stream_bytes / 1e6, packed.nbytes / 1e6, j.workspace_bytes / 1e6, median(decs), min(decs),
           max(decs), median(crops), walls["device"][-1], walls["host"][-1], same))
    pool.shutdown()


device_decode_arm("no restart markers", names)
device_decode_arm("restart_marker_rows=1", names_rst)


def fit_arms(arms):
    ws = O.init_vgg_weights(np.random.default_rng(0))
    for tag, frame_seqs, kw in arms:
        trk = tracker.NTMOffsetTracker(B, T, vgg_weights=ws, device=dev, seed=1)
        stamps = []
        # num_epochs epochs of the same sequences: each epoch is nseq // B steps; validation far apart, one loss read at the end
        t0 = time.perf_counter()
        res = train.fit(trk, frame_seqs, frame_seqs[:B], num_epochs=6, validation_interval=10 ** 6, validation_batch=1,
                        log_interval=10 ** 6, ckpt_dir=os.path.join(tmp, "ckpt"), seed=0,
                        on_event=lambda e: stamps.append((e[0], time.perf_counter())), **kw)
        torch.cuda.synchronize()
        per = np.diff([t for k, t in stamps if k == "train"])
        say("fit %s: %d steps of B=%d T=%d; seconds per step: median %.3f, min %.3f, max %.3f (host time between steps; first "
            "step excluded); whole run %.1f s" % (tag, res.steps, B, T, median(per), per.min(), per.max(), time.perf_counter() - t0))
        del trk


if ARMS == "device":
    fit_arms([("decode=host", seqs, dict(decode="host")), ("decode=device", seqs, dict(decode="device")),
              ("decode=host", seqs, dict(decode="host")), ("decode=device", seqs, dict(decode="device")),
              ("decode=host, restart rows", seqs_rst, dict(decode="host")), ("decode=device, restart rows", seqs_rst, dict(decode="device"))])
    import shutil
    shutil.rmtree(tmp, ignore_errors=True)
    sys.exit(0)

# ---- the per-frame path
torch.cuda.synchronize()
t0 = time.perf_counter()
recs = [data.load_frame_record(nm) for nm in names]
imgs = [data._decode_image(r["image_path"]) for r in recs]
t_dec = time.perf_counter() - t0
t0 = time.perf_counter()
ref = data.get_input(names, device=dev)
torch.cuda.synchronize()
t_all = time.perf_counter() - t0
say("get_input (per frame): %d frames: decode alone (one thread, fp32) %.3f s; whole call %.3f s; uploaded %.1f MB fp32 pageable; "
    "launches %d" % (n, t_dec, t_all, sum(i.size for i in imgs) * 4 / 1e6, 2 * n))
del imgs

# ---- the batched path
from concurrent.futures import ThreadPoolExecutor
pool = ThreadPoolExecutor(max_workers=data.default_workers())
for pack in ("full", "rect"):
    st = data.Staging()
    t0 = time.perf_counter()
    loaded = list(pool.map(lambda nm: data._load_frame(nm, None), names))
    t_dec = time.perf_counter() - t0
    packs = []
    for rep in range(3):
        t0 = time.perf_counter()
        packed = data.pack_frames([i for _r, i in loaded], [r["cropbox"] for r, _i in loaded], pack=pack, staging=st)
        packs.append(time.perf_counter() - t0)
    ev = lambda: torch.cuda.Event(enable_timing=True)
    ups, kers = [], []
    mean = data._vgg_mean(dev)
    res = torch.empty((n, 224, 224, 3), device=dev)
    L = data._lib.lib()
    for rep in range(13):
        e0, e1, e2 = ev(), ev(), ev()
        e0.record()
        pix = packed.pixels.to(dev, non_blocking=True)
        tab = packed.table.to(dev, non_blocking=True)
        box = packed.boxes.to(dev, non_blocking=True)
        e1.record()
        data._lib.check(L.ntk_frames_crop_batch(data._lib.ptr(pix), packed.nbytes, data._lib.ptr(tab), data._lib.ptr(box), data._lib.ptr(mean),
                                                data._lib.ptr(res), n, 3, 720, 1280, 224, 224, 0, 0.0, data._lib.stream()), "crop")
        e2.record()
        torch.cuda.synchronize()
        if rep >= 3:
            ups.append(e0.elapsed_time(e1))
            kers.append(e1.elapsed_time(e2))
    same = bool(torch.equal(res, ref[0]))
    t0 = time.perf_counter()
    got = data.get_input_batch(names, device=dev, pack=pack, staging=st)
    torch.cuda.synchronize()
    t_call = time.perf_counter() - t0
    say("get_input_batch pack=%s: decode (%d threads, uint8) %.3f s; pack %.3f s (median of 3; first %.3f); uploaded %.1f MB pinned; "
        "upload %.3f ms, kernel %.3f ms (event pairs, median of 10 after 3 warm-ups; min %.3f max %.3f); whole call %.3f s; "
        "bits equal to get_input: %s" % (pack, data.default_workers(), t_dec, median(packs), packs[0], packed.nbytes / 1e6, median(ups),
                                         median(kers), min(kers), max(kers), t_call, same and bool(torch.equal(got[0], ref[0]))))
    del loaded
pool.shutdown()
del ref, res, got

# ---- fit: seconds per step with and without the prefetcher
ws = O.init_vgg_weights(np.random.default_rng(0))
for prefetch in (True, False):
    trk = tracker.NTMOffsetTracker(B, T, vgg_weights=ws, device=dev, seed=1)
    stamps = []
    # num_epochs epochs of the same sequences: each epoch is nseq // B steps; validation far apart, one loss read at the end
    t0 = time.perf_counter()
    res = train.fit(trk, seqs, seqs[:B], num_epochs=6, validation_interval=10 ** 6, validation_batch=1, log_interval=10 ** 6,
                    ckpt_dir=os.path.join(tmp, "ckpt"), seed=0, prefetch=prefetch,
                    on_event=lambda e: stamps.append((e[0], time.perf_counter())))
    torch.cuda.synchronize()
    ts = [t for k, t in stamps if k == "train"]
    per = np.diff(ts)
    say("fit prefetch=%s: %d steps of B=%d T=%d; seconds per step: median %.3f, min %.3f, max %.3f (host time between steps; first "
        "step excluded); whole run %.1f s" % (prefetch, res.steps, B, T, median(per), per.min(), per.max(), time.perf_counter() - t0))
    del trk
import shutil
shutil.rmtree(tmp, ignore_errors=True)
