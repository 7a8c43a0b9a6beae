"""Time the repeat-copy task (dev tool; profiles/repeat_copy.txt holds its output).

  dev_repeat_copy_timing.py [--windows 3] [--steps 500] [--calls 500] [--train-seconds 60] [--out FILE]

One process.  Every figure is a host clock around work that ends in a device synchronise, over `windows` timed windows after a warm-up
of every shape the windows use (a batch's step count S takes the values 5, 6, 7 and 9 on train.py's task; the warm-up runs 100 steps);
the figure is the median window, the spread max - min over the windows.
  1. train_step of the default task (train.py's flags: bits 4, length 1-2, repeats 1-2, B 16; DNC 16 x 16, 1 read, 1 write, 64 hidden).
  2. one RepeatCopy() call (host sampling + device bits + the pack launch) against building the same batch with torch indexing ops on
     the device, sequence by sequence, the way copy_task.make_batch builds its batch (lengths known on the host in both).
  3. one train() run at the reference's learning rate (1e-4) for --train-seconds: its reported mean losses."""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

ap = argparse.ArgumentParser()
ap.add_argument("--windows", type=int, default=3)
ap.add_argument("--steps", type=int, default=500)
ap.add_argument("--calls", type=int, default=500)
ap.add_argument("--train-seconds", type=float, default=60.0)
ap.add_argument("--out", default=None)
args = ap.parse_args()

from ntmtrack.repeat_copy import RepeatCopy, RepeatCopyTask, train      # noqa: E402

dev = torch.device("cuda:0")
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def windows(fn, n):
    """fn() n times per window, args.windows windows -> seconds per call of each window."""
    out = []
    for _ in range(args.windows):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) / n)
    return out


def fmt(ws, unit=1e6, name="us"):
    return "median %.1f %s, spread %.1f (windows: %s)" % (np.median(ws) * unit, name, (max(ws) - min(ws)) * unit,
                                                           ", ".join("%.1f" % (w * unit) for w in ws))


def torch_batch(ds, bits, lengths, repeats):
    """The same batch with torch indexing ops on the device (zeros, then slice assignments per sequence)."""
    B, nb = bits.shape[0], ds.num_bits
    S = max(L * (r + 1) + 3 for L, r in zip(lengths, repeats))
    X = torch.zeros((B, S, ds.ldx), device=dev)
    T = torch.zeros((B, S, nb + 1), device=dev)
    M = torch.zeros((B, S), device=dev)
    X[:, 0, nb] = 1.0
    for b, (L, r) in enumerate(zip(lengths, repeats)):
        X[b, 1:1 + L, :nb] = bits[b, :L]
        X[b, L + 1, nb + 1] = r / ds.norm_max
        T[b, L + 2:L + 2 + L * r, :nb] = bits[b, :L].repeat(r, 1)
        T[b, L + 2 + L * r, nb] = 1.0
        M[b, L + 2:L + 3 + L * r] = 1.0
    return X, T, M


mk = lambda seed: RepeatCopy(num_bits=4, batch_size=16, min_length=1, max_length=2, min_repeats=1, max_repeats=2, device=dev, seed=seed)
say("repeat-copy timing: %s, torch %s, %d windows" % (torch.cuda.get_device_name(0), torch.__version__, args.windows))

# 1. the default task's training step
task = RepeatCopyTask(mk(0), "dnc", seed=0)
for _ in range(100):
    task.train_step()
task.check_step()
ws = windows(task.train_step, args.steps)
task.check_step()
say("1. train_step, default task (B 16, S 5..9, DNC 16x16 R1 W1 hidden 64), %d steps per window: %s; %.0f steps/s"
    % (args.steps, fmt(ws), 1.0 / np.median(ws)))

# 2. one batch: RepeatCopy() against torch indexing ops
ds = mk(1)
for _ in range(20):
    ds()
wa = windows(ds, args.calls)
ds2 = mk(2)


def by_torch():
    lengths, repeats = ds2.sample_lengths()
    bits = torch.empty((16, 2, 4), device=dev).random_(0, 2, generator=ds2._device_gen())
    return torch_batch(ds2, bits, lengths.tolist(), repeats.tolist())


for _ in range(20):
    by_torch()
wb = windows(by_torch, args.calls)
# the two build the same thing
lengths, repeats = ds2.sample_lengths()
bits = torch.empty((16, 2, 4), device=dev).random_(0, 2, generator=ds2._device_gen())
ref = torch_batch(ds2, bits, lengths.tolist(), repeats.tolist())
got = ds2.from_arrays(bits, lengths, repeats)
same = all(torch.equal(a, b) for a, b in zip(ref, (got.X, got.target_bm, got.mask_bm)))
say("2. one batch (B 16), %d calls per window: RepeatCopy() %s; torch indexing ops %s; ratio of medians %.1f; same batch: %s"
    % (args.calls, fmt(wa), fmt(wb), np.median(wb) / np.median(wa), same))

# 3. a train() run at the reference's learning rate
task = RepeatCopyTask(mk(3), "dnc", learning_rate=1e-4, seed=3)
curve, t0, n = [], time.perf_counter(), 0
while time.perf_counter() - t0 < args.train_seconds:
    n += 1000
    curve += train(task, n, 500, log=lambda s: None)
say("3. train() at learning rate 1e-4, %d iterations in %.0f s; mean loss of every 500 iterations:" % (n, time.perf_counter() - t0))
for i in range(0, len(curve), 10):
    say("   %6d: %s" % ((i + 1) * 500, " ".join("%.4f" % v for v in curve[i:i + 10])))
_loss, ber, perfect = task.eval(8, mk(1234))
say("   after it: bit error rate %.4f, sequences copied without a wrong bit %.3f (8 batches of 16 from another seed)" % (ber, perfect))

if args.out:
    with open(args.out, "a") as f:
        f.write("\n".join(lines) + "\n")
