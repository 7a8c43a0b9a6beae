"""Time the deep-controller NTM cell (StackedNTMCell) fused against step-wise (dev tool; output: profiles/ntm_deep_controller.txt).

  * forward and BPTT per step at B 32, S 1300, the tracker's shape (mem 128x20, 4 read + 1 write head, hid 200, D 514), L = 2, 3
  * forward per step at the reference constructor's default controller (10 layers of 100; 3 read + 3 write heads)
  * NTMOffsetTracker(num_layers=2).loss_and_grads at B 32, T 20 (ms per call)
The step-wise form runs the same cell with ``fused = False``.

  dev_ntm_deep_timing.py [B] [--similarity as_coded|smooth_cosine] [--fused-only]
--fused-only times the fused form of L = 2, 3 alone (profiles/ntm_smooth_cosine.txt: both similarity modes)."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ntmtrack import tracker
from ntmtrack.ntm import NTMCell

ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=32)
ap.add_argument("--similarity", default="as_coded", choices=("as_coded", "smooth_cosine"))
ap.add_argument("--fused-only", action="store_true")
args = ap.parse_args()
dev = torch.device("cuda:0")
B = args.B
S = 1300


def ev():
    return torch.cuda.Event(enable_timing=True)


def time_cell(cell, D, S, bptt, iters):
    g = torch.Generator().manual_seed(0)
    X = torch.relu(torch.randn((B, S, (D + 3) // 4 * 4), generator=g)).to(dev)
    X[:, :, D:] = 0
    dlog = (torch.randn((B, S, cell.output_dim), generator=g) * 1e-2).to(dev)
    best_f, best_b = 1e30, 1e30
    for it in range(iters + 1):
        st0 = cell.zero_state(B)
        e = [ev() for _ in range(3)]
        e[0].record()
        _l, _o, _new, rec = cell.run_sequence(X, st0, record=bptt, want_outputs=False)
        e[1].record()
        if bptt:
            cell.backward_sequence(X, st0, rec, dlog)
        e[2].record()
        torch.cuda.synchronize()
        if it > 0:                                   # the first pass warms up (packing buffers, LDS attributes, code objects)
            best_f = min(best_f, e[0].elapsed_time(e[1]))
            best_b = min(best_b, e[1].elapsed_time(e[2]))
    return best_f * 1e3 / S, (best_b * 1e3 / S if bptt else None), cell.last_form


def cell_for(L, hid, R, Wh):
    return NTMCell(2, mem_size=128, mem_dim=20, shift_range=1, controller_hidden_size=hid, controller_num_layers=L,
                   write_head_size=Wh, read_head_size=R, input_dim=514, device=dev, init_scale=0.05, seed=1, similarity=args.similarity)


print("similarity = %s" % args.similarity)
print("B = %d, S = %d; us per step (best of the timed passes); BPTT = backward_sequence incl. the weight-gradient GEMMs" % (B, S))
print("%-44s %12s %12s %10s" % ("shape", "forward", "BPTT", "form"))
for L in (2, 3):
    c = cell_for(L, 200, 4, 1)
    rows = {}
    for fused in ((None,) if args.fused_only else (None, False)):
        c.fused = fused
        f, b, form = time_cell(c, 514, S, True, 3 if fused is None else 1)
        rows[form] = (f, b)
        print("%-44s %12.1f %12.1f %10s" % ("tracker shape, L=%d (hid 200, R4 W1)" % L, f, b, form), flush=True)
    if not args.fused_only:
        print("%-44s %11.1fx %11.1fx" % ("  step-wise / fused", rows["stepwise"][0] / rows["fused"][0], rows["stepwise"][1] / rows["fused"][1]))
if args.fused_only:
    sys.exit(0)
c = cell_for(10, 100, 3, 3)
rows = {}
for fused in (None, False):
    c.fused = fused
    f, _b, form = time_cell(c, 514, S, False, 3 if fused is None else 1)
    rows[form] = f
    print("%-44s %12.1f %12s %10s" % ("constructor default, L=10 (hid 100, R3 W3)", f, "-", form), flush=True)
print("%-44s %11.1fx" % ("  step-wise / fused", rows["stepwise"] / rows["fused"]))

T = 20
trk = tracker.NTMOffsetTracker(B, T, vgg_weights=None, num_layers=2, device=dev, seed=1, similarity=args.similarity)
g = torch.Generator().manual_seed(0)
fmap = torch.relu(torch.randn((B * T, 28, 28, 512), generator=g)).to(dev)
gts0 = torch.rand((B, 64), generator=g).to(dev)
offs = (torch.rand((B, T, 2), generator=g) - 0.5).to(dev)
print("NTMOffsetTracker(num_layers=2), B %d, T %d (S = %d): ms per loss_and_grads" % (B, T, T * 65))
for fused in (None, False):
    trk.cell.fused = fused
    best = 1e30
    for it in range(3 if fused is None else 2):
        e = [ev(), ev()]
        e[0].record()
        trk.loss_and_grads(fmap, gts0, offs)
        e[1].record()
        torch.cuda.synchronize()
        if it > 0:
            best = min(best, e[0].elapsed_time(e[1]))
    print("  %-10s %10.2f ms" % (trk.cell.last_form, best), flush=True)
