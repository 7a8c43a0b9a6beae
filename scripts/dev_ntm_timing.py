"""Time the NTM sequence forward / BPTT kernels at a benchmark shape (dev tool).

  dev_ntm_timing.py [B [T]] [--similarity as_coded|smooth_cosine] [--iters N]
The last line is the median over the iterations after the first (which warms up); profiles/ntm_smooth_cosine.txt holds it for both modes."""
import argparse, sys, os
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import torch
from ntmtrack import tracker
ap = argparse.ArgumentParser()
ap.add_argument("B", nargs="?", type=int, default=32)
ap.add_argument("T", nargs="?", type=int, default=20)
ap.add_argument("--similarity", default="as_coded", choices=("as_coded", "smooth_cosine"))
ap.add_argument("--iters", type=int, default=3)
args = ap.parse_args()
B, T = args.B, args.T
dev = torch.device("cuda:0")
trk = tracker.NTMOffsetTracker(B, T, vgg_weights=None, device=dev, seed=1, similarity=args.similarity)
print("similarity %s: plan %s" % (args.similarity, trk.cell.plan(B)))
g = torch.Generator().manual_seed(0)
fmap = torch.relu(torch.randn((B * T, 28, 28, 512), generator=g)).to(dev)
gts0 = torch.rand((B, 64), generator=g).to(dev)
offs = (torch.rand((B, T, 2), generator=g) - 0.5).to(dev)
def ev(): return torch.cuda.Event(enable_timing=True)
fwd_us, bwd_us = [], []
for it in range(args.iters):
    e = [ev() for _ in range(5)]
    e[0].record()
    X = trk.serialize(fmap, gts0); st0 = trk.cell.zero_state(B)
    e[1].record()
    logits, _o, new, rec = trk.cell.run_sequence(X, st0, record=True, want_outputs=False)
    e[2].record()
    loss, pred, dlog = tracker.offset_loss(logits, offs, T)
    g0 = trk.cell.backward_sequence(X, st0, rec, dlog); trk.cell.init_state_backward(g0, B)
    e[3].record()
    trk.opt.step()
    e[4].record(); torch.cuda.synchronize()
    S = T * 65
    print("iter %d: serialize %.3f ms | fwd(xproj+seq) %.3f ms (%.2f us/step) | loss+bwd+wgrad %.3f ms (%.2f us/step) | opt %.3f ms | loss %.5f"
          % (it, e[0].elapsed_time(e[1]), e[1].elapsed_time(e[2]), e[1].elapsed_time(e[2]) * 1e3 / S,
             e[2].elapsed_time(e[3]), e[2].elapsed_time(e[3]) * 1e3 / S, e[3].elapsed_time(e[4]), float(loss.cpu())), flush=True)
    if it > 0:
        fwd_us.append(e[1].elapsed_time(e[2]) * 1e3 / S)
        bwd_us.append(e[2].elapsed_time(e[3]) * 1e3 / S)
if fwd_us:
    med = lambda v: sorted(v)[len(v) // 2]
    print("median of %d: %s B %d S %d forward %.2f us/step, loss+BPTT+wgrad %.2f us/step" % (len(fwd_us), args.similarity, B, T * 65, med(fwd_us), med(bwd_us)))
