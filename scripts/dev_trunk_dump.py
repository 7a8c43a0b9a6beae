"""Dev: dump what the VGG trunk computes in every form, for comparing two versions of the host code (or of the library) byte for byte.
    dev_trunk_dump.py OUT.npz           seeded weights and frames of (2, 64, 96), (2, 64, 64) and (4, 224, 224) -- the smallest frames
                                        that take the mixed split / F(4x4) route and the all-split route, and the workload's -- through
                                        the default, winograd, winograd nhwc, winograd2, direct, bf16 patch and bf16 tile trunks: the
                                        conv4_3 map of a plain call, of a latency=True call and of a call under a features window; for the
                                        fp32 trunks also forward_chunk up to conv1_2 and conv3_3
    dev_trunk_dump.py --compare A B     compare two dumps: every tensor must be equal byte for byte (Python only decides which entry is
                                        called with which pointers: any difference is a wrong route, not rounding)
NTK_LIB_PATH selects the library (one process per tree)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np

SHAPES = ((2, 64, 96), (2, 64, 64), (4, 224, 224))


def compare(pa, pb):
    A, B = np.load(pa), np.load(pb)
    assert sorted(A.files) == sorted(B.files), "the dumps hold different tensors"
    differ = 0
    for k in sorted(A.files):
        a, b = A[k], B[k]
        if a.shape != b.shape or a.tobytes() != b.tobytes():
            differ += 1
            print("DIFFERS %-50s %s" % (k, "shapes %s %s" % (a.shape, b.shape) if a.shape != b.shape else "max|a-b| %.3e" % np.max(np.abs(a - b))))
    print("%d tensors, %d differ" % (len(A.files), differ))
    return 1 if differ else 0


def dump(path):
    import torch
    from oracle import ntm_oracle as O
    from ntmtrack import vgg
    dev = torch.device("cuda:0")
    rng = np.random.default_rng(41)
    ws = O.init_vgg_weights(rng)
    for k in ws:
        ws[k] = (ws[k][0], (rng.standard_normal(ws[k][1].shape) * 0.05).astype(np.float32))
    nets = {"default": vgg.VGG16Conv43(ws, device=dev)}
    for algo in ("winograd", "winograd2", "direct"):
        nets[algo] = vgg.VGG16Conv43(ws, device=dev, algo=algo)
    nets["winograd nhwc"] = vgg.VGG16Conv43(ws, device=dev, algo="winograd")
    nets["winograd nhwc"].layout = "nhwc"
    for form in ("patch", "tile"):
        nets["bf16 " + form] = vgg.VGG16Conv43(ws, device=dev, dtype="bf16")
        nets["bf16 " + form].bf16_form = form
    out = {}
    for F, H, W in SHAPES:
        x = torch.from_numpy(np.random.default_rng(H * 1000 + W).uniform(0, 255, size=(F, H, W, 3)).astype(np.float32) - O.VGG_MEAN).to(dev)
        for name, net in nets.items():
            tag = "%dx%dx%d/%s/" % (F, H, W, name)
            out[tag + "plain"] = net(x).cpu().numpy()
            out[tag + "latency"] = net(x, latency=True).cpu().numpy()
            net.features_window = (4, 4, min(24, H // 8), min(24, W // 8))
            out[tag + "window"] = net(x).cpu().numpy()
            net.features_window = None
            if net.dtype == "f32":
                for upto in ("conv1_2", "conv3_3"):
                    out[tag + upto] = net.forward_chunk(x, upto=upto).cpu().numpy()
            torch.cuda.synchronize()
            print(tag + " done", flush=True)
    np.savez(path, **out)
    print("%d tensors -> %s" % (len(out), path))
    return 0


if __name__ == "__main__":
    sys.exit(compare(sys.argv[2], sys.argv[3]) if sys.argv[1] == "--compare" else dump(sys.argv[1]))
