"""Dev: dump what the VGG trunk computes in every form, for comparing two versions of the host code (or of the library) byte for byte.
    dev_trunk_dump.py OUT.npz           seeded weights and frames of (2, 64, 96), (2, 64, 64) and (4, 224, 224) -- the smallest frames
                                        that take the mixed split / F(4x4) route and the all-split route, and the workload's -- through
                                        the default, winograd, winograd nhwc, winograd2, direct, bf16 patch and bf16 tile trunks: the
                                        conv4_3 map of a plain call, of a latency=True call and of a call under a features window; for the
                                        fp32 trunks also forward_chunk up to conv1_2 and conv3_3
    dev_trunk_dump.py --layers OUT.npz  single layers of three frames with seeded inputs, small enough that sub-block groups cross frame
                                        boundaries, in every tile-block shape of the tiled conv kernels (csrc/conv_tiles.h) and every
                                        column-block count of the workgroup map (cout / 64 = 1, 2, 8, 16): F(4x4) on four and eight waves
                                        in all layout pairs and under two windows (output preset to NaN: what a window call leaves
                                        alone shows), F(2x2), the split and the bf16 patch form
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


def dump_layers(path):
    import torch
    from ntmtrack import vgg
    dev = torch.device("cuda:0")
    out = {}

    def layer(H, W, cin, cout):
        rng = np.random.default_rng(((H * 100 + W) * 100 + cin) * 10000 + cout)
        x, w, b = rng.standard_normal((3, H, W, cin)), rng.standard_normal((3, 3, cin, cout)) * 0.1, rng.standard_normal(cout) * 0.1
        return [torch.from_numpy(v.astype(np.float32)).to(dev) for v in (x, w, b)]

    def keep(tag, t):
        out[tag] = (t.view(torch.int16) if t.dtype == torch.bfloat16 else t).cpu().numpy()

    # F(4x4): whole frames pooled and un-pooled, and two frames under a window only (28x28: single tiles; 32x32: 2x2x8 blocks with
    # a nonzero origin)
    WHOLE = ((16, 32), (16, 16), (8, 8), (12, 12), (28, 28))
    WINDOW = {(28, 28): (4, 4, 24, 24), (32, 32): (8, 8, 24, 24)}
    for cin, cout in ((32, 64), (16, 128), (16, 512), (64, 1024)):
        for H, W in WHOLE + ((32, 32),):
            x, w, b = layer(H, W, cin, cout)
            u, xb = vgg.pack_weights_wino43(w), vgg.nhwc_to_blocked(x)
            tag = "wino43/%dx%d/%d-%d/" % (H, W, cin, cout)
            for waves in (4, 8):
                if (H, W) in WINDOW:
                    nan = torch.full((3, H, W, cout), float("nan"), device=dev)
                    keep(tag + "w%d window" % waves, vgg.conv3x3_relu_wino43(x, u, b, cin, cout, out=nan, window=WINDOW[(H, W)], waves=waves))
                if (H, W) not in WHOLE:
                    continue
                for pool in (False, True):
                    keep(tag + "w%d pool%d" % (waves, pool), vgg.conv3x3_relu_wino43(x, u, b, cin, cout, fuse_pool=pool, waves=waves))
                    if waves == 8:
                        for inb, outb in ((0, 1), (1, 0), (1, 1)):
                            keep(tag + "blocked%d%d pool%d" % (inb, outb, pool),
                                 vgg.conv3x3_relu_wino43_blocked(xb if inb else x, u, b, cin, cout, fuse_pool=pool, out_blocked=bool(outb)))
    for cin, cout in ((32, 64), (16, 512)):
        for H, W in ((8, 16), (8, 8), (12, 12)):
            x, w, b = layer(H, W, cin, cout)
            for pool in (False, True):
                keep("wino/%dx%d/%d-%d/pool%d" % (H, W, cin, cout, pool), vgg.conv3x3_relu_wino(x, vgg.pack_weights_wino(w), b, cin, cout, fuse_pool=pool))
    for cin, cout in ((64, 64), (32, 128), (64, 1024)):
        four = (cin, cout) == (64, 64)                                  # the four-wave form: its one-sub-block shape is 32 x 8
        for H, W in ((8, 32) if four else (16, 32), (16, 16), (8, 8), (20, 28), (28, 28), (12, 12)):
            x, w, b = layer(H, W, cin, cout)
            tag = "%%s/%dx%d/%d-%d/" % (H, W, cin, cout)
            pools = (False, True) if H % 8 == 0 else (False,)              # the pool needs sides that are multiples of 8
            for pool in pools:
                for f32 in (False, True):
                    if W != 12:
                        wp = vgg.pack_weights_split3(w, H, W)
                        keep(tag % "split3" + "pool%d f32out%d" % (pool, f32), vgg.conv3x3_relu_split3(vgg.to_split(x), wp, b, cin, cout, fuse_pool=pool, out_f32=f32))
                        if four and H % 8 == 0:
                            keep(tag % "split3 f32in" + "pool%d f32out%d" % (pool, f32), vgg.conv3x3_relu_split3(x, wp, b, cin, cout, fuse_pool=pool, out_f32=f32))
                    if W != 28:
                        keep(tag % "bf16p" + "pool%d f32out%d" % (pool, f32),
                             vgg.conv3x3_relu_bf16p(x.to(torch.bfloat16), vgg.pack_weights_bf16p(w, H, W), b, cin, cout, fuse_pool=pool, out_f32=f32))
    torch.cuda.synchronize()
    np.savez(path, **out)
    print("%d tensors -> %s" % (len(out), path))
    return 0


if __name__ == "__main__":
    if sys.argv[1] == "--compare":
        sys.exit(compare(sys.argv[2], sys.argv[3]))
    sys.exit(dump_layers(sys.argv[2]) if sys.argv[1] == "--layers" else dump(sys.argv[1]))
