"""Dev: dump what the six DNC sequence kernels compute, for comparing two builds of the library byte for byte.
    dev_dnc_cluster_dump.py OUT.npz           every CLUSTER_CASES row of tests/test_dnc_gpu.py through the one-workgroup kernels (seq/k0)
                                              and at every listed k in both cluster forms (lds, mp), c5_shape_short in the mp form,
                                              and one row with two write heads through the one-workgroup kernels (the BPTT's second
                                              instantiation): outputs, final state, the 18 records, every BPTT gradient tensor where
                                              a BPTT kernel takes the shape, and the gradients with the sequence cut into two segments
    dev_dnc_cluster_dump.py --compare A B     compare two dumps: bitwise, and max|a - b| against 2e-6 max|a| + 1e-7 where they differ
NTK_LIB_PATH selects the library (one process per library)."""
import os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np


def compare(pa, pb):
    A, B = np.load(pa), np.load(pb)
    assert sorted(A.files) == sorted(B.files), "the dumps hold different tensors"
    bad = differ = 0
    for k in sorted(A.files):
        a, b = A[k], B[k]
        if a.shape == b.shape and a.tobytes() == b.tobytes():
            continue
        differ += 1
        err, bound = float(np.max(np.abs(a - b))), 2e-6 * float(np.max(np.abs(a))) + 1e-7
        print("DIFFERS %-60s max|a-b| %.3e  bound %.3e  %s" % (k, err, bound, "ok" if err <= bound else "OVER"))
        bad += err > bound
    print("%d tensors, %d differ, %d over the bound" % (len(A.files), differ, bad))
    return 1 if bad else 0


def dump(path):
    import torch
    import test_dnc_gpu as T
    from oracle import dnc_oracle as D
    from ntmtrack import dnc as G
    dev = torch.device("cuda:0")
    out = {}
    cases = [c + (("lds", "mp"), 1) for c in T.CLUSTER_CASES] + [("c5_shape_short", 512, 128, 4, 200, 3, 1, (4,), ("mp",), 1),
                                                                  ("two_write_heads", 64, 16, 2, 24, 5, 2, (), (), 2)]
    for name, N, W, R, hid, S, B, ks, forms, Wn in cases:
        Din, O = 12, 2
        cfg = D.DNCConfig(Din, O, memory_size=N, word_size=W, num_reads=R, num_writes=Wn, hidden_size=hid, clip_value=20.0)
        rng = np.random.default_rng(41)
        p = D.init_params(cfg, rng)
        for kk in p:
            if kk.endswith("/b") or kk.endswith("b_gates"):
                p[kk] = rng.uniform(-0.3, 0.3, size=p[kk].shape).astype(np.float32)
            if kk.startswith("memory_access/") and kk.endswith("/w"):
                p[kk] = (p[kk] * 4).astype(np.float32)
        x = torch.from_numpy(rng.standard_normal((S, B, Din)).astype(np.float32)).to(dev)
        dout = torch.from_numpy(rng.standard_normal((B, S, O)).astype(np.float32)).to(dev)
        st0 = T._random_state(cfg, B, rng)
        t = lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)
        a0 = st0.access_state
        gst = G.DNCState(t(st0.access_output), G.AccessState(t(a0.memory), t(a0.read_weights), t(a0.write_weights),
                         G.TemporalLinkageState(t(a0.linkage.link), t(a0.linkage.precedence_weights)), t(a0.usage)),
                         G.LSTMState(t(st0.controller_state.hidden), t(st0.controller_state.cell)))
        for form, k in [(None, 0)] + [(f, k) for f in forms for k in ks]:
            for seg in (None, max(2, S // 2)):
                core = G.DNC({"memory_size": N, "word_size": W, "num_reads": R, "num_writes": Wn}, {"hidden_size": hid}, O, 20.0, device=dev)
                core.load_state_dict({kk: torch.from_numpy(v) for kk, v in p.items()})
                core.cluster_k, core.cluster_form, core.bptt_segment = k, form, seg
                y, st = core.run_sequence(x, gst, record=True)
                rec = {nm: core.last_record[nm].clone() for nm in G.DNC.REC_NAMES} if seg is None else {}
                bptt = core._cluster_bwd_plan(B) is not None if k else R * W + hid <= 1024      # else: no BPTT kernel takes the shape
                grads = core.backward_sequence(core.last_X, dout) if bptt else {}
                core.check_cluster()
                torch.cuda.synchronize()
                if core.last_cluster_k != max(k, 1) or (bptt and core.last_cluster_bwd_k != max(k, 1)):
                    print("%s %s k=%d: not usable (forward k %d)" % (name, form, k, core.last_cluster_k))
                    break
                assert core.last_cluster_form == form and (not bptt or core.last_cluster_bwd_form == form)
                tag = "%s/%s/k%d/" % (name, form or "seq", k)
                if seg is None:
                    a = st.access_state
                    fin = {"out": y, "memory": a.memory, "link": a.linkage.link, "usage": a.usage, "rw": a.read_weights, "ww": a.write_weights,
                           "prec": a.linkage.precedence_weights, "reads": st.access_output, "h": st.controller_state.hidden,
                           "c": st.controller_state.cell}
                    out.update({tag + nm: v.cpu().numpy() for nm, v in fin.items()})
                    out.update({tag + "rec_" + nm: v.cpu().numpy() for nm, v in rec.items()})
                out.update({tag + ("grad_" if seg is None else "seggrad_") + nm: v.cpu().numpy() for nm, v in grads.items()})
                print("%s %s k=%d segment=%s: done%s" % (name, form, k, seg, "" if bptt else " (forward only)"), flush=True)
    np.savez(path, **out)
    print("%d tensors -> %s" % (len(out), path))
    return 0


if __name__ == "__main__":
    sys.exit(compare(sys.argv[2], sys.argv[3]) if sys.argv[1] == "--compare" else dump(sys.argv[1]))
