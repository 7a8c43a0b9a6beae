"""GPU: the DNC sequence kernels at the edges of the shapes their launchers and planners accept, against the oracles.

One table.  A case names the boundary it sits on and, for each kernel family -- "seq" = one workgroup per sequence
(ntk_dnc_seq_fwd / _bwd), "lds" = the LDS-resident cluster form (ntk_dnc_cluster_*), "mp" = the memory-partitioned cluster form
(ntk_dnc_mp_*) -- and each direction, whether the family must take it.  For the cluster forms the table holds the cluster size the
four planners must answer at the case's batch and k_request (0: refused); test_planners_answer_as_the_table_says asserts them.  The
seq family has no planner: an accepted direction runs (the family that ran is asserted), a refused BPTT raises NtkError.
The one-workgroup BPTT takes K = reads x word + hidden <= 1024 (one thread per element of d[reads_prev ; h_prev]); the cluster
BPTT kernels stride there, so cl_w256 and cl_hid1024 have their gradients checked on a cluster form only.

Inputs as in tests/test_dnc_gpu.py (tests/dnc_util.py): init_params, biases uniform in +-0.3, interface weights x 6 forward and
x 4 in BPTT, a random non-degenerate initial state with distinct usages.

Per case and family:
  * conditioning, asserted on the oracle side before the kernel is looked at: the float32 numpy oracle and the float64 torch
    restatement agree within 1.25e-5 (a quarter of the forward bound) on the outputs, the final memory, the read and write
    weights, the link, the precedence and the usage.  A seed that fails this is changed; the bound is not;
  * forward: every quantity test_dnc_gpu.py::test_dnc_sequence_matches_oracle compares, against the float32 numpy oracle, 5e-5
    absolute;
  * records: the run is recorded with DNC.poison_records on (the record tensors start as NaN instead of whatever the caching
    allocator hands back): after the forward no element of any record is NaN;
  * BPTT where a kernel takes it: every parameter gradient against float64 autograd, relative to the tensor's largest entry at
    most max(1e-4, 3 x the float32 oracle's own error), finite first.

The oracles of a case are computed once and shared by its families."""
import ctypes
import functools

import numpy as np
import pytest
import torch

from oracle import dnc_oracle as D
from oracle import dnc_oracle_torch as DT

from dnc_util import _random_state, conditioned_params, convert_state, to_device, to_dtype

pytestmark = pytest.mark.gpu

DIN = 10
FWD_ATOL = 5e-5
COND = FWD_ATOL / 4


class Case(object):
    """dims = (N, W, R, Wn, hid, O).  seq = (forward, BPTT) accepted by ntk_dnc_seq_fwd / ntk_dnc_seq_bwd.  lds / mp = (forward, BPTT)
    cluster size ntk_dnc_cluster_plan / _bwd_plan and ntk_dnc_mp_plan / _bwd_plan must answer at batch B and k_request k; 0 = refused."""

    def __init__(self, name, dims, boundary, seq=(True, True), lds=(0, 0), mp=(0, 0), k=0, clip=20.0, S=4, B=2, seed=5):
        self.name, self.dims, self.boundary, self.seq, self.lds, self.mp, self.k = name, dims, boundary, seq, lds, mp, k
        self.clip, self.S, self.B, self.seed = clip, S, B, seed

    def cfg(self):
        N, W, R, Wn, hid, O = self.dims
        return D.DNCConfig(DIN, O, memory_size=N, word_size=W, num_reads=R, num_writes=Wn, hidden_size=hid, clip_value=self.clip)

    def families(self):
        """(family, forward k, BPTT k) of every family whose forward the table accepts; k = 1: the one-workgroup kernels, 0: refused."""
        out = [("seq", 1, 1 if self.seq[1] else 0)] if self.seq[0] else []
        return out + [(f, t[0], t[1]) for f, t in (("lds", self.lds), ("mp", self.mp)) if t[0]]


# The cluster planners take num_writes 1, memory_size a multiple of 64 up to 512 and at most 7 outputs: no row of the first block.
CASES = [
    Case("minimum", (4, 4, 1, 1, 4, 1), "every dimension at its minimum", S=6, B=3),
    # the one-workgroup BPTT sums d[reads_prev ; h_prev] with one thread per element: K = R W + hid <= 1024
    Case("rw1024", (16, 256, 4, 1, 16, 2), "R W = 1024 = one thread per read-word element; K = 1040: forward only", seq=(True, False)),
    Case("k1024", (16, 128, 4, 1, 512, 2), "K = R W + hid = 1024: the largest the one-workgroup BPTT takes"),
    Case("k1280", (16, 128, 4, 1, 768, 2), "K = 1280 with R W = 512: forward only", seq=(True, False)),
    Case("hid1024", (16, 8, 2, 1, 1024, 2), "hid = 1024 = one thread per hidden unit; K = 1040: forward only", seq=(True, False), S=3),
    Case("ip4152", (16, 256, 4, 4, 16, 2), "IP = 4152: 1038 interface column groups > 1024 threads; K = 1040: forward only",
         seq=(True, False)),
    Case("ip4124_wn5", (16, 256, 1, 5, 16, 2), "IP = 4124, five write heads: forward only", seq=(True, False)),
    Case("wn8", (40, 12, 3, 8, 24, 2), "eight write heads: forward only", seq=(True, False), S=5),
    Case("n260", (260, 8, 2, 2, 20, 3), "link column block 256 + 4, two write heads, O padded to 4"),
    Case("n340", (340, 12, 3, 1, 340, 2), "three allocation slices of 340 threads (1020 of 1024 busy), no clipping", clip=0.0),
    Case("n1024", (1024, 8, 1, 1, 16, 2), "N = 1024: one slot per thread", S=3, B=1),
    # the forward's LDS: 153120 B of 163840; the BPTT's: 237568 B
    Case("n1024_r4", (1024, 16, 4, 1, 64, 2), "N = 1024 with four read heads: the BPTT's LDS does not fit", seq=(True, False), S=3, B=1),
    Case("w132_o16", (24, 132, 2, 2, 36, 16), "W / 4 = 33 under 64-lane rows, O = 16 = one wave per output", S=5, B=3),
    Case("hid513", (16, 8, 2, 1, 513, 2), "odd hidden size: forward only (the BPTT wants a multiple of 4)", seq=(True, False), S=3),
    # cluster edges: num_writes 1, memory_size a multiple of 64; every family
    Case("cl_upk1", (64, 16, 1, 1, 4, 2), "8 link rows and one hidden unit per workgroup at k 8: four workgroups own no unit",
         lds=(8, 8), mp=(8, 8), k=8, S=6, B=3),
    Case("cl_n192", (192, 20, 3, 1, 36, 2), "memory_size 192 is no power of two: 24 rows per workgroup at k 8", lds=(8, 8), mp=(8, 8), k=8, S=5),
    # the LDS-resident BPTT keeps d(memory) in registers: word_size <= 64; K = 1056 is past the one-workgroup BPTT
    Case("cl_w256", (64, 256, 4, 1, 32, 2), "454 interface column groups and R W = 1024 against 512 threads", seq=(True, False),
         lds=(4, 0), mp=(4, 4), k=4),
    Case("cl_rw512", (64, 128, 4, 1, 32, 2), "R W = 512 = the threads of a cluster workgroup", lds=(4, 0), mp=(4, 4), k=4),
    # the memory-partitioned BPTT takes at most 128 hidden units per workgroup; K = 1028
    Case("cl_hid1024", (128, 4, 1, 1, 1024, 7), "W / 4 = 1, 512 hidden units per workgroup = its threads at k 2, O = 7", seq=(True, False),
         lds=(2, 2), mp=(2, 0), k=2, S=3),
    # 512 x 512 link: 128 KiB of rows per workgroup at k 8 beside 40 KiB of replicated memory; the LDS-resident BPTT stops at N 256
    Case("cl_n512", (512, 16, 2, 1, 40, 2), "memory_size 512: memory-partitioned form only (generic instantiation)", lds=(0, 0), mp=(4, 4),
         k=4, S=3, B=1),
]
BY_NAME = {c.name: c for c in CASES}
RUNS = [pytest.param(c.name, f, kf, kb, id="%s-%s" % (c.name, f)) for c in CASES for f, kf, kb in c.families()]


# ------------------------------------------------------------------------------------------------------------- oracle side
@functools.lru_cache(maxsize=None)
def _forward_oracle(name):
    """Inputs of the forward comparison, the float32 numpy oracle's results and the conditioning number (its largest distance from
    the float64 torch restatement over the quantities listed in the module docstring)."""
    case = BY_NAME[name]
    cfg, rng = case.cfg(), np.random.default_rng(case.seed)
    p = conditioned_params(cfg, rng, 6)
    x = rng.standard_normal((case.S, case.B, DIN)).astype(np.float32)
    st0 = _random_state(cfg, case.B, rng)
    ys, fin = D.run_model(cfg, p, x, state=st0)
    t64 = to_dtype(torch.float64)
    with torch.no_grad():
        ys64, fin64 = DT.run_model(cfg, {k: t64(v) for k, v in p.items()}, t64(x), convert_state(st0, DT, t64))
    a, a64 = fin.access_state, fin64.access_state
    cond = {nm: float(np.max(np.abs(np.asarray(u, np.float64) - v.numpy()))) for nm, u, v in (
        ("outputs", ys, ys64), ("memory", a.memory, a64.memory), ("read_weights", a.read_weights, a64.read_weights),
        ("write_weights", a.write_weights, a64.write_weights), ("link", a.linkage.link, a64.linkage.link),
        ("precedence", a.linkage.precedence_weights, a64.linkage.precedence_weights), ("usage", a.usage, a64.usage))}
    return cfg, p, x, st0, ys, fin, cond


@functools.lru_cache(maxsize=None)
def _bptt_oracle(name):
    """Inputs of the gradient comparison, float64 autograd's gradients and the float32 evaluation of the same restatement."""
    case = BY_NAME[name]
    cfg, rng = case.cfg(), np.random.default_rng(case.seed + 12)
    p = conditioned_params(cfg, rng, 4)
    x = rng.standard_normal((case.S, case.B, DIN)).astype(np.float32)
    Gy = rng.standard_normal((case.S, case.B, case.dims[5])).astype(np.float32)
    st0 = _random_state(cfg, case.B, rng)
    grads = {}
    for dtype in (torch.float64, torch.float32):
        t = to_dtype(dtype)
        pt = {k: t(v).requires_grad_(True) for k, v in p.items()}
        ys, _ = DT.run_model(cfg, pt, t(x), convert_state(st0, DT, t))
        (ys * t(Gy)).sum().backward()
        grads[dtype] = {k: v.grad.double().numpy() for k, v in pt.items()}
    return cfg, p, x, Gy, st0, grads[torch.float64], grads[torch.float32]


# ------------------------------------------------------------------------------------------------------------- device side
def _core(case, p, family, k, dev):
    from ntmtrack.dnc import DNC
    N, W, R, Wn, hid, O = case.dims
    core = DNC({"memory_size": N, "word_size": W, "num_reads": R, "num_writes": Wn}, {"hidden_size": hid}, O, case.clip, device=dev)
    core.load_state_dict({kk: torch.from_numpy(v) for kk, v in p.items()})
    core.poison_records = True
    if family == "seq":
        core.cluster_k = 0
    else:
        core.cluster_k, core.cluster_form = k, family
    return core


def _assert_family(core, family, k, bwd=False):
    """The kernel family and cluster size that RAN are the ones the table names (k = 1: the one-workgroup kernels)."""
    got_k = core.last_cluster_bwd_k if bwd else core.last_cluster_k
    got_f = core.last_cluster_bwd_form if bwd else core.last_cluster_form
    if k == 1:
        assert got_k == 1 and got_f is None, (got_k, got_f)
    else:
        assert got_k == k and got_f == family, (family, k, got_k, got_f)
        core.check_cluster()


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_planners_answer_as_the_table_says(cuda, name):
    from ntmtrack import _lib
    case, L = BY_NAME[name], _lib.lib()
    want = {"ntk_dnc_cluster_plan": case.lds[0], "ntk_dnc_cluster_bwd_plan": case.lds[1],
            "ntk_dnc_mp_plan": case.mp[0], "ntk_dnc_mp_bwd_plan": case.mp[1]}
    got = {}
    for fn in want:
        k, nbytes = ctypes.c_int(-1), ctypes.c_size_t(0)
        rc = getattr(L, fn)(case.B, *case.dims, case.k, ctypes.byref(k), ctypes.byref(nbytes))
        assert (rc == 0) == (k.value > 0) and (k.value > 0) == (nbytes.value > 0), (fn, rc, k.value, nbytes.value)
        assert rc == 0 or L.ntk_last_error(), fn
        got[fn] = k.value
    print("%s (%s): planners answer %s" % (name, case.boundary, got))
    assert got == want


@pytest.mark.parametrize("name,family,k_fwd,k_bwd", RUNS)
def test_dnc_edge_shape_forward_and_records(cuda, name, family, k_fwd, k_bwd):
    case = BY_NAME[name]
    cfg, p, x, st0, ys, fin, cond = _forward_oracle(name)
    print("%s/%s conditioning (float32 numpy oracle vs float64 torch): %s" % (name, family, {k: "%.1e" % v for k, v in cond.items()}))
    assert all(np.isfinite(v) and v <= COND for v in cond.values()), cond
    from ntmtrack import dnc as G
    core = _core(case, p, family, k_fwd, cuda)
    out, st = core.run_sequence(torch.from_numpy(x).to(cuda), convert_state(st0, G, to_device(cuda)), record=True)
    torch.cuda.synchronize()
    _assert_family(core, family, k_fwd)
    nan = {nm: int(torch.isnan(core.last_record[nm]).sum()) for nm in G.DNC.REC_NAMES}
    acc, ref = st.access_state, fin.access_state
    pairs = (("outputs", out, ys), ("memory", acc.memory, ref.memory), ("usage", acc.usage, ref.usage),
             ("write_weights", acc.write_weights, ref.write_weights), ("read_weights", acc.read_weights, ref.read_weights),
             ("link", acc.linkage.link, ref.linkage.link), ("precedence", acc.linkage.precedence_weights, ref.linkage.precedence_weights),
             ("reads", st.access_output, fin.access_output), ("h", st.controller_state.hidden, fin.controller_state.hidden),
             ("c", st.controller_state.cell, fin.controller_state.cell))
    errs = {nm: float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - want))) for nm, got, want in pairs}
    print("%s/%s forward error vs the float32 numpy oracle: %s" % (name, family, {k: "%.1e" % v for k, v in errs.items()}))
    print("%s/%s NaN elements left in the records: %s" % (name, family, {k: v for k, v in nan.items() if v} or "none"))
    bad = {nm: e for nm, e in errs.items() if not e <= FWD_ATOL}
    assert not bad, bad
    # the bias and padding columns of the three records that are left operands of the weight-gradient GEMMs: [.. ; 1 ; 0 ..]
    hid, RW = case.dims[4], case.dims[2] * case.dims[1]
    for nm, at in (("z", RW + hid), ("hc", hid), ("yin", hid + RW)):
        tail = core.last_record[nm][:, :, at:].cpu().numpy()
        assert np.all(tail[:, :, 0] == 1) and np.all(tail[:, :, 1:] == 0), (nm, tail[0, 0])
    # structural properties the reference tests assert (addressing_test.py:208-216)
    link, N = acc.linkage.link.cpu().numpy(), case.dims[0]
    assert link.min() >= -1e-6 and link.max() <= 1 + 1e-6
    assert np.abs(link[:, :, range(N), range(N)]).max() == 0
    assert not any(nan.values()), nan


@pytest.mark.parametrize("name,family,k_fwd,k_bwd", RUNS)
def test_dnc_edge_shape_bptt(cuda, name, family, k_fwd, k_bwd):
    """Where a cluster form has the forward and its planner refuses the BPTT, the one-workgroup BPTT kernel runs on the cluster
    forward's records (asserted), and its gradients are checked alike.  Where that kernel refuses the shape too, backward_sequence
    raises."""
    from ntmtrack import dnc as G
    from ntmtrack._lib import NtkError
    case = BY_NAME[name]
    if k_bwd == 0 and not case.seq[1]:
        cfg, p, x, st0 = _forward_oracle(name)[:4]
        core = _core(case, p, family, k_fwd, cuda)
        core.run_sequence(torch.from_numpy(x).to(cuda), convert_state(st0, G, to_device(cuda)), record=True)
        with pytest.raises(NtkError):
            core.backward_sequence(core.last_X, torch.ones((case.B, case.S, case.dims[5]), device=cuda))
        torch.cuda.synchronize()
        return
    cfg, p, x, Gy, st0, g64, g32 = _bptt_oracle(name)
    core = _core(case, p, family, k_fwd, cuda)
    core.run_sequence(torch.from_numpy(x).to(cuda), convert_state(st0, G, to_device(cuda)), record=True)
    _assert_family(core, family, k_fwd)
    dout = torch.from_numpy(np.ascontiguousarray(np.transpose(Gy, (1, 0, 2)))).to(cuda)      # [B,S,O]
    grads = core.backward_sequence(core.last_X, dout)
    torch.cuda.synchronize()
    _assert_family(core, family, k_bwd or 1, bwd=True)
    assert sorted(grads) == sorted(p)
    worst, bad = {}, {}
    for k in sorted(p):
        ref, got = g64[k], grads[k].cpu().numpy().astype(np.float64)
        assert got.shape == ref.shape, k
        scale = np.max(np.abs(ref)) + 1e-30
        err32 = float(np.max(np.abs(g32[k] - ref)) / scale)
        finite = bool(np.isfinite(got).all())
        err = float(np.max(np.abs(got - ref)) / scale) if finite else float("nan")
        worst[k] = (err, err32)
        if not finite or not err <= max(1e-4, 3 * err32):
            bad[k] = (err, err32)
    print("%s/%s relative gradient error (HIP, float32 oracle) vs float64: %s" % (name, family, {k: ("%.1e" % a, "%.1e" % b) for k, (a, b) in worst.items()}))
    assert not bad, bad


# ------------------------------------------------------------------------------------------- pointer checks of the cluster launchers
NTK_ERR_BAD_SHAPE, NTK_ERR_BAD_PTR = -1, -2
PTR_DIMS, PTR_B, PTR_S, PTR_K = (64, 16, 2, 1, 24, 2), 2, 3, 4
FWD_ALIGNED = ("xproj", "Wr", "Wi", "mem", "link", "rec_gates", "rec_M", "rec_L", "workspace")
BWD_ALIGNED = ("WrT", "Wi", "rec_gates", "rec_M", "rec_L", "gM", "gL", "dgates", "mem0", "link0", "workspace")


@pytest.mark.parametrize("form", ["lds", "mp"])
def test_cluster_launchers_refuse_bad_pointers_before_anything_is_enqueued(cuda, form):
    """ntk_dnc_cluster_fwd / _bwd and ntk_dnc_mp_fwd / _bwd at (64, 16, 2, 1, 24, 2), B 2, S 3, k 4, with real tensors: each required
    pointer null in turn (the workspace among them), each pointer of the 16-byte set at an address = 4 mod 16 (the workspace among
    them), 1 and 17 of the 18 forward records, and ldkT + 4 on the BPTT entries.  Every call is refused with its code and a reason
    that names the entry; afterwards the two workspaces still hold the pattern they were filled with: nothing was enqueued."""
    from ntmtrack import _lib
    from ntmtrack.dnc import DNC
    L, P = _lib.lib(), _lib.ptr
    N, W, R, Wn, hid, O = PTR_DIMS
    B, S, k = PTR_B, PTR_S, PTR_K
    core = DNC({"memory_size": N, "word_size": W, "num_reads": R, "num_writes": Wn}, {"hidden_size": hid}, O, 20.0, input_dim=DIN, device=cuda)
    z = lambda *s: torch.zeros(s, device=cuda)
    rec = core._alloc_records(B, S)
    ldkT = (core.K + 3) // 4 * 4
    sym = core.FORM_SYMBOLS[form]
    ws = {}
    for d in ("plan", "bwd_plan"):
        kk, nbytes = ctypes.c_int(0), ctypes.c_size_t(0)
        assert getattr(L, sym[d])(B, *PTR_DIMS, k, ctypes.byref(kk), ctypes.byref(nbytes)) == 0 and kk.value == k
        ws[d] = torch.full(((nbytes.value + 3) // 4,), 1.25, device=cuda)
    state = dict(mem=z(B, N, W), link=z(B, Wn, N, N), usage=z(B, N), rw=z(B, R, N), ww=z(B, Wn, N), prec=z(B, Wn, N))
    fwd = dict(xproj=z(B * S, 4 * hid), Wr=core.Wr, Wi=core.Wi, Wy=core.Wy, **state, reads=z(B, R, W), hc=z(B, 2 * hid), out=z(B, S, O))
    fwd.update({"rec_" + n: rec[n] for n in core.REC_NAMES}, workspace=ws["plan"])
    bwd = dict(WrT=z(4 * hid, ldkT), Wi=core.Wi, Wy=core.Wy, **{n + "0": t for n, t in state.items()}, hc0=z(B, 2 * hid))
    bwd.update({"rec_" + n: rec[n] for n in core.BWD_REC_NAMES}, dout=z(B, S, O), gM=z(B, N, W), gL=z(B, Wn, N, N), dgates=z(B, S, 4 * hid),
               dxi=z(B, S, core.IP), dypre=z(B, S, core.OP), gcarry=None, workspace=ws["bwd_plan"])
    assert len(fwd) == 13 + 18 + 1 and len(bwd) == 3 + 7 + 15 + 7 + 1
    off4 = lambda t: ctypes.c_void_p(t.data_ptr() + 4)
    bad = []

    def call(entry, args, want, what, ld=ldkT, **swap):
        a = {n: P(t) for n, t in args.items()}
        a.update(swap)
        v = list(a.values())
        if args is fwd:
            rc = getattr(L, entry)(B, S, *PTR_DIMS, 20.0, k, *v, _lib.stream())
        else:
            rc = getattr(L, entry)(B, S, *PTR_DIMS, 20.0, k, v[0], ld, *v[1:-1], 0, v[-1], _lib.stream())
        msg = L.ntk_last_error() or b""
        if rc != want or not msg.startswith(entry.encode()):
            bad.append("%s, %s: returned %d (expected %d), reason %r" % (entry, what, rc, want, msg))

    recs = ["rec_" + n for n in core.REC_NAMES]
    for n in fwd:
        if n not in recs:
            call(sym["fwd"], fwd, NTK_ERR_BAD_PTR, n + " null", **{n: None})
    for n in FWD_ALIGNED:
        call(sym["fwd"], fwd, NTK_ERR_BAD_PTR, n + " at 4 mod 16", **{n: off4(fwd[n])})
    call(sym["fwd"], fwd, NTK_ERR_BAD_PTR, "1 of 18 records", **{n: None for n in recs[1:]})
    call(sym["fwd"], fwd, NTK_ERR_BAD_PTR, "17 of 18 records", **{recs[-1]: None})
    for n in bwd:
        if n != "gcarry":
            call(sym["bwd"], bwd, NTK_ERR_BAD_PTR, n + " null", **{n: None})
    for n in BWD_ALIGNED:
        call(sym["bwd"], bwd, NTK_ERR_BAD_PTR, n + " at 4 mod 16", **{n: off4(bwd[n])})
    call(sym["bwd"], bwd, NTK_ERR_BAD_SHAPE, "ldkT + 4", ld=ldkT + 4)
    assert not bad, "\n  ".join(bad)
    torch.cuda.synchronize()
    for d, t in ws.items():
        assert bool((t == 1.25).all()), "%s: the %s workspace was written" % (form, d)
