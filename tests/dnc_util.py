"""Helpers shared by the DNC shape and value-regime tests: a valid non-degenerate access state, its conversion to the float64 torch
oracle's and to the HIP core's state tuples, and the conditioning of the parameters (tests/test_dnc_gpu.py builds its inputs the
same way); for the value-regime tests the two oracles with their traces, the clipped shares, the gradient rule and the core on a
named kernel family."""
import numpy as np
import torch

from oracle import dnc_oracle as D


def _random_state(cfg, B, rng):
    """A valid, NON-DEGENERATE access state: distinct usages (no near-ties for the allocation sort: with several write heads and
    exactly tied usages the winner of the sort hinges on the last fp32 bit in any implementation -- the reference's own tests
    plant distinct usages for the same reason, addressing_test.py:328-333), sub-stochastic weights and link."""
    a = cfg.access
    N, W, R, Wn = a.N, a.W, a.R, a.Wn
    f = lambda *s: rng.random(s).astype(np.float32)
    usage = np.stack([rng.permutation(N) for _ in range(B)]).astype(np.float32) / N * 0.8 + 0.1
    rw = f(B, R, N); rw /= rw.sum(2, keepdims=True) + 1
    ww = f(B, Wn, N); ww /= ww.sum(2, keepdims=True) + 1
    prec = f(B, Wn, N); prec /= prec.sum(2, keepdims=True) + 1
    link = f(B, Wn, N, N)
    link /= np.maximum(link.sum(2, keepdims=True), 1)
    link /= np.maximum(link.sum(3, keepdims=True), 1)
    link[:, :, np.arange(N), np.arange(N)] = 0
    mem = (f(B, N, W) - 0.5).astype(np.float32)
    acc = D.AccessState(mem, rw, ww, D.TemporalLinkageState(link.astype(np.float32), prec), usage)
    reads = (rw @ mem).astype(np.float32)
    h, c = (f(B, cfg.hid) - 0.5), (f(B, cfg.hid) - 0.5)
    return D.DNCState(reads, acc, D.LSTMState(h, c))


def conditioned_params(cfg, rng, interface_gain):
    """init_params with non-zero biases (uniform in +-0.3) and a stronger interface (x interface_gain: 6 in the forward tests, 4 in
    the BPTT tests), so that gates and keys are not all ~0.5."""
    p = D.init_params(cfg, rng)
    for k in p:
        if k.endswith("/b") or k.endswith("b_gates"):
            p[k] = rng.uniform(-0.3, 0.3, size=p[k].shape).astype(np.float32)
        if k.startswith("memory_access/") and k.endswith("/w"):
            p[k] = (p[k] * interface_gain).astype(np.float32)
    return p


def convert_state(st, mod, t):
    """The numpy oracle's DNCState as the state tuples of `mod` (oracle.dnc_oracle_torch or ntmtrack.dnc), every array through t."""
    a = st.access_state
    return mod.DNCState(t(st.access_output),
                        mod.AccessState(t(a.memory), t(a.read_weights), t(a.write_weights),
                                        mod.TemporalLinkageState(t(a.linkage.link), t(a.linkage.precedence_weights)), t(a.usage)),
                        mod.LSTMState(t(st.controller_state.hidden), t(st.controller_state.cell)))


def to_device(dev):
    return lambda v: torch.from_numpy(np.ascontiguousarray(v)).to(dev)


def to_dtype(dtype):
    return lambda v: torch.tensor(np.asarray(v), dtype=dtype)


# ------------------------------------------------------------------------------- the value-regime tests (tests/test_dnc_values_gpu.py)
def traced_oracles(cfg, p, x, st0):
    """Both oracles over one sequence with their traces: (ys, final state, trace) of the float32 numpy oracle -- the trace holds h, c
    and y before clipping, [S, B, .] -- the float64 torch restatement's trace as float64 numpy arrays (the same three, the LSTM's
    sigmoid / tanh arguments "gates" [S, B, 4 hid] as i, j, f + 1, o and the "strengths" pre-activations [S, B, Wn + R]), and the
    conditioning: the largest distance between the two over the quantities the shape tests list."""
    from oracle import dnc_oracle_torch as DT
    tr32, tr64 = {}, {}
    with np.errstate(over="ignore"):                            # the oracle's sigmoid is 1 / (1 + exp(-x)): exp(89) = inf, 1 / inf = 0
        ys, fin = D.run_model(cfg, p, x, state=st0, trace=tr32)
    t64 = to_dtype(torch.float64)
    with torch.no_grad():
        ys64, fin64 = DT.run_model(cfg, {k: t64(v) for k, v in p.items()}, t64(x), convert_state(st0, DT, t64), trace=tr64)
    tr32 = {k: np.stack(v, 0) for k, v in tr32.items()}
    tr64 = {k: torch.stack(v, 0).numpy() for k, v in tr64.items()}
    a, a64 = fin.access_state, fin64.access_state
    cond = {nm: float(np.max(np.abs(np.asarray(u, np.float64) - v.numpy()))) for nm, u, v in (
        ("outputs", ys, ys64), ("memory", a.memory, a64.memory), ("read_weights", a.read_weights, a64.read_weights),
        ("write_weights", a.write_weights, a64.write_weights), ("link", a.linkage.link, a64.linkage.link),
        ("precedence", a.linkage.precedence_weights, a64.linkage.precedence_weights), ("usage", a.usage, a64.usage))}
    return ys, fin, tr32, tr64, cond


def clip_shares_and_margin(clipv, traces):
    """({h, c, y: share of the pre-clip values outside +-clipv}, the smallest distance of any pre-clip value from +-clipv) over every
    trace given (the float32 and the float64 oracle's): all steps, sequences and elements."""
    shares = {nm: float(np.mean(np.abs(traces[0][nm]) > clipv)) for nm in ("h", "c", "y")}
    margin = min(float(np.min(np.abs(np.abs(np.asarray(tr[nm], np.float64)) - clipv))) for tr in traces for nm in ("h", "c", "y"))
    return shares, margin


def autograd_grads(cfg, p, x, Gy, st0, dtype, straight_through=()):
    """d(sum(ys * Gy)) / d(every parameter) by torch autograd over the restatement evaluated in `dtype`, as float64 numpy arrays."""
    from oracle import dnc_oracle_torch as DT
    t = to_dtype(dtype)
    pt = {k: t(v).requires_grad_(True) for k, v in p.items()}
    ys, _ = DT.run_model(cfg, pt, t(x), convert_state(st0, DT, t), straight_through=straight_through)
    (ys * t(Gy)).sum().backward()
    return {k: v.grad.double().numpy() for k, v in pt.items()}


def gradient_errors(got, g64, g32):
    """The project's gradient rule.  Per tensor (error of `got`, error of the float32 oracle `g32`, bound in force), all relative to the
    largest entry of the float64 gradient `g64`; bound = max(1e-4, 3 x the float32 oracle's error).  A tensor of `got` that is not
    finite has error NaN.  Second result: the tensors that miss their bound."""
    assert sorted(got) == sorted(g64), (sorted(got), sorted(g64))
    worst, bad = {}, {}
    for k in sorted(g64):
        ref, g = g64[k], np.asarray(got[k], np.float64)
        assert g.shape == ref.shape, k
        scale = np.max(np.abs(ref)) + 1e-30
        err32 = float(np.max(np.abs(g32[k] - ref)) / scale)
        err = float(np.max(np.abs(g - ref)) / scale) if np.isfinite(g).all() else float("nan")
        worst[k] = (err, err32, max(1e-4, 3 * err32))
        if not err <= worst[k][2]:                               # not `err > ...`: a NaN gradient must not pass
            bad[k] = worst[k]
    return worst, bad


def make_core(dims, clipv, p, family, k, dev):
    """The HIP core with the oracle's parameters, poisoned records, on the kernel family asked for ("seq": the one-workgroup kernels;
    "lds" / "mp": that cluster form at cluster size k)."""
    from ntmtrack.dnc import DNC
    N, W, R, Wn, hid, O = dims
    core = DNC({"memory_size": N, "word_size": W, "num_reads": R, "num_writes": Wn}, {"hidden_size": hid}, O, clipv, device=dev)
    core.load_state_dict({kk: torch.from_numpy(v) for kk, v in p.items()})
    core.poison_records = True
    if family == "seq":
        core.cluster_k = 0
    else:
        core.cluster_k, core.cluster_form = k, family
    return core


def assert_family(core, family, k, bwd=False):
    """The kernel family and cluster size that RAN are the ones asked for (k = 1: the one-workgroup kernels); no hand-off timed out."""
    got_k = core.last_cluster_bwd_k if bwd else core.last_cluster_k
    got_f = core.last_cluster_bwd_form if bwd else core.last_cluster_form
    if family == "seq":
        assert got_k == 1 and got_f is None, (got_k, got_f)
    else:
        assert got_k == k and got_f == family, (family, k, got_k, got_f)
        core.check_cluster()
