"""Helpers shared by the DNC shape tests: a valid non-degenerate access state, its conversion to the float64 torch oracle's and
to the HIP core's state tuples, and the conditioning of the parameters (tests/test_dnc_gpu.py builds its inputs the same way)."""
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
