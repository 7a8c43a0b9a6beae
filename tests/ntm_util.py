"""Helpers shared by tests/test_ntm_shapes_gpu.py and tests/test_ntm_values_gpu.py: the case record, the "focused" / i.i.d.
construction of parameters and inputs, the float64 / float32 oracle results of a case (computed once), the cell on the kernels the
case names, and the forward / gradient comparisons with their bounds."""
import functools

import numpy as np
import torch

from oracle import ntm_oracle as O
from oracle import ntm_oracle_torch as OT

DIN = 10
STATE_KEYS = ("M", "w", "read", "controller_state")
#: period 7 against gate blocks of `hidden` columns: a unit's four gates get different entries
DEEP_BIAS_PATTERN = np.array([0, 0, 0, 0.12, -0.12, 1, -1], np.float32)


class Case(object):
    """dims = (N, Md, R, Wh, hid, shift_range, O); fwd / bwd = the kernel the plan must report (None: refused).  xscale multiplies the
    inputs; deep_bias x DEEP_BIAS_PATTERN, repeated, is added to the LSTM biases of every layer above the first (such a layer sees the
    layer below's h, within +-1, whatever the inputs are); similarity is the content-addressing mode of the cell and of the oracles."""

    def __init__(self, name, dims, fwd, bwd, wf=0, B=2, S=6, layers=1, mode="focused", beta=30.0, gamma=1.0, scale=0.05, seed=0,
                 xscale=1.0, deep_bias=0.0, similarity="as_coded"):
        self.name, self.dims, self.fwd, self.bwd, self.wf, self.B, self.S, self.layers = name, dims, fwd, bwd, wf, B, S, layers
        self.mode, self.beta, self.gamma, self.scale, self.seed = mode, beta, gamma, scale, seed
        self.xscale, self.deep_bias, self.similarity = xscale, deep_bias, similarity

    def cfg(self):
        N, Md, R, Wh, hid, sr, O_ = self.dims
        return O.NTMConfig(DIN, O_, mem_size=N, mem_dim=Md, shift_range=sr, controller_hidden_size=hid,
                           controller_num_layers=self.layers, write_head_size=Wh, read_head_size=R, write_first=bool(self.wf),
                           similarity=self.similarity)


# ------------------------------------------------------------------------------------------------------------- inputs, oracle side
def _params(case):
    cfg, rng = case.cfg(), np.random.default_rng(1000 + case.seed)
    p = O.init_params(cfg, rng, scale=case.scale)
    for k in p:
        if k.endswith("biases"):
            p[k] = rng.uniform(-case.scale, case.scale, size=p[k].shape).astype(np.float32)
    if case.mode == "focused":
        H, Md, SS = cfg.heads, cfg.mem_dim, cfg.shift_space
        p["init_state/M"] = rng.standard_normal((cfg.mem_size, Md)).astype(np.float32)
        b = p["addressing/biases"].astype(np.float64)
        offs = np.cumsum([0] + cfg.control_sizes)
        b[offs[0]:offs[1]] += 1.5 * rng.choice([-1.0, 1.0], size=H * Md)                    # keys
        b[offs[1]:offs[2]] += case.beta                                                     # beta
        gate = rng.choice([-1.0, 1.0], size=H)
        gate[0], gate[-1] = 1.0, -1.0                                                       # both kinds of gate in every cell
        b[offs[2]:offs[3]] += 1.5 * gate
        taps = rng.integers(0, SS, size=H)
        taps[0] = 0                                                                         # head 0: an off-centre tap for certain
        for h in range(H):
            b[offs[3] + h * SS + taps[h]] += 3.0                                            # one shift tap per head
        b[offs[4]:offs[5]] += case.gamma * rng.uniform(0.5, 1.0, size=H)                    # gamma
        p["addressing/biases"] = b.astype(np.float32)
    for l in range(1, cfg.layers if case.deep_bias else 0):                                 # no draw: the other cases keep their inputs
        p["lstm/cell_%d/biases" % l] += np.resize(np.float32(case.deep_bias) * DEEP_BIAS_PATTERN, 4 * cfg.hidden)
    return cfg, p, rng


@functools.lru_cache(maxsize=None)
def _inputs(case):
    """Parameters, inputs, the perturbed initial state, the cotangents and the float64 / float32 oracle results of a case."""
    cfg, p, rng = _params(case)
    B, S = case.B, case.S
    x = (rng.standard_normal((B, S, DIN)) * case.xscale).astype(np.float32)
    st0 = O.zero_state(cfg, p, B)
    st0 = {k: (v + rng.uniform(0, 0.05, size=v.shape)).astype(np.float32) for k, v in st0.items()}
    st0["controller_state"] = rng.uniform(-0.3, 0.3, size=st0["controller_state"].shape).astype(np.float32)
    dlog = rng.standard_normal((B, S, cfg.output_dim)).astype(np.float32)
    dfin = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in st0.items()}
    # float64 numpy oracle, step by step (the records, the last step's controls and every step's gate pre-activations per layer)
    p64 = {k: v.astype(np.float64) for k, v in p.items()}
    st = {k: v.astype(np.float64) for k, v in st0.items()}
    outs, logits, states, pre, dbg = [], [], [], [], None
    for t in range(S):
        with np.errstate(over="ignore"):                     # the oracle's sigmoid is 1 / (1 + exp(-x)): exp(800) = inf, 1 / inf = 0
            o, l, st, dbg = O.ntm_step(cfg, p64, x[:, t].astype(np.float64), st)
        outs.append(o); logits.append(l); states.append(st); pre.append(dbg["gates_pre"])
    ref = {"outputs": np.stack(outs, 1), "logits": np.stack(logits, 1), "states": states, "final": st, "last": dbg,
           "gates_pre": [np.stack([s[l] for s in pre], 0) for l in range(cfg.layers)]}
    # the float32 evaluation of the torch restatement, the same quantities
    with torch.no_grad():
        p32 = {k: torch.tensor(v) for k, v in p.items()}
        s32 = {k: torch.tensor(v) for k, v in st0.items()}
        err32 = 0.0
        for t in range(S):
            l32, s32 = OT.ntm_step(cfg, p32, torch.tensor(x[:, t]), s32)
            err32 = max(err32, float(np.max(np.abs(l32.numpy() - ref["logits"][:, t]))),
                        float(np.max(np.abs(torch.softmax(l32, 1).numpy() - ref["outputs"][:, t]))),
                        *[float(np.max(np.abs(s32[k].numpy() - states[t][k]))) for k in STATE_KEYS])
    ref["err32"] = err32
    return case, cfg, p, x, st0, dlog, dfin, ref


# ------------------------------------------------------------------------------------------------------------------- kernel side
def _cell(case, cfg, p, cuda):
    from ntmtrack.ntm import NTMCell, StackedNTMCell
    N, Md, R, Wh, hid, sr, O_ = case.dims
    more = {} if case.similarity == "as_coded" else {"similarity": case.similarity}
    cell = NTMCell(O_, mem_size=N, mem_dim=Md, shift_range=sr, controller_hidden_size=hid, controller_num_layers=case.layers,
                   write_head_size=Wh, read_head_size=R, write_first=bool(case.wf), device=cuda, **more)
    assert isinstance(cell, StackedNTMCell) == (case.layers > 1)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()}, input_dim=DIN)
    plan = cell.plan(case.B)
    assert (plan["fwd_kernel"], plan["bwd_kernel"]) == (case.fwd, case.bwd), (case.name, plan)
    assert plan["forward"] and plan["bptt"] == (case.bwd is not None)
    return cell


def _dev(d, cuda):
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to(cuda) for k, v in d.items()}


def _forward(cell, x, st, cuda):
    X = cell._pad_inputs(torch.from_numpy(x).to(cuda))
    if X.shape[-1] != cell.input_ldx:                       # the deep cell pads inside run_sequence
        Xp = torch.zeros(X.shape[:2] + (cell.input_ldx,), device=cuda)
        Xp[:, :, :X.shape[-1]] = X
        X = Xp
    logits, outs, new, rec = cell.run_sequence(X, st, record=True)
    if getattr(cell, "L", 1) > 1:
        assert cell.last_form == "fused"
    return X, logits, outs, new, rec


def _grads(cell):
    sd = cell.state_dict(grad=True)
    return {k: v.numpy().astype(np.float64) for k, v in sd.items() if not k.startswith("init_state/")}


def _relerr(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def _check_forward(name, ref, logits, outs, new, rec, t0=0):
    """2e-5 absolute on everything the forward returns; rec covers steps t0 .. t0 + S' - 1 of the oracle's run."""
    S = logits.shape[1]
    worst = {}

    def cmp(what, got, want):
        worst[what] = max(worst.get(what, 0.0), float(np.max(np.abs(got.cpu().numpy() - want))))

    cmp("logits", logits, ref["logits"][:, t0:t0 + S])
    cmp("outputs", outs, ref["outputs"][:, t0:t0 + S])
    for k in STATE_KEYS:
        cmp("final " + k, new[k], ref["states"][t0 + S - 1][k])
    for t in (0, S // 2, S - 1):
        for k in ("M", "w", "read"):
            cmp("record " + k, rec[k][:, t], ref["states"][t0 + t][k])
    print("%s forward, absolute error vs float64: %s" % (name, {k: "%.1e" % v for k, v in worst.items()}))
    bad = {k: v for k, v in worst.items() if not v <= 2e-5}
    assert not bad, (name, bad)


def _oracle_grads(case, t0=None, t1=None, dfinal=None, state=None):
    """float64 and float32 autograd over steps t0 .. t1 - 1 (default: the whole sequence, the case's own cotangents)."""
    case, cfg, p, x, st0, dlog, dfin, ref = _inputs(case)
    t0, t1 = 0 if t0 is None else t0, case.S if t1 is None else t1
    state, dfinal = st0 if state is None else state, dfin if dfinal is None else dfinal
    out = []
    for dt, npdt in ((torch.float64, np.float64), (torch.float32, np.float32)):
        g, g0, _l, _f = OT.grads_with_state(cfg, p, x[:, t0:t1], {k: v.astype(npdt) for k, v in state.items()}, dlog[:, t0:t1],
                                            {k: v.astype(npdt) for k, v in dfinal.items()}, dtype=dt)
        g = {k: v.astype(np.float64) for k, v in g.items() if not k.startswith("init_state/")}
        g.update({"d " + k: v.astype(np.float64) for k, v in g0.items()})
        out.append(g)
    return out


def _check_grads(name, got, ref64, ref32):
    worst, bad, branch = {}, {}, []
    assert set(got) == set(ref64), (sorted(got), sorted(ref64))
    for k in sorted(ref64):
        err, err32 = _relerr(got[k], ref64[k]), _relerr(ref32[k], ref64[k])
        worst[k] = (err, err32)
        if not err <= max(1e-4, 3 * err32):                    # not `err > ...`: a NaN gradient must not pass
            bad[k] = (err, err32)
        elif err > 1e-4:
            branch.append(k)
    print("%s relative gradient error (HIP, float32 oracle) vs float64: %s" % (name, {k: ("%.1e" % a, "%.1e" % b_) for k, (a, b_) in worst.items()}))
    if branch:
        print("%s: within 3 x the float32 oracle's error but above 1e-4: %s" % (name, branch))
    assert not bad, (name, bad)
