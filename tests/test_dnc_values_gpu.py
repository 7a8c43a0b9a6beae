"""The DNC sequence kernels in the value regimes training enters: an ACTIVE clip on h, c and y, and SATURATED pre-activations.

tests/test_dnc_shapes_gpu.py pins the kernels at the edges of their shapes with inputs that stay inside the clip and keep the gates
off saturation.  Here the shapes are small and the values are not.  Families as there: "seq" = one workgroup per sequence, "lds" =
the LDS-resident cluster form, "mp" = the memory-partitioned cluster form; a run is (case, family, cluster size) and the family and
size that RAN are asserted.  Inputs as there (tests/dnc_util.py): conditioned_params with interface gain 6 for the forward and 4
for BPTT, _random_state, DIN 10; the forward and the BPTT comparison draw their inputs from two seeds of the case.

Active clip (clip_value 0.15): clip_cluster runs on all three families (k 2 and k 8 on the cluster forms; at k 8 a workgroup owns
three hidden units), clip_three_writes on the MW = 4 instantiation of the one-workgroup BPTT.  Each of the three clips masks the
gradient; the BPTT re-clips the recorded pre-clip cell for t > 0 and takes the initial cell as given.
Saturated (clip 20): saturated_cluster multiplies lstm/w_gates and the inputs until the fast forms of tanh, sigmoid and softplus in the
cluster kernels (1 - 2 rcp(1 + __expf(2x)), rcp(1 + __expf(-x)), max(x, 0) + __logf(1 + __expf(-|x|))) pass through the overflow of
exp and through log(1 + 0).

ORACLE SIDE, asserted before a kernel is looked at (test_oracle_side_conditions runs without a device; `python
tests/test_dnc_values_gpu.py` prints the numbers).  A seed that fails a condition is changed, the condition is not.
  * every case, both input sets: the float32 numpy oracle and the float64 torch restatement agree within 1.25e-5 (a quarter of the
    forward bound) on outputs, memory, read / write weights, link, precedence and usage;
  * active clip, both input sets: of the pre-clip h, of the pre-clip c and of the pre-clip y between 10 % and 90 % lie outside
    +-clip; no pre-clip value of either oracle is closer than 2e-4 to +-clip (4 x the forward bound: a kernel whose pre-clip values
    are within 5e-5 of the oracle's has the oracle's masks); some |c0| of the initial state exceeds the clip;
  * active clip: three mutants of the float64 oracle -- the gradient let straight through the h, the c or the y clip, forward
    unchanged (oracle.dnc_oracle_torch.run_model(straight_through=...)) -- fed to the gradient comparison in place of a kernel's
    gradients each miss the bound in force by at least 10 x on some tensor: the comparison would see a dropped mask;
  * saturated, the float64 oracle's pre-activations, both input sets: at least half of the LSTM's sigmoid / tanh arguments have
    |z| > 4, some lie beyond +44.4 and some beyond -44.4, some sigmoid arguments beyond +-88.8, some strength pre-activations
    beyond +17 and some beyond -17.

Measured on the oracle side (profiles/value_regimes.txt has every figure):
  active clip   shares outside the clip: h 0.15 .. 0.25, c 0.47 .. 0.57, y 0.39 .. 0.71; smallest margin 6.2e-4; 65 .. 76 % of |c0|
                beyond the clip; conditioning at most 2.3e-7; the float32 restatement's gradient error at most 2.7e-6; the mutants
                miss the bound by 2 465 x (h, clip_cluster) .. 54 195 x (y, clip_cluster), 22 to 24 of the 24 tensors each
  saturated     lstm/w_gates x 30, inputs x 3, interface gain 12, strength biases +-20 (x 12 / x 3 reaches +-57 only): 91 % of the
                sigmoid / tanh arguments beyond 4, range -147 .. 127 (forward inputs) and -118 .. 113 (BPTT inputs), strengths
                -32 .. 31; conditioning 3.6e-6 / 4.5e-6; the float32 restatement's gradient error 3.3e-5
Found with this file: B15 of both cluster families clipped the INITIAL cell of a launch as well (csrc/dnc_cluster_phases.h,
dncc_bwd_lstm), so with |c0| beyond the clip the forget-gate gradient of step 0 was wrong: lstm/w_gates 3.6e-2 and lstm/b_gates
1.7e-2 off float64 on lds and mp at k 2 and k 8, the one-workgroup kernel right.

KERNEL SIDE, per run:
  * forward: every quantity test_dnc_shapes_gpu.py compares, 5e-5 absolute against the float32 numpy oracle, and over all steps the
    records rec_c against the oracle's pre-clip c, rec_hc and rec_yin against its clipped h and rec_ypre against its pre-clip y;
    with DNC.poison_records on no record element is NaN afterwards;
  * BPTT: the same record comparison on the BPTT inputs (so the masks are the oracle's), then every parameter gradient against
    float64 autograd: finite, and relative to the tensor's largest entry at most max(1e-4, 3 x the float32 restatement's own error);
  * clip_cluster only: BPTT in segments of 3, 3 and 2 steps equals the unsegmented run's within 2e-5 of each tensor's largest entry
    (the bound of test_dnc_gpu.py::test_dnc_segmented_bptt_equals_whole_sequence) and meets the float64 rule; two chained
    run_sequence calls of 4 steps with the state handed over give the outputs and the final state of one call of 8 steps bit for
    bit (the segmented tests of test_dnc_gpu.py claim that of a segmented forward, which is such a chain, on every family)."""
import functools
import sys

import numpy as np
import pytest
import torch

from oracle import dnc_oracle as D

from dnc_util import (_random_state, assert_family, autograd_grads, clip_shares_and_margin, conditioned_params, convert_state,
                      gradient_errors, make_core, to_device, traced_oracles)

DIN = 10
FWD_ATOL = 5e-5
COND = FWD_ATOL / 4
MARGIN = 4 * FWD_ATOL
MUTANTS = ("h", "c", "y")
ALL_FAMILIES = (("seq", 1), ("lds", 2), ("lds", 8), ("mp", 2), ("mp", 8))


class Case(object):
    """dims = (N, W, R, Wn, hid, O); runs = (family, cluster size) pairs; seeds = (forward inputs, BPTT inputs).  gates / inputs
    multiply lstm/w_gates and x; iface = the interface gain (forward, BPTT); strength_bias goes on the write strengths and, with
    alternating sign, on the read strengths."""

    def __init__(self, name, dims, runs, clip, S, B, seeds, gates=1.0, inputs=1.0, iface=(6, 4), strength_bias=0.0):
        self.name, self.dims, self.runs, self.clip, self.S, self.B, self.seeds = name, dims, runs, clip, S, B, seeds
        self.gates, self.inputs, self.iface, self.strength_bias = gates, inputs, iface, strength_bias

    def cfg(self):
        N, W, R, Wn, hid, O = self.dims
        return D.DNCConfig(DIN, O, memory_size=N, word_size=W, num_reads=R, num_writes=Wn, hidden_size=hid, clip_value=self.clip)


CLUSTER_DIMS = (64, 16, 2, 1, 24, 2)
CASES = [
    Case("clip_cluster", CLUSTER_DIMS, ALL_FAMILIES, 0.15, 8, 3, seeds=(14, 7)),
    Case("clip_three_writes", (16, 8, 2, 3, 16, 3), (("seq", 1),), 0.15, 6, 2, seeds=(3, 0)),
    Case("saturated_cluster", CLUSTER_DIMS, (("seq", 1), ("lds", 8), ("mp", 8)), 20.0, 8, 3, seeds=(3, 1), gates=30.0, inputs=3.0,
         iface=(12, 12), strength_bias=20.0),
]
BY_NAME = {c.name: c for c in CASES}
RUNS = [pytest.param(c.name, f, k, id="%s-%s-k%d" % (c.name, f, k)) for c in CASES for f, k in c.runs]
CLIP_RUNS = [pytest.param(f, k, id="%s-k%d" % (f, k)) for f, k in ALL_FAMILIES]


# ------------------------------------------------------------------------------------------------------------- oracle side
@functools.lru_cache(maxsize=None)
def _oracle(name, which):
    """Inputs and oracle results of a case's forward ("fwd") or BPTT ("bptt") comparison.  The draws follow the shape tests': parameters,
    inputs, (output cotangent,) initial state."""
    case = BY_NAME[name]
    bptt = which == "bptt"
    cfg, rng = case.cfg(), np.random.default_rng(case.seeds[bptt])
    p = conditioned_params(cfg, rng, case.iface[bptt])
    p["lstm/w_gates"] = (p["lstm/w_gates"] * case.gates).astype(np.float32)
    if case.strength_bias:
        for nm in ("write_strengths", "read_strengths"):
            b = p["memory_access/%s/b" % nm]
            sign = 1.0 if nm == "write_strengths" else np.where(np.arange(b.size) % 2 == 0, -1.0, 1.0)
            p["memory_access/%s/b" % nm] = (b + case.strength_bias * sign).astype(np.float32)
    x = (rng.standard_normal((case.S, case.B, DIN)) * case.inputs).astype(np.float32)
    Gy = rng.standard_normal((case.S, case.B, case.dims[5])).astype(np.float32) if bptt else None
    st0 = _random_state(cfg, case.B, rng)
    ys, fin, tr32, tr64, cond = traced_oracles(cfg, p, x, st0)
    o = dict(case=case, cfg=cfg, p=p, x=x, Gy=Gy, st0=st0, ys=ys, fin=fin, tr32=tr32, tr64=tr64, cond=cond)
    if bptt:
        o["g64"] = autograd_grads(cfg, p, x, Gy, st0, torch.float64)
        o["g32"] = autograd_grads(cfg, p, x, Gy, st0, torch.float32)
    return o


@functools.lru_cache(maxsize=None)
def _mutant_factors(name):
    """Per straight-through mutant of the float64 oracle: the largest ratio, over the tensors, of its error in the gradient comparison to
    the bound in force there, and that tensor."""
    o = _oracle(name, "bptt")
    out = {}
    for m in MUTANTS:
        worst, bad = gradient_errors(autograd_grads(o["cfg"], o["p"], o["x"], o["Gy"], o["st0"], torch.float64, straight_through=(m,)),
                                     o["g64"], o["g32"])
        k = max(worst, key=lambda kk: worst[kk][0] / worst[kk][2])
        out[m] = (worst[k][0] / worst[k][2], k, len(bad))
    return out


def oracle_side(name):
    """Every figure the oracle-side conditions of a case are about, as {label: value}."""
    case, out = BY_NAME[name], {}
    hid = case.dims[4]
    for which in ("fwd", "bptt"):
        o = _oracle(name, which)
        out[which + " conditioning"] = max(o["cond"].values())
        if case.clip < 20:
            shares, margin = clip_shares_and_margin(case.clip, (o["tr32"], o["tr64"]))
            out.update({"%s share of pre-clip %s outside the clip" % (which, nm): v for nm, v in shares.items()})
            out[which + " margin"] = margin
            out[which + " share of |c0| beyond the clip"] = float(np.mean(np.abs(o["st0"].controller_state.cell) > case.clip))
        else:
            z, s = o["tr64"]["gates"], o["tr64"]["strengths"]
            sig = np.concatenate([z[..., :hid], z[..., 2 * hid:]], -1)
            out.update({which + " share of gate pre-activations beyond 4": float(np.mean(np.abs(z) > 4)),
                        which + " gate pre-activation min": float(z.min()), which + " gate pre-activation max": float(z.max()),
                        which + " sigmoid argument min": float(sig.min()), which + " sigmoid argument max": float(sig.max()),
                        which + " strength pre-activation min": float(s.min()), which + " strength pre-activation max": float(s.max())})
    o = _oracle(name, "bptt")
    out["float32 restatement's largest gradient error"] = max(v[1] for v in gradient_errors(o["g64"], o["g64"], o["g32"])[0].values())
    if case.clip < 20:
        for m, (factor, k, nbad) in _mutant_factors(name).items():
            out["mutant %s: x the bound (%s; %d tensors miss)" % (m, k, nbad)] = factor
    return out


@functools.lru_cache(maxsize=None)                                     # asserted (and printed) once per case and session
def _check_oracle_side(name):
    case, v = BY_NAME[name], oracle_side(name)
    print("%s oracle side: %s" % (name, {k: "%.3g" % x for k, x in v.items()}))
    for which in ("fwd", "bptt"):
        assert v[which + " conditioning"] <= COND, (name, which, _oracle(name, which)["cond"])
        if case.clip < 20:
            for nm in ("h", "c", "y"):
                share = v["%s share of pre-clip %s outside the clip" % (which, nm)]
                assert 0.10 <= share <= 0.90, (name, which, nm, share)
            assert v[which + " margin"] >= MARGIN, (name, which, v[which + " margin"])
            assert v[which + " share of |c0| beyond the clip"] > 0, (name, which)
        else:
            assert v[which + " share of gate pre-activations beyond 4"] >= 0.5, (name, which)
            assert v[which + " gate pre-activation max"] > 44.4 and v[which + " gate pre-activation min"] < -44.4, (name, which)
            assert v[which + " sigmoid argument max"] > 88.8 and v[which + " sigmoid argument min"] < -88.8, (name, which)
            assert v[which + " strength pre-activation max"] > 17 and v[which + " strength pre-activation min"] < -17, (name, which)
    if case.clip < 20:
        for m, (factor, k, nbad) in _mutant_factors(name).items():
            print("%s: the gradient let straight through the %s clip misses the bound by %.0f x (%s)" % (name, m, factor, k))
            assert factor >= 10 and nbad >= 1, (name, m, factor)


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_oracle_side_conditions(name):
    _check_oracle_side(name)


# ------------------------------------------------------------------------------------------------------------- device side
def _run_recorded(o, family, k, dev, segment=None):
    from ntmtrack import dnc as G
    case = o["case"]
    core = make_core(case.dims, case.clip, o["p"], family, k, dev)
    core.bptt_segment = segment
    out, st = core.run_sequence(torch.from_numpy(o["x"]).to(dev), convert_state(o["st0"], G, to_device(dev)), record=True)
    torch.cuda.synchronize()
    assert_family(core, family, k)
    return core, out, st


def _record_errors(o, core, out):
    """Outputs and the four records the clips sit on, over all steps, against the float32 numpy oracle; NaN elements per record."""
    from ntmtrack import dnc as G
    case, tr = o["case"], o["tr32"]
    hid = case.dims[4]
    sb = lambda v: np.transpose(v, (1, 0, 2))                                                # the records are [B, S, .]
    rec = {nm: core.last_record[nm].cpu().numpy() for nm in ("c", "hc", "yin", "ypre")}
    h_clipped = D.clip(case.cfg(), tr["h"])
    pairs = (("outputs", out.cpu().numpy(), o["ys"]), ("rec_c", rec["c"], sb(tr["c"])), ("rec_hc", rec["hc"][:, :, :hid], sb(h_clipped)),
             ("rec_yin", rec["yin"][:, :, :hid], sb(h_clipped)), ("rec_ypre", rec["ypre"], sb(tr["y"])))
    errs = {nm: float(np.max(np.abs(got.astype(np.float64) - want))) for nm, got, want in pairs}
    nan = {nm: int(torch.isnan(core.last_record[nm]).sum()) for nm in G.DNC.REC_NAMES}
    return errs, nan


@pytest.mark.gpu
@pytest.mark.parametrize("name,family,k", RUNS)
def test_value_regime_forward_and_records(cuda, name, family, k):
    _check_oracle_side(name)
    o = _oracle(name, "fwd")
    core, out, st = _run_recorded(o, family, k, cuda)
    errs, nan = _record_errors(o, core, out)
    acc, fin = st.access_state, o["fin"]
    ref = fin.access_state
    pairs = (("memory", acc.memory, ref.memory), ("usage", acc.usage, ref.usage), ("write_weights", acc.write_weights, ref.write_weights),
             ("read_weights", acc.read_weights, ref.read_weights), ("link", acc.linkage.link, ref.linkage.link),
             ("precedence", acc.linkage.precedence_weights, ref.linkage.precedence_weights), ("reads", st.access_output, fin.access_output),
             ("h", st.controller_state.hidden, fin.controller_state.hidden), ("c", st.controller_state.cell, fin.controller_state.cell))
    errs.update({nm: float(np.max(np.abs(got.cpu().numpy().astype(np.float64) - want))) for nm, got, want in pairs})
    print("%s/%s/k%d forward error vs the float32 numpy oracle (largest %.1e, bound %.0e): %s"
          % (name, family, k, max(errs.values()), FWD_ATOL, {kk: "%.1e" % v for kk, v in errs.items()}))
    print("%s/%s/k%d NaN elements left in the records: %s" % (name, family, k, {kk: v for kk, v in nan.items() if v} or "none"))
    bad = {nm: e for nm, e in errs.items() if not e <= FWD_ATOL}
    assert not bad, bad
    assert not any(nan.values()), nan


def _check_bptt(o, core, out, family, k, dev, what):
    errs, nan = _record_errors(o, core, out) if core.last_record else ({}, {})
    bad = {nm: e for nm, e in errs.items() if not e <= FWD_ATOL}
    assert not bad and not any(nan.values()), (bad, nan)
    dout = torch.from_numpy(np.ascontiguousarray(np.transpose(o["Gy"], (1, 0, 2)))).to(dev)      # [B,S,O]
    grads = core.backward_sequence(core.last_X, dout)
    torch.cuda.synchronize()
    assert_family(core, family, k, bwd=True)
    grads = {kk: v.cpu().numpy().astype(np.float64) for kk, v in grads.items()}
    worst, bad = gradient_errors(grads, o["g64"], o["g32"])
    assert not [n for n, v in worst.items() if v[0] != v[0]], "not finite: %s" % [n for n, v in worst.items() if v[0] != v[0]]
    kk = max(worst, key=lambda n: worst[n][0] / worst[n][2])
    print("%s relative gradient error vs float64: largest %.1e; closest to its bound %s: %.1e (float32 oracle %.1e, bound %.1e)"
          % (what, max(v[0] for v in worst.values()), kk, worst[kk][0], worst[kk][1], worst[kk][2]))
    assert not bad, bad
    return grads


@pytest.mark.gpu
@pytest.mark.parametrize("name,family,k", RUNS)
def test_value_regime_bptt(cuda, name, family, k):
    _check_oracle_side(name)
    o = _oracle(name, "bptt")
    core, out, _st = _run_recorded(o, family, k, cuda)
    _check_bptt(o, core, out, family, k, cuda, "%s/%s/k%d" % (name, family, k))


@pytest.mark.gpu
@pytest.mark.parametrize("family,k", CLIP_RUNS)
def test_segmented_bptt_under_an_active_clip(cuda, family, k):
    """clip_cluster in BPTT segments of 3, 3 and 2 steps: the cell that crosses a seam is the clipped one of the checkpoint (the hc0
    of the segment's launch), inside a segment the recorded pre-clip one."""
    _check_oracle_side("clip_cluster")
    o = _oracle("clip_cluster", "bptt")
    what = "clip_cluster/%s/k%d" % (family, k)
    core, out, _st = _run_recorded(o, family, k, cuda)
    whole = _check_bptt(o, core, out, family, k, cuda, what + " whole")
    core, out_s, _st = _run_recorded(o, family, k, cuda, segment=3)
    assert core.last_segments is not None and [b - a for a, b in core.last_segments[2]] == [3, 3, 2]
    assert torch.equal(out_s, out)
    seg = _check_bptt(o, core, out_s, family, k, cuda, what + " segments of 3")
    diff = {kk: float(np.max(np.abs(seg[kk] - g)) / (np.max(np.abs(g)) + 1e-30)) for kk, g in whole.items()}
    print("%s segmented vs whole, relative to each tensor's largest entry: largest %.1e (bound 2e-5)" % (what, max(diff.values())))
    bad = {kk: v for kk, v in diff.items() if not v <= 2e-5}
    assert not bad, bad


@pytest.mark.gpu
@pytest.mark.parametrize("family,k", CLIP_RUNS)
def test_chained_sequences_under_an_active_clip(cuda, family, k):
    """Two run_sequence calls of 4 steps, the state handed over (a clipped cell; 65 % of the initial one lies beyond the clip), against one of 8."""
    from ntmtrack import dnc as G
    _check_oracle_side("clip_cluster")
    o = _oracle("clip_cluster", "fwd")
    case = o["case"]
    core = make_core(case.dims, case.clip, o["p"], family, k, cuda)
    x, st0 = torch.from_numpy(o["x"]).to(cuda), convert_state(o["st0"], G, to_device(cuda))
    whole, fin = core.run_sequence(x, st0)
    first, mid = core.run_sequence(x[:4].contiguous(), st0)
    second, end = core.run_sequence(x[4:].contiguous(), mid)
    torch.cuda.synchronize()
    assert_family(core, family, k)
    assert float(mid.controller_state.cell.abs().max()) == float(np.float32(case.clip))           # handed over clipped, and the clip bit
    flat = lambda s: (("reads", s.access_output), ("h", s.controller_state.hidden), ("c", s.controller_state.cell)) + tuple(
        zip(("memory", "read_weights", "write_weights"), s.access_state[:3])) + (
        ("link", s.access_state.linkage.link), ("precedence", s.access_state.linkage.precedence_weights), ("usage", s.access_state.usage))
    differ = [nm for (nm, a), (_n, b) in zip(flat(end), flat(fin)) if not torch.equal(a, b)]
    if not torch.equal(torch.cat([first, second], 0), whole):
        differ.append("outputs")
    assert not differ, differ


if __name__ == "__main__":
    for c in CASES:
        for label, value in oracle_side(c.name).items():
            print("%-20s %-70s %.4g" % (c.name, label, value))
    sys.exit(0)
