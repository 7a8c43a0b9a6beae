"""The NTM sequence kernels in the value regimes training enters: SATURATED LSTM pre-activations and COLLAPSED weightings.

tests/test_ntm_shapes_gpu.py runs every kernel id on inputs whose gate pre-activations stay within a few units and ASSERTS that no
weighting collapses.  Here five kernels (the table below; the plan must report them, tests/ntm_util.py::_cell asserts it) run the
focused construction of that file in the two regimes it keeps away from.  Bounds as there: forward 2e-5 absolute against the
float64 numpy oracle, the float32 oracle within 5e-6 of float64 on every forward quantity, parameter and initial-state gradients for a
random dlogits and a random final-state cotangent by max(1e-4, 3 x the float32 oracle's own error) of the tensor's largest entry.

  saturated   the inputs x 300 (x 200 leaves the largest pre-activation at 72 .. 86); on the second layer of the deep controller,
              which sees the first layer's h whatever the inputs are, biases of +-12 and +-100 on four columns of seven.  The kernels' fast activations (NTM_FAST_MATH, csrc/ntm_common.h: tanh = 1 - 2 rcp(1 + __expf(2x)),
              sigmoid = rcp(1 + __expf(-x))) pass through the overflow of exp (x beyond +-44.4 / +-88.8).  Oracle side: of every
              layer's gate pre-activations at least a quarter have |z| > 10, some lie beyond +44.4, -44.4, +88.8 and -88.8.
  collapsed   gamma bias 8.  Sharpening divides by sum + 1e-3 (quirk Q4): a head whose powered weighting has no mass left keeps
              none, its entries reach float32 denormals and exact zeros, and ntm_pow's `x > 0 ? .. : 0`, __logf of a denormal and
              the BPTT's `wv > 0 ? dpw * gam * pw / wv : 0` / `dpw * pw * logf(wv)` take their other branch.  Oracle side, at the
              last step: some head's weighting sums to less than 0.01 and some head's to more than 0.5; in the float32 numpy oracle
              at least one entry of w is exactly 0 and at least one is a denormal (0 < w < 1.18e-38).  The peak / mass conditions
              of the focused construction are not asserted here.  The wv and w records of the last step are compared as well
              (2e-5; a flushed denormal differs by less than 1e-38): nothing there may be NaN or Inf.

test_oracle_side_conditions runs without a device; `python tests/test_ntm_values_gpu.py` prints the numbers.  Measured
(profiles/value_regimes.txt has every figure):
  saturated   share of |z| > 10: 0.57 .. 0.71 per layer; range of z -129 .. 127 over the cases, every layer beyond +-88.8; float32
              oracle error at most 3.4e-6 (tracker); its gradient error at most 5.6e-6 (d w, tracker)
  collapsed   smallest head mass 5.7e-11 .. 2.4e-7, largest 0.93 .. 0.99; exact zeros in the float32 oracle's w 11 .. 845, denormals
              23 .. 95; float32 oracle error at most 1.4e-6; its gradient error at most 2.7e-6
The kernels flush denormals: their w has no denormal left and more zeros (73 .. 964), within 1.9e-6 of the oracle's."""
import functools
import sys

import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O

from ntm_util import STATE_KEYS, Case, _cell, _check_forward, _check_grads, _dev, _forward, _grads, _inputs, _oracle_grads

TRACKER = (128, 20, 4, 1, 200, 1, 2)
HEADS15 = (64, 4, 8, 7, 64, 1, 2)
SMOOTH = "smooth_cosine"
# name, dims, the kernel the plan must report forward / in BPTT, and the focused construction's settings of the same row in
# tests/test_ntm_shapes_gpu.py
KERNELS = [
    ("tracker", TRACKER, "ws", "ws", dict(B=2, beta=40, gamma=2)),
    ("tracker_write_first", TRACKER, "fixdims-512", "generic-768", dict(wf=1, B=3, beta=30, gamma=2, seed=2)),
    ("heads15", HEADS15, "generic-1024", "generic-1024", dict(B=3, beta=20, seed=9)),
    ("deep2_tracker", TRACKER, "deep-768", "deep-768", dict(layers=2, beta=30, gamma=2, seed=30)),
    ("tracker_smooth", TRACKER, "fixdims-512", "fix", dict(B=2, beta=40, gamma=2, similarity=SMOOTH)),
]
# x 200 leaves the largest pre-activation at 72 .. 86: x 300.  The second layer of a deep controller sees h of the first, within +-1:
# scaling its weights makes the recurrence chaotic (float32 oracle 1e-5 .. 1e-3 from float64), so its biases get +-12 and +-100 on
# four columns of seven (tests/ntm_util.py).  Seeds: the row's own where it meets the conditions, else one of 100 .. 111 that does.
REGIMES = {"saturated": dict(xscale=300.0), "collapsed": dict(gamma=8)}
PER_CASE = {"deep2_tracker-saturated": dict(deep_bias=100.0), "tracker_smooth-saturated": dict(seed=2),
            "tracker_write_first-collapsed": dict(seed=105), "heads15-collapsed": dict(seed=102), "deep2_tracker-collapsed": dict(seed=108)}
CASES = [Case("%s-%s" % (name, regime), dims, fwd, bwd, **dict(dict(kw, **more), **PER_CASE.get("%s-%s" % (name, regime), {})))
         for name, dims, fwd, bwd, kw in KERNELS for regime, more in REGIMES.items()]
BY_NAME = {c.name: c for c in CASES}
FLT_MIN = float(np.finfo(np.float32).tiny)                      # 1.18e-38


@functools.lru_cache(maxsize=None)
def _final_w32(name):
    """The weightings after the last step in the float32 numpy oracle (numpy flushes no denormal)."""
    case, cfg, p, x, st0, dlog, dfin, ref = _inputs(BY_NAME[name])
    st = st0
    for t in range(case.S):
        with np.errstate(over="ignore"):
            _o, _l, st, _d = O.ntm_step(cfg, p, x[:, t], st)
    assert st["w"].dtype == np.float32
    return st["w"]


def oracle_side(name):
    """Every figure the oracle-side conditions of a case are about, as {label: value}."""
    case, cfg, p, x, st0, dlog, dfin, ref = _inputs(BY_NAME[name])
    out = {"float32 oracle error": ref["err32"]}
    for l, z in enumerate(ref["gates_pre"]):
        out.update({"layer %d share of |z| > 10" % l: float(np.mean(np.abs(z) > 10)), "layer %d z min" % l: float(z.min()),
                    "layer %d z max" % l: float(z.max())})
    mass, w32 = ref["final"]["w"].sum(axis=2), _final_w32(name)
    out.update({"smallest head mass": float(mass.min()), "largest head mass": float(mass.max()),
                "exact zeros in w (float32)": float(np.sum(w32 == 0)), "denormals in w (float32)": float(np.sum((w32 > 0) & (w32 < FLT_MIN)))})
    return out


def _check_oracle_side(name):
    v = oracle_side(name)
    print("%s oracle side: %s" % (name, {k: "%.3g" % x for k, x in v.items()}))
    assert v["float32 oracle error"] <= 5e-6, "%s: the float32 oracle is %.2e from float64" % (name, v["float32 oracle error"])
    if name.endswith("-saturated"):
        for l in range(BY_NAME[name].layers):
            assert v["layer %d share of |z| > 10" % l] >= 0.25, (name, l)
            assert v["layer %d z max" % l] > 88.8 and v["layer %d z min" % l] < -88.8, (name, l)
    else:
        assert v["smallest head mass"] < 0.01 and v["largest head mass"] > 0.5, name
        assert v["exact zeros in w (float32)"] >= 1 and v["denormals in w (float32)"] >= 1, name


@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_oracle_side_conditions(name):
    _check_oracle_side(name)


@pytest.mark.gpu
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_value_regime_matches_the_oracles(cuda, name):
    _check_oracle_side(name)
    case, cfg, p, x, st0, dlog, dfin, ref = _inputs(BY_NAME[name])
    cell = _cell(case, cfg, p, cuda)
    st = _dev(st0, cuda)
    X, logits, outs, new, rec = _forward(cell, x, st, cuda)
    torch.cuda.synchronize()
    _check_forward(name, ref, logits, outs, new, rec)
    if name.endswith("-collapsed"):
        last = {"wv": ref["last"]["w_conv"], "w": ref["last"]["w"]}
        got = {k: rec[k][:, case.S - 1].cpu().numpy() for k in last}
        assert all(np.isfinite(g).all() for g in got.values()), {k: int((~np.isfinite(g)).sum()) for k, g in got.items()}
        errs = {k: float(np.max(np.abs(got[k] - last[k]))) for k in last}
        print("%s last step's records vs float64: %s; exact zeros in the kernel's w: %d, denormals: %d"
              % (name, {k: "%.1e" % e for k, e in errs.items()}, int(np.sum(got["w"] == 0)), int(np.sum((got["w"] > 0) & (got["w"] < FLT_MIN)))))
        assert all(e <= 2e-5 for e in errs.values()), errs
    g0 = cell.backward_sequence(X, st, rec, torch.from_numpy(dlog).to(cuda), dfinal=_dev(dfin, cuda))
    torch.cuda.synchronize()
    got = _grads(cell)
    got.update({"d " + k: g0[k].cpu().numpy().astype(np.float64) for k in STATE_KEYS})
    ref64, ref32 = _oracle_grads(BY_NAME[name])
    _check_grads(name, got, ref64, ref32)


if __name__ == "__main__":
    for c in CASES:
        for label, value in oracle_side(c.name).items():
            print("%-32s %-32s %.4g" % (c.name, label, value))
    sys.exit(0)
