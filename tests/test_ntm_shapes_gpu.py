"""GPU: the NTM sequence kernels, single-layer and deep, at shapes of every kernel id their plan reports
(ntk_ntm_seq_plan / ntk_ntm_seq_deep_plan; tests/test_ntm_shapes_cabi.py sweeps the plan itself), against the float64 oracles.

Per shape: the forward from a NON-TRIVIAL initial state (the oracle's zero state plus a perturbation, different per sequence) against
the float64 numpy oracle -- logits, softmax outputs, the final M / w / read / controller state and the M / w / read records at the
first, a middle and the last step, 2e-5 absolute (the bound of test_ntm_gpu.py::test_sequence_matches_oracle); where the plan has
the BPTT, every parameter gradient (TF naming) and the gradient of every initial-state tensor for a random dlogits AND a random
final-state cotangent against float64 autograd (oracle.ntm_oracle_torch.grads_with_state), by the rule of
test_ntm_train_gpu.py::test_bptt_gradients_match_autograd_oracle: relative to the tensor's largest entry, at most
max(1e-4, 3 x the float32 oracle's own error); where the plan has the forward only, backward_sequence raises and leaves the gradient
buffer as it was.

Inputs.  Parameters drawn i.i.d. at a small scale leave every weighting within a few percent of 1/N (the slot-axis normalisation of
quirk Q1 keeps the similarities small), and a circular shift of a flat vector is the same flat vector: a kernel that shifted the
wrong way would hardly show.  So most shapes use a "focused" construction -- init_state/M ~ N(0, 1), everything else at scale 0.05,
then structured addressing biases: keys +-1.5 per element, gates +-1.5 per head, +3 on one shift tap per head, a gamma bias and a
large beta bias chosen per shape -- and the test ASSERTS on the oracle's side, before it looks at the kernel, that at the last step
every head's weighting has an entry of at least 4/N and a sum of at least 0.5 (no collapse through the 1e-3 of quirk Q4), some
head's largest entry is below 0.9, the gates are not all near 0.5 and some head shifts mostly off-centre; and for EVERY shape that
the float32 evaluation of the torch oracle is within 5e-6 of float64 on every forward quantity (a quarter of the bound: the
inputs are not ill-conditioned; beta amplifies the rounding of the similarities, so seeds and beta biases are chosen per shape).
Five shapes keep the i.i.d. construction, the regime the reference starts training in."""
import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O

import ntm_util
from ntm_util import STATE_KEYS, Case, _cell, _check_forward, _check_grads, _dev, _forward, _grads

pytestmark = pytest.mark.gpu

TRACKER = (128, 20, 4, 1, 200, 1, 2)
# name, (N, Md, R, Wh, hid, shift_range, O), the kernel the plan must report forward / in BPTT (None: refused; the test asserts it)
SINGLE = [
    Case("tracker", TRACKER, "ws", "ws", B=2, beta=40, gamma=2),
    Case("tracker_flat", TRACKER, "ws", "ws", B=3, S=8, mode="iid", seed=1),
    Case("tracker_write_first", TRACKER, "fixdims-512", "generic-768", wf=1, B=3, beta=30, gamma=2, seed=2),
    Case("tracker_write_first_flat", TRACKER, "fixdims-512", "generic-768", wf=1, B=1, S=5, mode="iid", seed=3),
    Case("tracker_O3", (128, 20, 4, 1, 200, 1, 3), "generic-768", "generic-768", beta=30, gamma=2, seed=4),
    Case("tracker_shift2", (128, 20, 4, 1, 200, 2, 2), "generic-768", "generic-768", B=3, beta=30, gamma=2, seed=5),
    Case("tracker_2write", (128, 20, 4, 2, 200, 1, 2), "generic-768", "generic-768", wf=1, beta=30, gamma=2, seed=56),
    Case("odd_dims_hid77", (192, 13, 2, 1, 77, 1, 2), "generic-768", None, B=1, S=5, beta=40, seed=7),
    Case("hid320", (128, 20, 4, 1, 320, 1, 2), "generic-1024", "generic-1024", beta=40, gamma=2, seed=8),
    Case("heads15", (64, 4, 8, 7, 64, 1, 2), "generic-1024", "generic-1024", B=3, beta=20, seed=9),
    Case("heads15_flat", (64, 4, 8, 7, 64, 1, 2), "generic-1024", "generic-1024", wf=1, mode="iid", seed=10),
    Case("pp828", (64, 100, 2, 2, 100, 1, 2), "generic-1024", "generic-1024", beta=20, seed=44),
    Case("pp828_write_first", (64, 100, 2, 2, 100, 1, 2), "generic-1024", None, wf=1, B=3, S=5, beta=30, seed=12),
    Case("shift4_n256", (256, 15, 2, 1, 320, 4, 2), "generic-1024", "generic-1024", wf=1, B=3, S=5, beta=80, seed=13),
    Case("mem_dim_1", (128, 1, 2, 1, 300, 1, 2), "generic-1024", "generic-1024", S=5, mode="iid", seed=14),
    Case("n512", (512, 16, 1, 1, 256, 1, 4), "generic-1024", None, S=5, beta=200, gamma=0, seed=54),
    Case("n1024", (1024, 8, 1, 1, 64, 1, 2), "generic-1024", None, S=5, beta=300, gamma=0, seed=46),
    Case("n256_md40", (256, 40, 3, 1, 200, 1, 2), "generic-1024", None, B=3, S=5, beta=80, seed=53),
    Case("hid960", (128, 20, 4, 1, 960, 1, 2), "generic-1024", None, S=5, beta=30, gamma=2, seed=18),
    Case("mem_dim_201", (64, 201, 1, 1, 64, 1, 2), "generic-1024", None, S=5, beta=20, seed=19),
]
DEEP = [
    Case("deep2_tracker", TRACKER, "deep-768", "deep-768", layers=2, beta=30, gamma=2, seed=30),
    Case("deep3_odd_write_first", (64, 12, 2, 2, 24, 1, 3), "deep-768", "deep-768", wf=1, layers=3, B=3, beta=20, seed=59),
    Case("deep2_heads15", (64, 4, 8, 7, 64, 1, 2), "deep-1024", "deep-1024", layers=2, beta=20, seed=32),        # Tf 1024, Tb 960
    Case("deep3_heads15", (64, 4, 8, 7, 64, 1, 2), "deep-1024", "deep-1024", layers=3, B=3, S=5, mode="iid", seed=33),
    Case("deep2_hid280", (64, 12, 2, 2, 280, 1, 2), "deep-1024", "deep-1024", layers=2, wf=1, beta=20, seed=34),  # Tf = Tb = 896
    Case("deep3_hid280", (64, 12, 2, 2, 280, 1, 2), "deep-1024", "deep-1024", layers=3, B=1, S=5, beta=20, seed=35),
    # the smooth-cosine instantiations above 768 threads, which tests/test_ntm_similarity_gpu.py (deep-768 only) does not launch:
    # 3 hid = 960 threads in both directions at the smallest memory
    Case("deep2_hid320_smooth", (64, 8, 1, 1, 320, 1, 2), "deep-1024", "deep-1024", layers=2, S=3, beta=10, gamma=2, seed=62,
         similarity="smooth_cosine"),
]
CASES = SINGLE + DEEP
CHAINED = [c for c in CASES if c.name in ("tracker", "hid320", "deep2_tracker")]
BY_NAME = {c.name: c for c in CASES}


def _inputs(name):
    """The construction and the oracle results of a case (tests/ntm_util.py), computed once."""
    return ntm_util._inputs(BY_NAME[name])


def _oracle_grads(name):
    return ntm_util._oracle_grads(BY_NAME[name])


def test_the_largest_mem_dim_in_the_list_is_the_largest_the_forward_takes():
    """mem 64 x 201 with one read and one write head: PP + Md = 820 + 201 <= 1024; at 202, P = 4 Md + 12 = 820, PP = 824 and
    PP + Md = 1026."""
    from ntmtrack import _lib
    plan = lambda Md: _lib.lib().ntk_ntm_seq_plan(2, 64, Md, 1, 1, 64, 1, 2, 0, 0, 0, None, None, None, None)
    assert plan(201) == 1 and all(plan(Md) == 0 for Md in range(202, 258))


# ------------------------------------------------------------------------------------------------------------- inputs, oracle side
def _check_inputs(name):
    """The conditions on the inputs, on the oracle's side (module docstring)."""
    case, cfg, p, x, st0, dlog, dfin, ref = _inputs(name)
    assert ref["err32"] <= 5e-6, "%s: the float32 oracle is %.2e from float64 (inputs too ill-conditioned for a 2e-5 bound)" % (name, ref["err32"])
    w, g, sw, N = ref["final"]["w"], ref["last"]["g"][..., 0], ref["last"]["sw"], cfg.mem_size
    peak, mass = w.max(axis=2), w.sum(axis=2)                                                # [B, H]
    centre = [j for j, s in enumerate(O.shift_offsets(cfg.shift_space)) if s == 0][0]
    off_centre = np.delete(sw, centre, axis=2).max(axis=2)                                   # [B, H]
    print("%s inputs: float32 oracle error %.1e; per-head peak x N %.1f .. %.1f, mass %.2f .. %.2f, gates %.2f .. %.2f, largest "
          "off-centre tap %.2f" % (name, ref["err32"], peak.min() * N, peak.max() * N, mass.min(), mass.max(), g.min(), g.max(), off_centre.max()))
    if case.mode != "focused":
        return
    assert (peak >= 4.0 / N).all(), "%s: a head's weighting is nearly flat (largest entry %.2f / N)" % (name, peak.min() * N)
    assert (mass >= 0.5).all(), "%s: a head's weighting collapsed (sum %.3f)" % (name, mass.min())
    assert (peak.min(axis=1) < 0.9).all(), "%s: every head is one-hot" % name
    assert not ((g > 0.45) & (g < 0.55)).all(), "%s: every interpolation gate is near 0.5" % name
    assert (off_centre.max(axis=1) > 0.5).all(), "%s: no head shifts mostly off-centre" % name


# ------------------------------------------------------------------------------------------------------------------- kernel side
@pytest.mark.parametrize("name", [c.name for c in CASES])
def test_shape_matches_the_oracles(cuda, name):
    from ntmtrack._lib import NtkError
    case, cfg, p, x, st0, dlog, dfin, ref = _inputs(name)
    _check_inputs(name)
    cell = _cell(case, cfg, p, cuda)
    st = _dev(st0, cuda)
    X, logits, outs, new, rec = _forward(cell, x, st, cuda)
    torch.cuda.synchronize()
    _check_forward(name, ref, logits, outs, new, rec)
    dl, df = torch.from_numpy(dlog).to(cuda), _dev(dfin, cuda)
    if case.bwd is None:
        # forward only: the BPTT is refused before anything is launched, the gradient buffer stays as it was bit for bit
        cell.params.grad.copy_(torch.arange(cell.params.grad.numel(), device=cuda, dtype=torch.float32) * 0.5 - 3.0)
        before = cell.params.grad.clone()
        with pytest.raises(NtkError):
            cell.backward_sequence(X, st, rec, dl, dfinal=df)
        torch.cuda.synchronize()
        assert torch.equal(cell.params.grad, before)
        assert not cell.plan(case.B)["bptt"] and cell.plan(case.B)["reason"]
        return
    g0 = cell.backward_sequence(X, st, rec, dl, dfinal=df)
    torch.cuda.synchronize()
    got = _grads(cell)
    got.update({"d " + k: g0[k].cpu().numpy().astype(np.float64) for k in STATE_KEYS})
    ref64, ref32 = _oracle_grads(name)
    _check_grads(name, got, ref64, ref32)


@pytest.mark.parametrize("name", [c.name for c in CHAINED])
def test_two_halves_equal_the_whole_sequence(cuda, name):
    """Segmented BPTT: S = 2k steps run as two halves -- the state carried forward, the second half's initial-state gradient handed
    to the first half as its final-state gradient, the parameter gradients of the halves added -- against the whole-sequence run.
    Both runs meet the oracle bounds, and agree with each other within 2e-6 x scale + 1e-7 (the bound of
    test_wave_specialised_kernels_equal_the_resident_form_on_short_sequences; scale = the tensor's largest entry).
    Observed on an MI355X, at all three shapes: logits, outputs, the final state and the four initial-state gradients come out
    equal bit for bit (the state and its gradient cross the seam as the fp32 values the kernels hold anyway); the parameter
    gradients do not (two weight-gradient GEMMs added against one: up to 6.6e-7 at a scale of 4.6).  The test prints which is
    which and asserts the bound only."""
    case, cfg, p, x, st0, dlog, dfin, ref = _inputs(name)
    _check_inputs(name)
    cell = _cell(case, cfg, p, cuda)
    S, k = case.S, case.S // 2
    assert S == 2 * k
    st, dl, df = _dev(st0, cuda), torch.from_numpy(dlog).to(cuda), _dev(dfin, cuda)
    # the whole sequence
    X, logits, outs, new, rec = _forward(cell, x, st, cuda)
    g0 = cell.backward_sequence(X, st, rec, dl, dfinal=df)
    torch.cuda.synchronize()
    whole = _grads(cell)
    whole.update({"d " + key: g0[key].cpu().numpy().astype(np.float64) for key in STATE_KEYS})
    whole_f = {"logits": logits.cpu().numpy(), "outputs": outs.cpu().numpy()}
    whole_f.update({"final " + key: new[key].cpu().numpy() for key in STATE_KEYS})
    # two halves
    Xa, la, oa, mid, rec_a = _forward(cell, x[:, :k], st, cuda)
    Xb, lb, ob, fin, rec_b = _forward(cell, x[:, k:], mid, cuda)
    torch.cuda.synchronize()
    _check_forward(name + " first half", ref, la, oa, mid, rec_a)
    _check_forward(name + " second half", ref, lb, ob, fin, rec_b, t0=k)
    g_mid = cell.backward_sequence(Xb, mid, rec_b, dl[:, k:].contiguous(), dfinal=df)
    torch.cuda.synchronize()
    grads_b = _grads(cell)
    g_first = cell.backward_sequence(Xa, st, rec_a, dl[:, :k].contiguous(), dfinal=g_mid)
    torch.cuda.synchronize()
    halves = {key: v + grads_b[key] for key, v in _grads(cell).items()}
    halves.update({"d " + key: g_first[key].cpu().numpy().astype(np.float64) for key in STATE_KEYS})
    halves_f = {"logits": torch.cat([la, lb], 1).cpu().numpy(), "outputs": torch.cat([oa, ob], 1).cpu().numpy()}
    halves_f.update({"final " + key: fin[key].cpu().numpy() for key in STATE_KEYS})
    ref64, ref32 = _oracle_grads(name)
    _check_grads(name + " whole", whole, ref64, ref32)
    _check_grads(name + " halves", halves, ref64, ref32)
    bad = {}
    for a, b_ in ((whole_f, halves_f), (whole, halves)):
        for key in sorted(a):
            diff, scale = float(np.max(np.abs(a[key] - b_[key]))), float(np.max(np.abs(a[key])))
            print("%s halves vs whole, %s: %s" % (name, key, "bitwise" if np.array_equal(a[key], b_[key]) else "%.1e (scale %.1e)" % (diff, scale)))
            if not diff <= 2e-6 * scale + 1e-7:
                bad[key] = (diff, scale)
    assert not bad, bad
