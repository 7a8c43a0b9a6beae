"""GPU: the fused NTM kernels in smooth-cosine mode (NTMCell(similarity="smooth_cosine")) against the oracles in the same mode.

Content addressing is row-wise k.M[n] / (|k||M[n]| + 1e-3) instead of the reference's as-coded similarity (quirk Q1).  The two
are different models: every parity case first shows, on the float64 oracle alone, that at its inputs the modes differ by far more
than the tolerance, so a kernel that ignored the mode could not pass.

Inputs as tests/test_ntm_train_gpu.py::test_bptt_gradients_match_autograd_oracle builds them (rng 21, init_params(scale=0.2),
random biases, serialised ReLU-like features, D = 514, T = 2 frames = 130 steps), with addressing/weights and init_state/M
multiplied by 5 so that addressing matters.  Tolerances are the project's: logits atol 2e-5, loss rtol 1e-4, every gradient
tensor within max(1e-4, 3 x the float32 oracle's own error) of float64, relative to the tensor's largest entry."""
import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O
from oracle import ntm_oracle_torch as OT

pytestmark = pytest.mark.gpu

D, T = 514, 2
SMOOTH = "smooth_cosine"

#       name  cell kwargs                                                                                 B  forward kernel   BPTT kernel
CASES = {
    "a": (dict(mem_size=128, mem_dim=20, read_head_size=4, write_head_size=1, controller_hidden_size=200), 2, "fixdims-512", "fix"),
    "b": (dict(mem_size=64, mem_dim=8, read_head_size=2, write_head_size=2, controller_hidden_size=64, write_first=True), 3,
          "generic-768", "generic-768"),
    "c": (dict(mem_size=128, mem_dim=8, read_head_size=1, write_head_size=2, controller_hidden_size=48, shift_range=4,
               write_first=True), 2, "generic-768", "generic-768"),
    "d": (dict(mem_size=256, mem_dim=4, read_head_size=3, write_head_size=1, controller_hidden_size=32), 2, "generic-1024", "generic-1024"),
    "e": (dict(mem_size=64, mem_dim=72, read_head_size=1, write_head_size=1, controller_hidden_size=32), 1, "generic-768", "generic-768"),
    "f": (dict(mem_size=64, mem_dim=5, read_head_size=1, write_head_size=1, controller_hidden_size=32), 2, "generic-768", "generic-768"),
    "g2": (dict(mem_size=64, mem_dim=8, read_head_size=2, write_head_size=1, controller_hidden_size=48, controller_num_layers=2), 2,
           "deep-768", "deep-768"),
    "g3": (dict(mem_size=64, mem_dim=8, read_head_size=2, write_head_size=1, controller_hidden_size=48, controller_num_layers=3), 2,
           "deep-768", "deep-768"),
}


def _relerr(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def _config(kw, similarity):
    full = dict(shift_range=1, controller_num_layers=1)
    full.update(kw)
    return O.NTMConfig(D, 2, similarity=similarity, **full)


# The batch of cases a and b is given; for the others it is 2 wherever the float32 oracle's own logits error at that sample is under a
# tenth of the 2e-5 bound, so that the bound measures the kernel and not the conditioning of the sample.  Case e's sample at B = 2 is
# not such a one: the float32 numpy oracle is 4.8e-6 from float64 there (1.4e-7 at B = 1, 1.9e-7 .. 3.8e-7 for d and f), and the
# kernels' hardware exp / log / pow (NTM_FAST_MATH, ~1-2 ulp each) reach 4.1e-5 in smooth mode and 2.2e-5 as coded at that sample
# -- 5.3e-6 and 1.8e-6 with -DNTM_FAST_MATH=0, i.e. the oracle's own error -- against 4.7e-7 and 1.9e-6 at B = 1.  Case e runs B = 1.
#
# three LSTM layers damp what the addressing does to the logits: at init scale 0.2 the two modes' float64 logits are 9.3e-4 apart,
# under the 1e-3 this file asks of every case, so that case draws its parameters at 0.3 (the bound stays)
INIT_SCALE = {"g3": 0.3}


def _inputs(kw, B, scale=0.2):
    """(params, x [B,130,514], offsets) of a case: the same for both modes (the mode is no parameter)."""
    cfg = _config(kw, SMOOTH)
    rng = np.random.default_rng(21)
    params = O.init_params(cfg, rng, scale=scale)
    for k in params:
        if k.endswith("biases"):
            params[k] = rng.uniform(-scale, scale, size=params[k].shape).astype(np.float32)
    for k in ("addressing/weights", "init_state/M"):
        params[k] = (params[k] * 5).astype(np.float32)
    feats = np.maximum(rng.standard_normal((B, T, 64, 512)), 0).astype(np.float32)
    gts = rng.uniform(0, 1, size=(B, T, 64)).astype(np.float32)
    x = O.serialize_inputs(feats, gts)
    offs = rng.uniform(-0.5, 0.5, size=(B, T, 2)).astype(np.float32)
    return params, x, offs


_REF = {}


def _reference(name):
    """Float64 oracle of a case in smooth-cosine mode, its float32 evaluation, and the float64 oracle as coded; computed once
    per case and shared (never modified)."""
    if name not in _REF:
        kw, B = CASES[name][:2]
        params, x, offs = _inputs(kw, B, INIT_SCALE.get(name, 0.2))
        loss, grads, logits, _ = OT.loss_and_grads(_config(kw, SMOOTH), params, x, offs)
        _l32, grads32, _lg32, _p32 = OT.loss_and_grads(_config(kw, SMOOTH), params, x, offs, dtype=torch.float32)
        _la, grads_a, logits_a, _pa = OT.loss_and_grads(_config(kw, "as_coded"), params, x, offs)
        _REF[name] = dict(params=params, x=x, offs=offs, loss=loss, grads=grads, logits=logits, grads32=grads32,
                          grads_as_coded=grads_a, logits_as_coded=logits_a)
    return _REF[name]


def _assert_the_modes_differ(name, ref):
    """On the float64 oracle alone: logits >= 1e-3 apart, the addressing/weights and init_state/M gradients >= 1e-2 (relative to
    the tensor's largest entry) -- 50x and 100x the tolerances below."""
    dl = float(np.max(np.abs(ref["logits"] - ref["logits_as_coded"])))
    da = _relerr(ref["grads_as_coded"]["addressing/weights"], ref["grads"]["addressing/weights"])
    dm = _relerr(ref["grads_as_coded"]["init_state/M"], ref["grads"]["init_state/M"])
    print("case %s, smooth cosine against as coded (float64 oracle): logits %.2e, d addressing/weights %.2e, d init_state/M %.2e" % (name, dl, da, dm))
    assert dl >= 1e-3 and da >= 1e-2 and dm >= 1e-2, (name, dl, da, dm)


def _cell(kw, cuda, similarity=SMOOTH, params=None, keyword=True):
    from ntmtrack.ntm import NTMCell
    full = dict(shift_range=1, controller_num_layers=1)
    full.update(kw)
    more = dict(similarity=similarity) if keyword else {}
    cell = NTMCell(2, device=cuda, **full, **more)
    if params is not None:
        cell.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, input_dim=D)
    return cell


def _forward_backward(cell, x, offs, cuda):
    """forward + BPTT + init_state_backward through the tracking loss; (logits, loss, final state, gradients in the TF layout)."""
    from ntmtrack import tracker
    B = x.shape[0]
    X = cell._pad_inputs(torch.from_numpy(x).to(cuda))
    st0 = cell.zero_state(B)
    logits, _o, new, rec = cell.run_sequence(X, st0, record=True)
    loss, _pred, dlogits = tracker.offset_loss(logits, torch.from_numpy(offs).to(cuda), T)
    g0 = cell.backward_sequence(X, st0, rec, dlogits)
    cell.init_state_backward(g0, B)
    torch.cuda.synchronize()
    return logits, loss, new, cell.state_dict(grad=True)


def _assert_parity(name, ref, logits, loss, got):
    np.testing.assert_allclose(logits.cpu().numpy(), ref["logits"], atol=2e-5, rtol=0)
    np.testing.assert_allclose(float(loss.cpu()), ref["loss"], rtol=1e-4)
    assert sorted(got) == sorted(ref["grads"])
    worst, bad = {}, {}
    for k in sorted(ref["grads"]):
        err, err32 = _relerr(got[k].numpy(), ref["grads"][k]), _relerr(ref["grads32"][k].astype(np.float64), ref["grads"][k])
        worst[k] = (err, err32)
        if not err <= max(1e-4, 3 * err32):                    # not `err > ...`: a NaN gradient must not pass
            bad[k] = (err, err32)
    print("case %s relative gradient error (HIP, float32 oracle) vs float64: %s" % (name, {k: ("%.1e" % a, "%.1e" % b_) for k, (a, b_) in worst.items()}))
    assert not bad, bad


@pytest.mark.parametrize("name", ["a", "b", "c", "d", "e", "f"])
def test_single_layer_kernels_match_the_smooth_cosine_oracle(cuda, name):
    kw, B, fwd_kernel, bwd_kernel = CASES[name]
    ref = _reference(name)
    _assert_the_modes_differ(name, ref)
    cell = _cell(kw, cuda, params=ref["params"])
    plan = cell.plan(B)
    assert (plan["forward"], plan["bptt"], plan["fwd_kernel"], plan["bwd_kernel"]) == (True, True, fwd_kernel, bwd_kernel), plan
    logits, loss, _new, got = _forward_backward(cell, ref["x"], ref["offs"], cuda)
    _assert_parity(name, ref, logits, loss, got)


def test_wide_memory_under_two_heads_trains_as_coded_too(cuda):
    """Case e's shape (mem 64 x 72, two heads) was refused by the BPTT in either mode: 4608 memory elements over the 384 threads its
    heads and controls ask for are more than the 8 a thread prefetches.  The plan now takes the 576 threads that needs, whatever the
    mode; the as-coded kernel at that shape against the as-coded oracle."""
    kw, B, fwd_kernel, bwd_kernel = CASES["e"]
    ref = _reference("e")
    cell = _cell(kw, cuda, similarity="as_coded", params=ref["params"])
    plan = cell.plan(B)
    assert (plan["fwd_kernel"], plan["bwd_kernel"], plan["bwd_threads"]) == (fwd_kernel, bwd_kernel, 576), plan
    logits, loss, _new, got = _forward_backward(cell, ref["x"], ref["offs"], cuda)
    _l32, grads32, _lg32, _p32 = OT.loss_and_grads(_config(kw, "as_coded"), ref["params"], ref["x"], ref["offs"], dtype=torch.float32)
    as_coded = dict(ref, logits=ref["logits_as_coded"], grads=ref["grads_as_coded"], grads32=grads32,
                    loss=float(OT.offset_loss(torch.from_numpy(ref["logits_as_coded"]), torch.from_numpy(ref["offs"]).double())[0]))
    _assert_parity("e as coded", as_coded, logits, loss, got)


@pytest.mark.parametrize("name,fused", [("g2", True), ("g3", True), ("g2", False)], ids=["2-layers", "3-layers", "2-layers-stepwise"])
def test_deep_controller_matches_the_smooth_cosine_oracle(cuda, name, fused):
    """The deep persistent kernels, and once the step-wise form (layers from Python, addressing in the single-layer step kernels
    through the *_step_*_sim entries): the mode reaches both."""
    from ntmtrack.ntm import StackedNTMCell
    kw, B, fwd_kernel, bwd_kernel = CASES[name]
    ref = _reference(name)
    _assert_the_modes_differ(name, ref)
    cell = _cell(kw, cuda, params=ref["params"])
    assert isinstance(cell, StackedNTMCell) and cell.top.similarity == SMOOTH
    plan = cell.plan(B)
    assert (plan["forward"], plan["bptt"], plan["fwd_kernel"], plan["bwd_kernel"]) == (True, True, fwd_kernel, bwd_kernel), plan
    if not fused:
        cell.fused = False
    logits, loss, _new, got = _forward_backward(cell, ref["x"], ref["offs"], cuda)
    assert cell.last_form == ("fused" if fused else "stepwise")
    _assert_parity(name + ("" if fused else " step-wise"), ref, logits, loss, got)


def _random_state(cfg, params, B, rng):
    st = O.zero_state(cfg, params, B)
    return {k: (v + rng.uniform(-0.3, 0.3, size=v.shape)).astype(np.float32) for k, v in st.items()}


def test_step_api_in_smooth_cosine_mode(cuda):
    """One cell(inputs, state) step from a random state: debug["similarity"] is the stand-alone ops kernel in smooth mode on
    (M_prev, k) and the numpy oracle's; then ntk_ntm_step_bwd_sim on that step's records against autograd from the same state."""
    import ctypes
    from ntmtrack import _lib, ops
    from ntmtrack.ntm import _P
    kw, B = CASES["b"][0], 3
    cfg = _config(kw, SMOOTH)
    params = _reference("b")["params"]
    rng = np.random.default_rng(5)
    st = _random_state(cfg, params, B, rng)
    x = rng.standard_normal((B, D)).astype(np.float32)
    _out, logit_ref, new_ref, dbg = O.ntm_step(cfg, params, x, st)
    dbg_a = O.ntm_step(_config(kw, "as_coded"), params, x, st)[3]
    assert np.max(np.abs(dbg["similarity"] - dbg_a["similarity"])) > 1e-2           # the two modes are apart at this state

    cell = _cell(kw, cuda, params=params)
    tst = {k: torch.from_numpy(v).to(cuda) for k, v in st.items()}
    _o, logit, _state, debug, M, w, read, cs = cell(torch.from_numpy(x).to(cuda), tst)
    torch.cuda.synchronize()
    sim_ops = ops.batched_smooth_cosine_similarity(tst["M"], debug["k"].contiguous(), similarity=SMOOTH, device=cuda)
    assert torch.equal(debug["similarity"], sim_ops)
    np.testing.assert_allclose(debug["similarity"].cpu().numpy(), dbg["similarity"], atol=1e-6, rtol=0)
    np.testing.assert_allclose(debug["w_content_focused"].cpu().numpy(), dbg["w_content_focused"], atol=1e-5, rtol=0)
    np.testing.assert_allclose(logit.cpu().numpy(), logit_ref, atol=1e-5, rtol=0)
    for got, key in ((M, "M"), (w, "w"), (read, "read"), (cs, "controller_state")):
        np.testing.assert_allclose(got.cpu().numpy(), new_ref[key], atol=1e-5, rtol=0, err_msg=key)

    # the step's BPTT through the C ABI's step entry, with cotangents on the logits and on the whole new state
    d, L, stream = cell.dims, _lib.lib(), _lib.stream()
    X = cell._pad_inputs(torch.from_numpy(x).to(cuda).unsqueeze(1))
    _lg, _out2, _new, rec = cell.run_sequence(X, tst, record=True)
    dlogits = rng.standard_normal((B, 1, 2)).astype(np.float32)
    dfin = {k: rng.standard_normal(v.shape).astype(np.float32) for k, v in st.items()}
    grads_ref, g0_ref, _l, _f = OT.grads_with_state(cfg, params, x[:, None], st, dlogits, dfin)
    grads32, g032, _l, _f = OT.grads_with_state(cfg, params, x[:, None], st, dlogits, dfin, dtype=torch.float32)
    ldkT, ldhT = (d.K + 3) // 4 * 4, (d.hid + 3) // 4 * 4
    WrT, WaT = torch.empty((4 * d.hid, ldkT), device=cuda), torch.empty((d.PP, ldhT), device=cuda)
    _lib.check(L.ntk_transpose_pad(_P(cell.params.view("Wr")), 4 * d.hid, _P(WrT), ldkT, d.K, 4 * d.hid, stream), "ntk_transpose_pad")
    _lib.check(L.ntk_transpose_pad(_P(cell.params.view("Wa")), d.PP, _P(WaT), ldhT, d.hid, d.PP, stream), "ntk_transpose_pad")
    dgates, du = torch.empty((B, 4 * d.hid), device=cuda), torch.empty((B, d.PP), device=cuda)
    g0 = cell.state_placeholder(B)
    dl = torch.from_numpy(dlogits).to(cuda)
    df = {k: torch.from_numpy(v).to(cuda) for k, v in dfin.items()}
    _lib.check(L.ntk_ntm_step_bwd_sim(
        B, d.N, d.Md, d.R, d.Wh, d.hid, d.shift_range, d.O, 1 if cell.write_first else 0, 1,
        _P(WrT), ldkT, _P(WaT), ldhT, _P(tst["M"]), _P(tst["w"]), _P(tst["controller_state"]),
        _P(rec["gates"]), _P(rec["c"]), _P(rec["u"]), _P(rec["wc"]), _P(rec["wv"]), _P(rec["w"]), _P(rec["M"]), _P(dl),
        _P(df["M"]), _P(df["w"]), _P(df["read"]), _P(df["controller_state"]),
        _P(dgates), _P(du), _P(g0["M"]), _P(g0["w"]), _P(g0["read"]), _P(g0["controller_state"]), stream), "ntk_ntm_step_bwd_sim")
    torch.cuda.synchronize()
    got = {"state " + k: g0[k].cpu().numpy() for k in g0}
    want = {"state " + k: g0_ref[k] for k in g0_ref}
    want32 = {"state " + k: g032[k] for k in g032}
    # the controls' weight gradient is h^T du (one row of records): addressing and output weights and biases
    h1 = rec["h"][:, 0].cpu().numpy().astype(np.float64)            # [B, ldh] = [h | 1 | 0..]
    dWa = h1.T @ du.cpu().numpy().astype(np.float64)
    got.update({"addressing/weights": dWa[:d.hid, :d.P], "addressing/biases": dWa[d.hid, :d.P],
                "output/weights": dWa[:d.hid, d.P:d.P + d.O], "output/biases": dWa[d.hid, d.P:d.P + d.O]})
    for k in ("addressing/weights", "addressing/biases", "output/weights", "output/biases"):
        want[k], want32[k] = grads_ref[k], grads32[k]
    bad = {}
    for k in sorted(want):
        err, err32 = _relerr(got[k], want[k]), _relerr(want32[k].astype(np.float64), want[k])
        if not err <= max(1e-4, 3 * err32):                    # not `err > ...`: a NaN gradient must not pass
            bad[k] = (err, err32)
    assert not bad, bad


@pytest.mark.parametrize("name", ["a", "b"])
def test_a_zero_memory_row_is_similarity_zero_and_has_finite_gradients(cuda, name):
    """|M[n]| = 0: sim[.][n] = 0 / (0 + 1e-3) = 0 in the forward (equal to the oracle, no NaN); in the BPTT the gradient through
    that norm is defined as 0 where autograd yields NaN, so only finiteness is asserted there."""
    from ntmtrack import tracker
    kw, B = CASES[name][:2]
    cfg = _config(kw, SMOOTH)
    params = _reference(name)["params"]
    rng = np.random.default_rng(9)
    st = _random_state(cfg, params, B, rng)
    st["M"][:, 7, :] = 0.0
    st["M"][0, 0, :] = 0.0
    S = 3
    x = rng.standard_normal((B, S, D)).astype(np.float32)
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    _outs, logits_ref, fin, states = O.loop_ntm_tracker(cfg, p64, x.astype(np.float64), state={k: v.astype(np.float64) for k, v in st.items()},
                                                        return_states=True)
    assert np.isfinite(logits_ref).all()
    cell = _cell(kw, cuda, params=params)
    tst = {k: torch.from_numpy(v).to(cuda) for k, v in st.items()}
    X = cell._pad_inputs(torch.from_numpy(x).to(cuda))
    logits, _o, new, rec = cell.run_sequence(X, tst, record=True)
    torch.cuda.synchronize()
    np.testing.assert_allclose(logits.cpu().numpy(), logits_ref, atol=2e-5, rtol=0)
    np.testing.assert_allclose(rec["wc"][:, 0].cpu().numpy(), _wc_of_first_step(cfg, p64, x, st), atol=1e-5, rtol=0)
    for key in ("M", "w", "read", "controller_state"):
        np.testing.assert_allclose(new[key].cpu().numpy(), fin[key], atol=2e-5, rtol=0, err_msg=key)
    dlogits = torch.from_numpy(rng.standard_normal((B, S, 2)).astype(np.float32)).to(cuda)
    g0 = cell.backward_sequence(X, tst, rec, dlogits)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(cell.params.grad).all())
    for key in g0:
        assert bool(torch.isfinite(g0[key]).all()), key
    assert float(g0["M"].abs().max()) > 0 and float(cell.params.grad.abs().max()) > 0


def _wc_of_first_step(cfg, p64, x, st):
    dbg = O.ntm_step(cfg, p64, x[:, 0].astype(np.float64), {k: v.astype(np.float64) for k, v in st.items()})[3]
    return dbg["w_content_focused"]


@pytest.mark.parametrize("name", ["a", "b"])
def test_defaults_are_as_coded_and_smooth_cosine_is_reproducible(cuda, name):
    """similarity="as_coded" is the cell without the keyword, bit for bit (logits, final state, gradients); two runs of a smooth
    cell are bitwise equal (fixed summation orders)."""
    kw, B = CASES[name][:2]
    ref = _reference(name)
    runs = []
    for similarity, keyword in (("as_coded", False), ("as_coded", True), (SMOOTH, True), (SMOOTH, True)):
        cell = _cell(kw, cuda, similarity=similarity, params=ref["params"], keyword=keyword)
        assert cell.similarity == similarity
        logits, loss, new, _g = _forward_backward(cell, ref["x"], ref["offs"], cuda)
        runs.append((logits, loss, new, cell.params.grad.clone()))
    for (la, lossa, na, ga), (lb, lossb, nb, gb) in ((runs[0], runs[1]), (runs[2], runs[3])):
        assert torch.equal(la, lb) and torch.equal(lossa, lossb) and torch.equal(ga, gb)
        for key in na:
            assert torch.equal(na[key], nb[key]), key
    assert not torch.equal(runs[0][0], runs[2][0])
    np.testing.assert_allclose(runs[0][0].cpu().numpy(), ref["logits_as_coded"], atol=2e-5, rtol=0)


def test_full_length_sequence_in_smooth_cosine_mode(cuda):
    """S = 1300 strictly sequential steps at the benchmark shape, forward only, B = 1, init_scale 0.05: tanh(logit), the quantity
    the tracker consumes, stays within the north-star tolerance 1e-4 of the float64 numpy oracle (the inputs and the bound of
    tests/test_ntm_gpu.py::test_full_length_sequence_drift)."""
    from ntmtrack.ntm import LoopNTMTracker
    kw = CASES["a"][0]
    cfg = _config(kw, SMOOTH)
    rng = np.random.default_rng(123)
    params = O.init_params(cfg, rng, scale=0.05)
    for k in params:
        if k.endswith("biases"):
            params[k] = rng.uniform(-0.05, 0.05, size=params[k].shape).astype(np.float32)
    B, frames = 1, 20
    feats = np.maximum(rng.standard_normal((B, frames, 64, 512)), 0).astype(np.float32)
    x = O.serialize_inputs(feats, rng.uniform(0, 1, size=(B, frames, 64)).astype(np.float32))
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    _, logits, fin = O.loop_ntm_tracker(cfg, p64, x.astype(np.float64))
    cell = _cell(kw, cuda, params=params)
    assert cell.plan(B)["fwd_kernel"] == "fixdims-512"
    trk = LoopNTMTracker.__new__(LoopNTMTracker)
    trk.cell, trk.initializer, trk.sequence_length = cell, None, frames * 65
    _o, l_gpu = trk(torch.from_numpy(x).to(cuda))
    torch.cuda.synchronize()
    assert l_gpu.shape == (B, 1300, 2)
    err = np.max(np.abs(np.tanh(l_gpu.cpu().numpy()) - np.tanh(logits)))
    assert err < 1e-4, err
    assert np.max(np.abs(trk.last_state["M"].cpu().numpy() - fin["M"])) < 1e-4


def test_offset_tracker_train_step_matches_the_oracle_update(cuda):
    """NTMOffsetTracker(similarity="smooth_cosine") without VGG: one loss_and_grads + clipped RMSProp step equals the oracle update
    on the autograd gradients of the smooth-cosine model (as tests/test_ntm_train_gpu.py::test_train_step_matches_oracle_update)."""
    from ntmtrack import tracker
    kw, B = CASES["a"][0], 2
    cfg = _config(kw, SMOOTH)
    rng = np.random.default_rng(33)
    params = O.init_params(cfg, rng, scale=0.3)       # large weights -> gradient norm above the clip
    feats = np.maximum(rng.standard_normal((B, T, 64, 512)), 0).astype(np.float32) * 3
    gts = rng.uniform(0, 1, size=(B, T, 64)).astype(np.float32)
    offs = rng.uniform(-0.5, 0.5, size=(B, T, 2)).astype(np.float32)
    x = O.serialize_inputs(feats, gts)
    loss_ref, grads_ref, _, _ = OT.loss_and_grads(cfg, params, x, offs)
    names = sorted(grads_ref)
    clipped, gn = O.clip_by_global_norm([grads_ref[k] for k in names], 5.0)
    new_ref = {k: O.rmsprop_step(params[k].astype(np.float64), g, np.ones_like(g), np.zeros_like(g))[0] for k, g in zip(names, clipped)}

    trk = tracker.NTMOffsetTracker(B, T, vgg_weights=None, device=cuda, similarity=SMOOTH)
    assert trk.cell.similarity == SMOOTH and trk.cell.plan(B)["bwd_kernel"] == "fix"
    trk.cell.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, input_dim=D)
    fmap = np.zeros((B * T, 28, 28, 512), np.float32)
    for i, (y, xx) in enumerate(O.CONV43_POINTS):
        fmap[:, y, xx, :] = feats.reshape(B * T, 64, 512)[:, i]
    loss, _ = trk.loss_and_grads(torch.from_numpy(fmap).to(cuda), torch.from_numpy(gts[:, 0].copy()).to(cuda), torch.from_numpy(offs).to(cuda))
    trk.opt.step()
    torch.cuda.synchronize()
    np.testing.assert_allclose(float(loss.cpu()), loss_ref, rtol=1e-4)
    np.testing.assert_allclose(float(trk.opt.gnorm.cpu()), gn, rtol=2e-3)
    assert gn > 5.0
    got = trk.cell.state_dict()
    for k in names:
        delta_ref = new_ref[k] - params[k]
        err = np.max(np.abs(got[k].numpy().astype(np.float64) - new_ref[k]))
        # fp32 storage of the parameter (|p| <= 0.3 -> half an ulp = 1.5e-8) plus 0.5 % of the step
        assert err <= 3e-8 + 5e-3 * np.max(np.abs(delta_ref)), "%s: %.3e (step %.3e)" % (k, err, np.max(np.abs(delta_ref)))


def test_copy_task_in_smooth_cosine_mode_matches_the_oracle(cuda):
    """CopyTask(similarity="smooth_cosine"), L = 4: loss and every gradient against float64 autograd of the smooth-cosine model
    (bounds of tests/test_copy_task_gpu.py, the gradient bound by this file's rule)."""
    from ntmtrack.copy_task import CopyTask, make_batch
    B, L = 3, 4
    task = CopyTask(B, L, hidden_size=100, device=cuda, seed=2, init_scale=0.2, similarity=SMOOTH)
    sd = {k: v.numpy() for k, v in task.cell.state_dict().items()}
    kw = dict(mem_size=128, mem_dim=20, shift_range=1, controller_hidden_size=100, controller_num_layers=1, write_head_size=1, read_head_size=1)
    bits = torch.randint(0, 2, (B, L, 3), generator=torch.Generator().manual_seed(1)).float()
    x, y = make_batch(bits)

    def oracle(similarity, dtype):
        cfg = O.NTMConfig(4, 4, similarity=similarity, **kw)
        pt = {k: torch.tensor(v, dtype=dtype, requires_grad=True) for k, v in sd.items()}
        logits, _ = OT.loop(cfg, pt, x.to(dtype))
        p, yl = torch.sigmoid(logits), y.to(dtype)
        loss = (-(yl * torch.log(p + 1e-7) + (1 - yl) * torch.log(1 - p + 1e-7))).mean()     # tf.losses.log_loss
        loss.backward()
        return float(loss.detach()), logits.detach().numpy(), {k: v.grad.numpy() for k, v in pt.items()}

    loss_ref, logits_ref, grads_ref = oracle(SMOOTH, torch.float64)
    _l32, _lg32, grads32 = oracle(SMOOTH, torch.float32)
    _la, logits_a, _ga = oracle("as_coded", torch.float64)
    assert np.max(np.abs(logits_ref - logits_a)) > 2e-4                    # the modes are 5.9e-4 apart here: 30x the bound below
    loss, lg = task.loss_and_grads(x.to(cuda), y.to(cuda))
    torch.cuda.synchronize()
    np.testing.assert_allclose(lg.cpu().numpy(), logits_ref, atol=2e-5, rtol=0)
    np.testing.assert_allclose(float(loss.cpu()), loss_ref, rtol=1e-5)
    got = task.cell.params.to_tf(grad=True)
    for k in sorted(sd):
        err, err32 = _relerr(got[k].numpy(), grads_ref[k]), _relerr(grads32[k].astype(np.float64), grads_ref[k])
        assert err <= max(1e-4, 3 * err32), (k, err, err32)


def test_a_checkpoint_carries_the_similarity_mode(cuda, tmp_path):
    """Saved by a smooth-cosine tracker: an as-coded tracker refuses it, a smooth-cosine one resumes from it bit for bit; a file
    without the field (written before the mode existed) is as coded."""
    from ntmtrack import _lib, tracker
    B, frames = 2, 2
    g = torch.Generator().manual_seed(1)
    fmap = torch.relu(torch.randn((B * frames, 28, 28, 512), generator=g)).to(cuda)
    gts0 = torch.rand((B, 64), generator=g).to(cuda)
    offs = (torch.rand((B, frames, 2), generator=g) - 0.5).to(cuda)
    a = tracker.NTMOffsetTracker(B, frames, vgg_weights=None, device=cuda, seed=3, learning_rate=1e-2, similarity=SMOOTH)
    a.loss_and_grads(fmap, gts0, offs); a.opt.step()
    path = a.save_checkpoint(str(tmp_path / "smooth.pt"))
    assert torch.load(path, map_location="cpu", weights_only=True)["similarity"] == SMOOTH
    a.loss_and_grads(fmap, gts0, offs); a.opt.step()
    coded = tracker.NTMOffsetTracker(B, frames, vgg_weights=None, device=cuda, seed=3, learning_rate=1e-2)
    before = coded.cell.params.flat.clone()
    with pytest.raises(_lib.NtkError, match="similarity"):
        coded.load_checkpoint(path)
    assert torch.equal(coded.cell.params.flat, before)                     # refused before anything was copied
    b = tracker.NTMOffsetTracker(B, frames, vgg_weights=None, device=cuda, seed=99, learning_rate=1e-2, similarity=SMOOTH)
    b.load_checkpoint(path)
    assert b.opt.global_step == 1
    b.loss_and_grads(fmap, gts0, offs); b.opt.step()
    torch.cuda.synchronize()
    assert torch.equal(a.cell.params.flat, b.cell.params.flat) and torch.equal(a.opt.ms, b.opt.ms) and torch.equal(a.opt.mom, b.opt.mom)
    # a checkpoint without the field loads into an as-coded tracker and is refused by a smooth-cosine one
    old = str(tmp_path / "old.pt")
    coded.save_checkpoint(old)
    ck = torch.load(old, map_location="cpu", weights_only=True)
    del ck["similarity"]
    torch.save(ck, old)
    coded.load_checkpoint(old)
    with pytest.raises(_lib.NtkError, match="similarity"):
        b.load_checkpoint(old)


def test_heatmap_and_two_step_trackers_take_the_keyword(cuda):
    """NTMHeatmapTracker / NTMTwoStepTracker(similarity="smooth_cosine"): the keyword reaches the cell and the loss of one
    loss_and_grads is the float64 oracle's in smooth-cosine mode (rtol 1e-4; inputs and bound of tests/test_heatmap_gpu.py and
    tests/test_twostep_gpu.py).  This pins the plumbing; at these small inputs the two models' losses are close (printed), and it is
    the parity cases above that tell the modes' arithmetic apart."""
    from ntmtrack import heatmap, twostep
    B, frames, F = 2, 3, 9
    kw = dict(mem_size=64, mem_dim=8, shift_range=1, controller_hidden_size=32, controller_num_layers=1, write_head_size=1, read_head_size=2)

    def oracle_loss(cfg_args, sd, x, loss_of):
        out = []
        for similarity in (SMOOTH, "as_coded"):
            cfg = O.NTMConfig(*cfg_args, similarity=similarity, **kw)
            pt = {k: torch.tensor(v, dtype=torch.float64) for k, v in sd.items()}
            out.append(float(loss_of(OT.loop(cfg, pt, torch.tensor(x, dtype=torch.float64))[0])))
        return out

    # heatmap: sequential presentation, per-frame F-way softmax cross-entropy
    C = 16
    rng = np.random.default_rng(6)
    trk = heatmap.NTMHeatmapTracker(B, frames, F, C, mem_size=64, mem_dim=8, hidden_size=32, read_head_size=2, write_head_size=1,
                                    init_scale=0.2, device=cuda, seed=5, similarity=SMOOTH)
    assert trk.cell.similarity == SMOOTH
    sd = {k: v.numpy() for k, v in trk.cell.state_dict().items()}
    feats = np.maximum(rng.standard_normal((B, frames, F, C)), 0).astype(np.float32)
    gts = rng.uniform(0, 1, size=(B, frames, F)).astype(np.float32)
    gts /= gts.sum(2, keepdims=True)

    def heat_loss(logits):
        z = logits.reshape(B, -1)[:, F:].reshape(B, frames - 1, 2 * F + 1)[:, :, 1:].reshape(B, frames - 1, F, 2)[:, :, :, 1]
        return -(torch.tensor(gts[:, 1:], dtype=torch.float64) * torch.log_softmax(z, dim=2)).sum() / (frames - 1)

    ref, ref_as_coded = oracle_loss((C + 3, 1), sd, O.serialize_sequential(feats, gts), heat_loss)
    loss, _probs = trk.loss_and_grads(torch.from_numpy(feats.reshape(B * frames, 3, 3, C)).to(cuda), torch.from_numpy(gts).to(cuda))
    torch.cuda.synchronize()
    print("loss: smooth cosine %.6f, as coded %.6f (float64 oracle), HIP %.6f" % (ref, ref_as_coded, float(loss.cpu())))
    np.testing.assert_allclose(float(loss.cpu()), ref, rtol=1e-4)
    assert bool(torch.isfinite(trk.cell.params.grad).all())

    # two-step: presentation + query steps, softmax cross-entropy on soft labels, write_first
    Dm = 36
    rng = np.random.default_rng(6)
    kw["write_first"] = True
    trk = twostep.NTMTwoStepTracker(B, frames, F, Dm, mem_size=64, mem_dim=8, hidden_size=32, read_head_size=2, write_head_size=1,
                                    write_first=True, init_scale=0.2, device=cuda, seed=5, similarity=SMOOTH)
    assert trk.cell.similarity == SMOOTH
    sd = {k: v.numpy() for k, v in trk.cell.state_dict().items()}
    feat = np.maximum(rng.standard_normal((B, frames, Dm)), 0).astype(np.float32)
    gts = (rng.uniform(0, 1, size=(B, frames, F)) > 0.7).astype(np.float32)
    q = torch.softmax(torch.tensor(O.two_step_labels(gts.astype(np.float64))), dim=2)
    ref, ref_as_coded = oracle_loss((1 + Dm + F, F + 1), sd, O.two_step_inputs(feat, gts[:, 0]),
                                    lambda logits: -(q * torch.log_softmax(logits, dim=2)).sum() / ((2 * frames - 1) * B))
    loss, _probs = trk.loss_and_grads(torch.from_numpy(feat).to(cuda), torch.from_numpy(gts).to(cuda))
    torch.cuda.synchronize()
    print("loss: smooth cosine %.6f, as coded %.6f (float64 oracle), HIP %.6f" % (ref, ref_as_coded, float(loss.cpu())))
    np.testing.assert_allclose(float(loss.cpu()), ref, rtol=1e-4)
    assert bool(torch.isfinite(trk.cell.params.grad).all())
