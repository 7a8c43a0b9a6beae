"""GPU: NTM cells with a deep (MultiRNNCell, L >= 2) controller on the deep persistent kernels (ntk_ntm_seq_fwd_deep /
ntk_ntm_seq_bwd_deep) -- the C entries directly, the long horizon, BPTT through the tracking head, the step-wise form, bitwise
reproducibility, the static unroll and the online tracker, against the oracles."""
import ctypes

import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O
from oracle import ntm_oracle_torch as OT

pytestmark = pytest.mark.gpu


def _relerr(a, b):
    return float(np.max(np.abs(a - b)) / (np.max(np.abs(b)) + 1e-30))


def _params(cfg, seed, scale=0.3):
    rng = np.random.default_rng(seed)
    params = O.init_params(cfg, rng, scale=scale)
    for k in params:
        if k.endswith("biases"):
            params[k] = rng.uniform(-0.2, 0.2, size=params[k].shape).astype(np.float32)
    return params, rng


def _cell(kw, params, cuda, D):
    from ntmtrack.ntm import NTMCell, StackedNTMCell
    cell = NTMCell(kw.pop("O"), device=cuda, **kw)
    assert isinstance(cell, StackedNTMCell)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, input_dim=D)
    return cell


ODD = dict(mem_size=64, mem_dim=12, shift_range=1, controller_hidden_size=24, write_head_size=2, read_head_size=2)


@pytest.mark.parametrize("layers,extra", [(2, {}), (3, {}), (4, {}), (3, dict(shift_range=3, write_first=True))])
def test_cabi_deep_forward_matches_oracle(cuda, layers, extra):
    """ntk_ntm_seq_deep_pack + ntk_gemm_nt_f32 + ntk_ntm_seq_fwd_deep called through ctypes, as a C caller would, at odd shapes
    (mem 64x12, hid 24, 2 read + 2 write heads, B 3, S 20): logits and every returned state against the numpy oracle."""
    from ntmtrack import _lib
    from ntmtrack.ntm import gemm_nt
    kw = dict(ODD, controller_num_layers=layers, **extra)
    D, O_, B, S = 11, 3, 3, 20
    cfg = O.NTMConfig(D, O_, **kw)
    params, rng = _params(cfg, 70 + layers)
    cell = _cell(dict(kw, O=O_), params, cuda, D)
    L, P, d, hid = _lib.lib(), _lib.ptr, cell.dims, 24
    assert L.ntk_ntm_seq_deep_supported(B, 64, 12, 2, 2, hid, kw["shift_range"], O_, layers) == 1
    xs = rng.standard_normal((B, S, D)).astype(np.float32)
    ldx = (D + 3) // 4 * 4
    X = torch.zeros((B, S, ldx), device=cuda)
    X[:, :, :D] = torch.from_numpy(xs).to(cuda)
    n = [ctypes.c_size_t() for _ in range(3)]
    assert L.ntk_ntm_seq_deep_packed_floats(D, 2, 12, hid, layers, *[ctypes.byref(v) for v in n]) == 0
    Wx0, Wf, Wb = [torch.empty(v.value, device=cuda) for v in n]
    o0 = cell.params.lower_off[0][0]
    lowerT = cell.params.flat[o0:]
    st = _lib.stream()
    _lib.check(L.ntk_ntm_seq_deep_pack(D, 2, 12, hid, layers, P(lowerT), P(cell.top.params.view("WxT")), P(cell.top.params.view("Wr")),
                                       P(Wx0), P(Wf), P(Wb), st), "pack")
    xproj = gemm_nt(X.view(B * S, ldx), Wx0.view(4 * hid, ldx))
    s0 = cell.zero_state(B)
    logits, outs = torch.empty((B, S, O_), device=cuda), torch.empty((B, S, O_), device=cuda)
    new = cell.state_placeholder(B)
    _lib.check(L.ntk_ntm_seq_fwd_deep(
        B, S, 64, 12, 2, 2, hid, kw["shift_range"], O_, layers, 1 if kw.get("write_first") else 0, D,
        P(X), P(xproj), P(Wf), P(cell.top.params.view("Wa")), P(s0["M"]), P(s0["w"]), P(s0["read"]), P(s0["controller_state"]),
        P(logits), P(outs), P(new["M"]), P(new["w"]), P(new["read"]), P(new["controller_state"]), *([None] * 15), st), "fwd_deep")
    torch.cuda.synchronize()
    oouts, ologits, fin = O.loop_ntm_tracker(cfg, params, xs)
    np.testing.assert_allclose(logits.cpu().numpy(), ologits, atol=3e-5)
    np.testing.assert_allclose(outs.cpu().numpy(), oouts, atol=3e-5)
    for key in ("M", "w", "read", "controller_state"):
        np.testing.assert_allclose(new[key].cpu().numpy(), fin[key], atol=3e-5, err_msg=key)


def test_long_horizon_drift_at_the_tracker_shape(cuda):
    """L = 2 at the tracker's shape (mem 128x20, 4 read + 1 write head, hid 200, D 514), B 2, S = 1300 strictly sequential
    steps: tanh(logit) within 1e-4 of the float64 oracle, the single-layer drift test's bound."""
    from ntmtrack.ntm import LoopNTMTracker
    kw = dict(mem_size=128, mem_dim=20, shift_range=1, controller_hidden_size=200, controller_num_layers=2, write_head_size=1,
              read_head_size=4)
    cfg = O.NTMConfig(514, 2, **kw)
    rng = np.random.default_rng(123)
    params = O.init_params(cfg, rng, scale=0.05)
    B, T = 2, 20
    feats = np.maximum(rng.standard_normal((B, T, 64, 512)), 0).astype(np.float32)
    x = O.serialize_inputs(feats, rng.uniform(0, 1, size=(B, T, 64)).astype(np.float32))
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    _, logits, fin = O.loop_ntm_tracker(cfg, p64, x.astype(np.float64))
    trk = LoopNTMTracker(T * 65, 2, None, device=cuda, **kw)
    trk.cell.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    _o, l_gpu = trk(torch.from_numpy(x).to(cuda))
    torch.cuda.synchronize()
    assert trk.cell.last_form == "fused"
    err = np.max(np.abs(np.tanh(l_gpu.cpu().numpy()) - np.tanh(logits)))
    print("deep (L=2) 1300-step drift of tanh(logit) vs float64: %.3e" % err)
    assert err < 1e-4, err
    assert np.max(np.abs(trk.last_state["M"].cpu().numpy() - fin["M"])) < 1e-4


def _offset_tracker_case(cuda, layers, T, seed):
    from ntmtrack import tracker
    B = 2
    kw = dict(mem_size=64, mem_dim=8, shift_range=1, controller_hidden_size=32, controller_num_layers=layers,
              write_head_size=1, read_head_size=2)
    cfg = O.NTMConfig(514, 2, **kw)
    rng = np.random.default_rng(seed)
    params = O.init_params(cfg, rng, scale=0.15)
    for k in params:
        if k.endswith("biases"):
            params[k] = rng.uniform(-0.15, 0.15, size=params[k].shape).astype(np.float32)
    feats = np.maximum(rng.standard_normal((B, T, 64, 512)), 0).astype(np.float32)
    gts = rng.uniform(0, 1, size=(B, T, 64)).astype(np.float32)
    offs = rng.uniform(-0.5, 0.5, size=(B, T, 2)).astype(np.float32)
    trk = tracker.NTMOffsetTracker(B, T, vgg_weights=None, mem_size=64, mem_dim=8, hidden_size=32, num_layers=layers,
                                   read_head_size=2, write_head_size=1, device=cuda, learning_rate=1e-2)
    trk.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    fmap = np.zeros((B * T, 28, 28, 512), np.float32)
    for i, (y, xx) in enumerate(O.CONV43_POINTS):
        fmap[:, y, xx, :] = feats.reshape(B * T, 64, 512)[:, i]
    args = (torch.from_numpy(fmap).to(cuda), torch.from_numpy(gts[:, 0].copy()).to(cuda), torch.from_numpy(offs).to(cuda))
    return cfg, params, O.serialize_inputs(feats, gts), offs, trk, args


@pytest.mark.parametrize("layers", [2, 3])
def test_fused_bptt_matches_autograd_oracle(cuda, layers):
    """NTMOffsetTracker(num_layers=L).loss_and_grads on the fused kernels, T = 2 frames (130 steps): every variable's gradient,
    lower LSTM layers included, within 2e-3 relative of float64 torch autograd."""
    cfg, params, x, offs, trk, args = _offset_tracker_case(cuda, layers, 2, 50 + layers)
    loss_ref, grads_ref, _, _ = OT.loss_and_grads(cfg, params, x, offs)
    loss, _ = trk.loss_and_grads(*args)
    torch.cuda.synchronize()
    assert trk.cell.last_form == "fused"
    np.testing.assert_allclose(float(loss.cpu()), loss_ref, rtol=1e-4)
    got = trk.cell.state_dict(grad=True)
    assert sorted(got) == sorted(grads_ref)
    errs = {k: _relerr(got[k].numpy(), grads_ref[k]) for k in sorted(grads_ref)}
    print("L=%d fused BPTT relative gradient error vs float64 autograd: %s" % (layers, {k: "%.1e" % v for k, v in errs.items()}))
    assert max(errs.values()) < 2e-3, errs


def test_fused_bptt_ten_frames_within_the_float32_oracle_error(cuda):
    """T = 10 frames (650 steps), L = 2: each tensor's gradient within max(1e-4 of its largest entry, 3x the float32 oracle's own
    error) of float64 autograd (the DNC precedent)."""
    cfg, params, x, offs, trk, args = _offset_tracker_case(cuda, 2, 10, 61)
    _, grads64, _, _ = OT.loss_and_grads(cfg, params, x, offs)
    _, grads32, _, _ = OT.loss_and_grads(cfg, params, x, offs, dtype=torch.float32)
    trk.loss_and_grads(*args)
    torch.cuda.synchronize()
    assert trk.cell.last_form == "fused"
    got = trk.cell.state_dict(grad=True)
    worst, bad = {}, {}
    for k, ref in grads64.items():
        scale = float(np.max(np.abs(ref))) + 1e-30
        err = float(np.max(np.abs(got[k].numpy().astype(np.float64) - ref))) / scale
        err32 = float(np.max(np.abs(grads32[k].astype(np.float64) - ref))) / scale
        worst[k] = (err, err32)
        if not err <= max(1e-4, 3 * err32):                    # not `err > ...`: a NaN gradient must not pass
            bad[k] = (err, err32)
    print("T=10 L=2 relative gradient error (HIP, float32 oracle) vs float64: %s" % {k: ("%.1e" % a, "%.1e" % b) for k, (a, b) in worst.items()})
    assert not bad, bad


def test_fused_equals_stepwise_and_is_bitwise_reproducible(cuda, monkeypatch):
    """The same cell, fused and step-wise (fused = False; NTK_NTM_DEEP_FORM=stepwise does the same): logits within 1e-5 over
    S = 130, gradients within 1e-4 relative; two fused forward + BPTT runs are bitwise equal."""
    cfg, params, x, offs, trk, args = _offset_tracker_case(cuda, 2, 2, 77)
    cell = trk.cell

    def run():
        X, st0, logits, rec = trk.forward_features(args[0], args[1], record=True)
        from ntmtrack import tracker
        _loss, _pred, dlog = tracker.offset_loss(logits, args[2], trk.T)
        g0 = cell.backward_sequence(X, st0, rec, dlog)
        cell.init_state_backward(g0, trk.B)
        torch.cuda.synchronize()
        return logits.clone(), cell.params.grad.clone(), {k: v.clone() for k, v in g0.items()}, cell.last_form

    l1, g1, s1, f1 = run()
    l2, g2, s2, f2 = run()
    assert f1 == f2 == "fused"
    assert torch.equal(l1, l2) and torch.equal(g1, g2) and all(torch.equal(s1[k], s2[k]) for k in s1)
    cell.fused = False
    l3, _g3, _s3, f3 = run()
    assert f3 == "stepwise"
    sd3 = cell.state_dict(grad=True)
    cell.fused = None
    monkeypatch.setenv("NTK_NTM_DEEP_FORM", "stepwise")
    _l4, _g4, _s4, f4 = run()
    assert f4 == "stepwise"
    monkeypatch.delenv("NTK_NTM_DEEP_FORM")
    run()
    sd1 = cell.state_dict(grad=True)
    assert cell.last_form == "fused"
    assert float((l1 - l3).abs().max()) < 1e-5
    for k in sd1:
        assert _relerr(sd1[k].numpy(), sd3[k].numpy()) < 1e-4, k
    for k in s1:
        assert _relerr(s1[k].cpu().numpy(), _s3[k].cpu().numpy()) < 1e-4, k


def test_static_unroll_on_a_fused_deep_cell_returns_every_state(cuda):
    """PlainNTMTracker on a 2-layer cell that runs fused: S + 1 states, controller_state = [c_0, h_0, c_1, h_1], against the oracle."""
    from ntmtrack.ntm import PlainNTMTracker
    kw = dict(ODD, controller_num_layers=2, write_head_size=1)
    cfg = O.NTMConfig(11, 3, **kw)
    params, rng = _params(cfg, 8)
    B, S = 2, 6
    plain = PlainNTMTracker(S, 3, device=cuda, **kw)
    plain.cell.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()})
    xs = rng.standard_normal((B, S, 11)).astype(np.float32)
    outs, logits, states, debugs = plain(torch.from_numpy(xs).to(cuda))
    torch.cuda.synchronize()
    assert plain.cell.last_form == "fused"
    _oo, ologits, _fin, ostates = O.loop_ntm_tracker(cfg, params, xs, return_states=True)
    assert len(states) == S + 1
    np.testing.assert_allclose(logits.cpu().numpy(), ologits, atol=3e-5)
    for t in range(S):
        for key in ("M", "w", "read", "controller_state"):
            assert states[t + 1][key].shape == ostates[t][key].shape, (key, t)
            np.testing.assert_allclose(states[t + 1][key].cpu().numpy(), ostates[t][key], atol=3e-5, err_msg="%s step %d" % (key, t))
    assert states[1]["controller_state"].shape == (B, 2 * 24 * 2)
    assert debugs["w"].shape == (B, S, 3, 64) and debugs["M"].shape == (B, S, 64, 12)


def test_online_tracker_on_a_deep_cell_matches_oracle(cuda):
    """online.NTMTracker with a 2-layer cell: two frames against the numpy chain (test_online_gpu.py's two-frame test)."""
    from ntmtrack import online
    from ntmtrack.ntm import NTMCell
    from ntmtrack.vgg import VGG16Conv43
    from oracle import online_oracle as OO
    rng = np.random.default_rng(5)
    ws = O.init_vgg_weights(rng)
    cfg = O.NTMConfig(514, 2, mem_size=128, mem_dim=20, shift_range=1, controller_hidden_size=200, controller_num_layers=2,
                      write_head_size=1, read_head_size=4)
    params = O.init_params(cfg, rng, scale=0.05)
    H, W = 90, 120
    frames = [rng.uniform(0, 255, size=(H, W, 3)).astype(np.float32) for _ in range(2)]
    region = (40.0, 30.0, 36.0, 27.0)
    x1, y1, w, h = region
    nb = online.normalize_bbox((W, H), (y1, x1, y1 + h, x1 + w))
    cb = online.calculate_cropbox(nb, 8, 6)
    tr = online.calculate_transformation(cb)
    ws64 = {k: (wt.astype(np.float64), b.astype(np.float64)) for k, (wt, b) in ws.items()}
    p64 = {k: v.astype(np.float64) for k, v in params.items()}
    st = O.zero_state(cfg, p64, 1)

    def o_frame(img, first, st):
        crop = OO.crop_and_resize(img.astype(np.float64) - np.array(online.VGG_MEAN), cb, 224, 224)
        fmap = O.vgg16_conv43(crop[None], ws64)
        gt = online.generate_gt(online.apply_transformation(nb, tr), 8, 6) if first else None
        blk = OO.frame_block(cfg, fmap, gt)
        _, logits, st = O.loop_ntm_tracker(cfg, p64, blk[None], state=st)
        return np.tanh(logits[0, -1]), st
    _, st = o_frame(frames[0], True, st)
    offs, st = o_frame(frames[1], False, st)

    cell = NTMCell(2, mem_size=128, mem_dim=20, controller_hidden_size=200, controller_num_layers=2, write_head_size=1,
                   read_head_size=4, device=cuda)
    cell.load_state_dict({k: torch.from_numpy(v) for k, v in params.items()}, input_dim=514)
    trk = online.NTMTracker(frames[0], region, cell, VGG16Conv43(ws, device=cuda), device=cuda)
    got = trk.track(frames[1])
    torch.cuda.synchronize()
    assert cell.last_form == "fused"
    np.testing.assert_allclose(trk.offsets, offs, atol=1e-4)
    assert isinstance(got, online.Rectangle)
