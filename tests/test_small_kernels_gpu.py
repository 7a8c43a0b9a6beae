"""GPU: the small kernels around the recurrent cores -- the single-workgroup loss heads, the serialisers, the optimiser and
the elementwise kernels (csrc/head_loss.hip, csrc/optimizer.hip, csrc/step_api.hip, transpose_pad of csrc/ntm_seq_bwd.hip) -- each on its own,
against the float64 oracle (oracle/ntm_oracle.py; gradients from float64 torch autograd), at the sizes where their loops
change shape: a lane stride that runs or not, a wave stride with and without a remainder, one workgroup and several, the
grid-stride loops.  Every output buffer is NaN before the call.

Tolerances are the ones the existing tests of each kernel use (rtol 1e-5 on a loss, atol 1e-6 on probabilities and gradients,
1e-7 on the two-step gradient).  Where a case needs more, the bound is 4 x the gap between an fp32 numpy restatement of the
same formula and the float64 oracle on the same inputs -- reference against reference, measured on the CPU inside the test and
printed (the device's expf / logf / tanhf are not numpy's, hence the factor).  `tol()` takes the larger of the two."""
import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O
from small_kernel_util import lstm_pointwise64, nan_tensor, still_guard, to_dev, vptr

pytestmark = pytest.mark.gpu


def tol(case, base, measured):
    bound = max(float(base), 4.0 * float(measured))
    if bound > base:
        print("tolerance %s: fp32 restatement vs float64 oracle %.3e, base %.3e, bound used %.3e" % (case, measured, base, bound))
    return bound


def gap(a32, a64):
    return float(np.max(np.abs(np.asarray(a32, dtype=np.float64) - np.asarray(a64, dtype=np.float64)))) if np.size(a64) else 0.0


def call(name, *args):
    from ntmtrack import _lib
    _lib.check(getattr(_lib.lib(), name)(*(list(args) + [_lib.stream()])), name)


def host(t):
    return t.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------
# heat-map head: softmax cross entropy over the feature-delimiter steps
# ---------------------------------------------------------------------------------------------------------
def heatmap_restated(logits, gt, T, dt):
    """The kernel's formula in dtype dt: (loss, probs, dlogits).  In float64 the loss and the probabilities are the oracle's."""
    B, F = gt.shape[0], gt.shape[2]
    z = O.heatmap_gather(logits, T, F).astype(dt)
    y = gt.astype(dt)
    inv = dt(1.0) / dt(T - 1)
    zz = z - z.max(axis=2, keepdims=True)
    lse = np.log(np.exp(zz).sum(axis=2, keepdims=True, dtype=dt))
    sl = y.sum(axis=2, keepdims=True, dtype=dt)
    loss = (sl[..., 0] * lse[..., 0] - (y * zz).sum(axis=2, dtype=dt)).sum(dtype=dt) * inv
    p = np.exp(zz - lse)
    d = np.zeros(logits.shape, dt).reshape(B, -1)
    dz = (p * sl - y) * inv
    S = F + (T - 1) * (2 * F + 1)
    for t in range(1, T):
        base = F + (t - 1) * (2 * F + 1) + 1
        d[:, base + 1:base + 2 * F:2] = dz[:, t - 1]
    assert d.shape[1] == S
    return float(loss), p, d.reshape(logits.shape)


def heatmap_case(cuda, B, T, F, rng, spread=2.0, zero_row=False, null=None):
    S = F + (T - 1) * (2 * F + 1)
    logits = (rng.standard_normal((B, S, 1)) * spread).astype(np.float32)
    if spread > 10:
        logits = rng.uniform(-spread, spread, size=(B, S, 1)).astype(np.float32)
    gt = rng.uniform(0, 1, size=(B, T - 1, F)).astype(np.float32)
    gt /= gt.sum(2, keepdims=True)
    gt[0, 0] *= 0.7                                      # labels need not sum to one
    if zero_row:
        gt[B - 1, T - 2] = 0.0                           # sl = 0: the gradient of that row is exactly -0 * ... = 0
    loss64, p64, d64 = heatmap_restated(logits, gt, T, np.float64)
    o_loss, o_probs = O.heatmap_ce_loss(logits, gt, T)
    np.testing.assert_allclose(loss64, o_loss, rtol=1e-12, atol=1e-300)
    np.testing.assert_allclose(p64, o_probs, rtol=0, atol=1e-15)
    lt = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    zt = lt.reshape(B, -1)[:, F:].reshape(B, T - 1, 2 * F + 1)[:, :, 1:].reshape(B, T - 1, F, 2)[:, :, :, 1]
    (-(torch.tensor(gt, dtype=torch.float64) * torch.log_softmax(zt, dim=2)).sum() / (T - 1)).backward()
    np.testing.assert_allclose(d64, lt.grad.numpy(), atol=1e-13)
    loss32, p32, d32 = heatmap_restated(logits, gt, T, np.float32)
    name = "heatmap B%d T%d F%d spread%g" % (B, T, F, spread)
    tl, tg = to_dev(logits, cuda), to_dev(gt, cuda)
    probs = None if null == "probs" else nan_tensor((B, T - 1, F), cuda)
    loss = None if null == "loss" else nan_tensor(1, cuda)
    dlog = None if null == "dlogits" else nan_tensor((B, S, 1), cuda)
    call("ntk_heatmap_ce_loss", vptr(tl), vptr(tg), vptr(probs), vptr(loss), vptr(dlog), B, T, F)
    if loss is not None:
        assert abs(float(host(loss)[0]) - loss64) <= tol(name + " loss", 1e-5 * abs(loss64), abs(loss32 - loss64)), (name, float(host(loss)[0]), loss64)
    if probs is not None:
        assert gap(host(probs), p64) <= tol(name + " probs", 1e-6, gap(p32, p64)), name
    if dlog is not None:
        got = host(dlog)
        assert gap(got, d64) <= tol(name + " dlogits", 1e-6, gap(d32, d64)), name
        mask = np.ones(got.shape, bool).reshape(B, -1)
        for t in range(1, T):
            base = F + (t - 1) * (2 * F + 1) + 1
            mask[:, base + 1:base + 2 * F:2] = False
        assert not got.reshape(B, -1)[mask].any(), name            # zero (not NaN, not stale) off the gathered steps


@pytest.mark.parametrize("BT", [(1, 2), (4, 5), (17, 2), (5, 8)], ids=["rows1", "rows16", "rows17", "rows35"])
@pytest.mark.parametrize("F", [1, 63, 64, 65, 130])
def test_heatmap_ce_loss_shapes(cuda, F, BT):
    heatmap_case(cuda, BT[0], BT[1], F, np.random.default_rng(100 * F + BT[0]))


def test_heatmap_ce_loss_wide_logits_zero_labels_and_null_outputs(cuda):
    rng = np.random.default_rng(11)
    heatmap_case(cuda, 5, 8, 130, rng, spread=80.0)                   # max subtraction: exp(80) overflows nothing
    heatmap_case(cuda, 3, 4, 65, rng, zero_row=True)
    for null in ("probs", "loss", "dlogits"):
        heatmap_case(cuda, 3, 7, 65, rng, null=null)


# ---------------------------------------------------------------------------------------------------------
# two-step head: (F + 1)-way cross entropy on softmaxed labels, one wave per row
# ---------------------------------------------------------------------------------------------------------
def two_step_case(cuda, B, T, F, rng, real_valued=False, null=None):
    """Measured: with one row (B 1, T 1) the 1 / (B (2T - 1)) factor is 1 and the 1e-7 of the gradient does not hold for the
    formula itself: fp32 restatement against the float64 oracle 5.9e-8 (F 1), 4.0e-8 (F 64), 4.5e-8 (F 128), bounds used 2.3e-7,
    1.6e-7, 1.8e-7.  Every other case keeps the base tolerances."""
    S, K = 2 * T - 1, F + 1
    logits = (rng.standard_normal((B, S, K)) * 2).astype(np.float32)
    gt = (rng.uniform(0, 1, size=(B, T, F)) > 0.8).astype(np.float32)
    if real_valued:
        gt = rng.uniform(0, 3, size=(B, T, F)).astype(np.float32)
    elif T > 1:
        gt[0, 1] = rng.uniform(0, 3, size=F).astype(np.float32)
    loss64, p64, d64 = O.two_step_ce_loss(logits.astype(np.float64), gt.astype(np.float64))
    loss32, p32, d32 = O.two_step_ce_loss(logits, gt)                 # the same function in fp32
    lt = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    q = torch.softmax(torch.tensor(O.two_step_labels(gt.astype(np.float64))), dim=2)
    (-(q * torch.log_softmax(lt, dim=2)).sum() / (S * B)).backward()
    np.testing.assert_allclose(lt.grad.numpy(), d64, atol=1e-14)
    name = "two_step B%d T%d F%d%s" % (B, T, F, " real" if real_valued else "")
    tl, tg = to_dev(logits, cuda), to_dev(gt, cuda)
    probs = None if null == "probs" else nan_tensor((B, S, K), cuda)
    loss = None if null == "loss" else nan_tensor(1, cuda)
    dlog = None if null == "dlogits" else nan_tensor((B, S, K), cuda)
    call("ntk_two_step_ce_loss", vptr(tl), vptr(tg), vptr(probs), vptr(loss), vptr(dlog), B, T, F)
    if loss is not None:
        assert abs(float(host(loss)[0]) - loss64) <= tol(name + " loss", 1e-5 * abs(loss64), abs(float(loss32) - loss64)), (name, float(host(loss)[0]), loss64)
    if probs is not None:
        assert gap(host(probs), p64) <= tol(name + " probs", 1e-6, gap(p32, p64)), name
    if dlog is not None:
        assert gap(host(dlog), d64) <= tol(name + " dlogits", 1e-7, gap(d32, d64)), name


@pytest.mark.parametrize("BT", [(1, 1), (3, 3), (16, 1), (17, 1), (8, 3)], ids=["rows1", "rows15", "rows16", "rows17", "rows40"])
@pytest.mark.parametrize("F", [1, 63, 64, 128])
def test_two_step_ce_loss_shapes(cuda, F, BT):
    two_step_case(cuda, BT[0], BT[1], F, np.random.default_rng(200 * F + BT[0]))


def test_two_step_ce_loss_real_valued_heatmaps_and_null_outputs(cuda):
    rng = np.random.default_rng(12)
    two_step_case(cuda, 8, 3, 128, rng, real_valued=True)
    two_step_case(cuda, 3, 3, 64, rng, real_valued=True)
    for null in ("probs", "loss", "dlogits"):
        two_step_case(cuda, 3, 4, 64, rng, null=null)


# ---------------------------------------------------------------------------------------------------------
# offset head: tanh + l2 at the delimiter step of frames 1..T-1
# ---------------------------------------------------------------------------------------------------------
def offset_case(cuda, B, T, NF, Oq, rng):
    S = T * (NF + 1)
    logits = rng.standard_normal((B, S, Oq)).astype(np.float32)
    offs = rng.uniform(-.5, .5, size=(B, T, Oq)).astype(np.float32)
    loss64, pred64 = O.offset_loss(logits.astype(np.float64), offs.astype(np.float64), num_features=NF)
    loss32, pred32 = O.offset_loss(logits, offs, num_features=NF)
    lt = torch.tensor(logits, dtype=torch.float64, requires_grad=True)
    g = lt[:, NF + 1:, :].reshape(B, T - 1, NF + 1, Oq)[:, :, NF, :]
    (0.5 * ((torch.tanh(g) - torch.tensor(offs[:, 1:], dtype=torch.float64)) ** 2).sum()).backward()
    d64 = lt.grad.numpy()
    d32 = np.zeros_like(logits)
    p32 = pred32.astype(np.float32)
    d32.reshape(B, T, NF + 1, Oq)[:, 1:, NF, :] = (p32 - offs[:, 1:]) * (np.float32(1) - p32 * p32)
    name = "offset B%d T%d NF%d O%d" % (B, T, NF, Oq)
    tl, to = to_dev(logits, cuda), to_dev(offs, cuda)
    pred, loss, dlog = nan_tensor((B, T - 1, Oq), cuda), nan_tensor(1, cuda), nan_tensor((B, S, Oq), cuda)
    call("ntk_offset_loss", vptr(tl), vptr(to), vptr(pred), vptr(loss), vptr(dlog), B, T, NF, Oq)
    assert abs(float(host(loss)[0]) - float(loss64)) <= tol(name + " loss", 1e-5 * abs(float(loss64)), abs(float(loss32) - float(loss64))), name
    assert gap(host(pred), pred64) <= tol(name + " pred", 1e-6, gap(pred32, pred64)), name
    got = host(dlog)
    assert gap(got, d64) <= tol(name + " dlogits", 1e-6, gap(d32, d64)), name
    assert not got[d64 == 0].any(), name                              # zero elsewhere
    # pred null; loss null with dlogits given; the two-call form
    loss_b, dlog_b = nan_tensor(1, cuda), nan_tensor((B, S, Oq), cuda)
    call("ntk_offset_loss", vptr(tl), vptr(to), None, vptr(loss_b), vptr(dlog_b), B, T, NF, Oq)
    assert torch.equal(loss_b, loss) and torch.equal(dlog_b, dlog), name
    dlog_c = nan_tensor((B, S, Oq), cuda)
    call("ntk_offset_loss", vptr(tl), vptr(to), None, None, vptr(dlog_c), B, T, NF, Oq)
    assert torch.equal(dlog_c, dlog), name
    pred2, loss2, dlog2 = nan_tensor((B, T - 1, Oq), cuda), nan_tensor(1, cuda), nan_tensor((B, S, Oq), cuda)
    call("ntk_offset_loss_fwd", vptr(tl), vptr(to), vptr(pred2), vptr(loss2), B, T, NF, Oq)
    call("ntk_offset_loss_bwd", vptr(tl), vptr(to), vptr(dlog2), B, T, NF, Oq)
    assert torch.equal(pred2, pred) and torch.equal(loss2, loss) and torch.equal(dlog2, dlog), name


@pytest.mark.parametrize("Oq", [1, 2, 3])
@pytest.mark.parametrize("NF", [1, 4, 64])
def test_offset_loss_shapes(cuda, NF, Oq):
    offset_case(cuda, 3, 5, NF, Oq, np.random.default_rng(300 + 10 * NF + Oq))


def test_offset_loss_thread_stride(cuda):
    B, T, Oq = 9, 40, 3
    assert B * (T - 1) * Oq > 1024
    offset_case(cuda, B, T, 1, Oq, np.random.default_rng(13))


# ---------------------------------------------------------------------------------------------------------
# copy-task head: sigmoid + tf.losses.log_loss
# ---------------------------------------------------------------------------------------------------------
def log_loss_restated(z, y, dt):
    z, y = z.astype(dt), y.astype(dt)
    eps, one = dt(1e-7), dt(1)
    p = one / (one + np.exp(-z))
    loss = np.sum(-(y * np.log(p + eps) + (one - y) * np.log(one - p + eps)), dtype=dt) / dt(z.size)
    d = (-(y / (p + eps)) + (one - y) / (one - p + eps)) * p * (one - p) / dt(z.size)
    return float(loss), d


@pytest.mark.parametrize("n", [1, 63, 1023, 1024, 1025, 5000])
def test_log_loss(cuda, n):
    """Measured: at n 1 the one element is logit +30 with label 0; fp32 has p = 1 exactly, so the gradient's (1 - p) factor is 0
    against 9.4e-7 in float64: fp32 restatement against float64 9.3e-7, bound used 3.7e-6.  Every other size keeps 1e-6."""
    rng = np.random.default_rng(400 + n)
    z = (rng.standard_normal(n) * 3).astype(np.float32)
    y = (rng.uniform(size=n) > 0.5).astype(np.float32)
    edge = [(30.0, 0.0), (30.0, 1.0), (-30.0, 0.0), (-30.0, 1.0)][:n]
    for i, (zi, yi) in enumerate(edge):
        z[-1 - i], y[-1 - i] = zi, yi
    loss64, d64 = log_loss_restated(z, y, np.float64)
    loss32, d32 = log_loss_restated(z, y, np.float32)
    zt = torch.tensor(z, dtype=torch.float64, requires_grad=True)
    yt, pt = torch.tensor(y, dtype=torch.float64), torch.sigmoid(zt)
    lref = (-(yt * torch.log(pt + 1e-7) + (1 - yt) * torch.log(1 - pt + 1e-7))).mean()
    lref.backward()
    np.testing.assert_allclose(loss64, float(lref.detach()), rtol=1e-12)
    np.testing.assert_allclose(d64, zt.grad.numpy(), atol=1e-13)
    tz, ty = to_dev(z, cuda), to_dev(y, cuda)
    loss, dlog = nan_tensor(1, cuda), nan_tensor(n, cuda)
    call("ntk_log_loss", vptr(tz), vptr(ty), vptr(loss), vptr(dlog), n)
    name = "log_loss n%d" % n
    assert abs(float(host(loss)[0]) - loss64) <= tol(name + " loss", 1e-5 * abs(loss64), abs(loss32 - loss64)), (float(host(loss)[0]), loss64)
    assert gap(host(dlog), d64) <= tol(name + " dlogits", 1e-6, gap(d32, d64))
    loss_b = nan_tensor(1, cuda)
    call("ntk_log_loss", vptr(tz), vptr(ty), vptr(loss_b), None, n)    # dlogits null
    assert torch.equal(loss_b, loss)


# ---------------------------------------------------------------------------------------------------------
# serialisers: bit-exact
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("grid_n", [1, 8])
@pytest.mark.parametrize("C", [4, 512, 1024])
def test_gather_serialize_both_orders(cuda, C, grid_n):
    rng = np.random.default_rng(500 + C + grid_n)
    B, T, g0, gstep = 2, 2, 1, 2
    Hf = Wf = g0 + (grid_n - 1) * gstep + 2
    NF = grid_n * grid_n
    fmap = rng.standard_normal((B * T, Hf, Wf, C)).astype(np.float32)
    gts = rng.uniform(0, 1, size=(B, T, NF)).astype(np.float32)
    points = [(g0 + (i // grid_n) * gstep, g0 + (i % grid_n) * gstep) for i in range(NF)]
    feats = O.extract_features(fmap, points).reshape(B, T, NF, C)
    tf_, tg = to_dev(fmap, cuda), to_dev(gts[:, 0], cuda)
    for ldx in (C + 4, C + 12):
        for with_gt in (True, False):
            ref = O.serialize_inputs(feats, gts if with_gt else np.zeros_like(gts))           # [B, T (NF+1), C+2], delimiter row last
            ref_online = np.roll(ref.reshape(B, T, NF + 1, C + 2), 1, axis=2).reshape(ref.shape)   # quirk Q8: delimiter row first
            for entry, want in (("ntk_gather_serialize", ref), ("ntk_gather_serialize_online", ref_online)):
                X = nan_tensor((B, T * (NF + 1), ldx), cuda)
                call(entry, vptr(tf_), vptr(tg) if with_gt else None, vptr(X), B, T, Hf, Wf, C, ldx, g0, gstep, grid_n)
                got = host(X)
                assert np.array_equal(got[:, :, :C + 2], want), (entry, C, ldx, grid_n, with_gt)
                assert not got[:, :, C + 2:].any() and np.isfinite(got).all(), (entry, C, ldx, grid_n)


@pytest.mark.parametrize("BTFC", [(2, 3, 1, 8), (1, 2, 3, 1024), (2, 2, 5, 16)], ids=["F1", "C1024", "F5"])
def test_serialize_sequential(cuda, BTFC):
    B, T, F, C = BTFC
    rng = np.random.default_rng(600 + C)
    feats = rng.standard_normal((B, T, F, C)).astype(np.float32)
    gts = rng.uniform(0, 1, size=(B, T, F)).astype(np.float32)
    S = F + (T - 1) * (2 * F + 1)
    tf_, tg = to_dev(feats, cuda), to_dev(gts[:, 0], cuda)
    for ldx in (C + 4, C + 8):
        for with_gt in (True, False):
            ref = O.serialize_sequential(feats, gts if with_gt else np.zeros_like(gts))
            X = nan_tensor((B, S, ldx), cuda)
            call("ntk_serialize_sequential", vptr(tf_), vptr(tg) if with_gt else None, vptr(X), B, T, F, C, ldx)
            got = host(X)
            assert np.array_equal(got[:, :, :C + 3], ref) and not got[:, :, C + 3:].any() and np.isfinite(got).all(), (BTFC, ldx, with_gt)


@pytest.mark.parametrize("BTDF", [(3, 4, 37, 9, 48), (2, 1, 5, 3, 9), (8, 17, 3900, 49, 4000)], ids=["odd_D", "T1", "grid_stride"])
def test_serialize_two_step(cuda, BTDF):
    B, T, D, F, ldx = BTDF
    if BTDF[2] == 3900:
        assert B * (2 * T - 1) * ldx > 4096 * 256                    # the grid-stride loop runs
    rng = np.random.default_rng(700 + D)
    feat = rng.standard_normal((B, T, D)).astype(np.float32)
    target = rng.uniform(0, 1, size=(B, F)).astype(np.float32)
    tf_, tt = to_dev(feat, cuda), to_dev(target, cuda)
    for with_target in (True, False):
        ref = O.two_step_inputs(feat, target if with_target else np.zeros_like(target))
        X = nan_tensor((B, 2 * T - 1, ldx), cuda)
        call("ntk_serialize_two_step", vptr(tf_), vptr(tt) if with_target else None, vptr(X), B, T, D, F, ldx)
        got = host(X)
        assert np.array_equal(got[:, :, :1 + D + F], ref) and not got[:, :, 1 + D + F:].any() and np.isfinite(got).all(), (BTDF, with_target)


# ---------------------------------------------------------------------------------------------------------
# optimiser
# ---------------------------------------------------------------------------------------------------------
def global_norm(cuda, g):
    from ntmtrack import _lib
    n = g.size
    nws = _lib.lib().ntk_global_norm_workspace_bytes(n) // 4
    assert nws == (n + 4095) // 4096
    ws, out = nan_tensor(nws + 16, cuda), nan_tensor(1 + 16, cuda)
    tg = to_dev(g, cuda)
    call("ntk_global_norm", vptr(tg), n, vptr(ws), vptr(out))
    assert still_guard(ws[nws:]) and still_guard(out[1:]) and bool(torch.isfinite(ws[:nws]).all())
    return float(host(out)[0])


GN_SIZES = [1, 255, 256, 257, 4095, 4096, 4097, 3 * 4096 + 5, 1024 * 4096 + 3]


@pytest.mark.parametrize("n", GN_SIZES)
def test_global_norm(cuda, n):
    """Bound: all terms are non-negative, so the relative error of the fp32 sum is at most depth * 2^-24 with depth the longest
    chain of roundings on the way to the sum.  From the code (csrc/optimizer.hip): sumsq_partial_kernel squares (1 rounding, none
    when fused), each thread adds its 4096 / 256 = 16 terms (16), wave_sum adds 4 + 3 times (7), thread 0 adds the 4 wave sums
    (4); sumsq_final_kernel: each of the 1024 threads adds ceil(nblocks / 1024) partials, wave_sum (7), thread 0 adds 16 wave
    sums (16): depth = 1 + 16 + 7 + 4 + ceil(nblocks / 1024) + 7 + 16 = 51 + ceil(nblocks / 1024).  The square root halves the
    relative error and adds one rounding; 1.001 covers the second-order terms."""
    rng = np.random.default_rng(800 + n % 997)
    g = rng.standard_normal(n).astype(np.float32)
    ref = float(np.sqrt(np.sum(g.astype(np.float64) ** 2)))
    nblocks = (n + 4095) // 4096
    depth = 51 + (nblocks + 1023) // 1024
    if n == GN_SIZES[-1]:
        assert nblocks == 1025 and depth == 53                        # the final kernel's threads take two partials
    bound = 1.001 * (depth / 2.0 + 1.0) * 2.0 ** -24
    got = global_norm(cuda, g)
    print("global_norm n=%d: relative error %.3e, bound %.3e (depth %d)" % (n, abs(got - ref) / ref, bound, depth))
    assert abs(got - ref) <= bound * ref


@pytest.mark.parametrize("n", [7, 257, 4097, 3 * 4096 + 5])
def test_global_norm_exact_on_a_perfect_square(cuda, n):
    """Integer entries whose squares sum to a perfect square below 2^24: every partial sum is an exact integer, so the only
    rounding is the square root's: within one ulp of the integer root."""
    g = np.zeros(n, np.float32)
    idx = np.random.default_rng(n).permutation(n)[:7]
    g[idx] = np.array([2, -3, 6, 24, -60, 156, -1092][:len(idx)], np.float32)    # roots 7, 25, 65, 169, 1105 as the entries are added
    ss = int(np.sum(g.astype(np.float64) ** 2))
    root = int(round(np.sqrt(ss)))
    assert root * root == ss and ss < 2 ** 24
    got = np.float32(global_norm(cuda, g))
    assert abs(float(got) - root) <= float(np.spacing(np.float32(root))), (float(got), root)


def f32(x):
    """The value the kernel receives for a hyper-parameter passed as a C float."""
    return float(np.float32(x))


HYPER = dict(lr=f32(1e-2), decay=f32(0.95), eps=f32(1e-10))      # fp32-representable: 1 - decay is then exact on the device too


def rmsprop_reference(dt, p, g_steps, ms, mom, momentum, clip, gnorms):
    p, ms, mom = p.astype(dt), ms.astype(dt), mom.astype(dt)
    for g, gn in zip(g_steps, gnorms):
        g = g.astype(dt)
        if clip > 0:
            g = g * (dt(clip) / np.maximum(dt(gn), dt(clip)))         # O.clip_by_global_norm's scale with the norm given
        p, ms, mom = O.rmsprop_step(p, g, ms, mom, lr=HYPER["lr"], decay=HYPER["decay"], momentum=momentum, eps=HYPER["eps"])
    return p, ms, mom


@pytest.mark.parametrize("clipmode", ["active", "inactive", "off"])
@pytest.mark.parametrize("momentum", [0.0, 0.9])
@pytest.mark.parametrize("n", [1, 255, 256, 257, 1000])
def test_rmsprop_two_consecutive_steps(cuda, n, momentum, clipmode):
    """Random positive ms, random mom, two steps with different gradients against O.rmsprop_step in float64 (clip scale as
    O.clip_by_global_norm's, from the norm word given)."""
    import ctypes
    f = ctypes.c_float
    momentum = f32(momentum)
    rng = np.random.default_rng(900 + n)
    p0 = rng.standard_normal(n).astype(np.float32)
    ms0 = rng.uniform(0.05, 2.0, n).astype(np.float32)
    mom0 = (rng.standard_normal(n) * 0.05).astype(np.float32)
    g_steps = [rng.standard_normal(n).astype(np.float32), (rng.standard_normal(n) * 2).astype(np.float32)]
    true_norms = [float(np.sqrt(np.sum(g.astype(np.float64) ** 2))) for g in g_steps]
    if clipmode == "active":
        clip = f32(0.5 * min(true_norms))
        scaled, gn0 = O.clip_by_global_norm([g_steps[0].astype(np.float64)], clip)      # the oracle's clip is the scale used below
        np.testing.assert_allclose(gn0, true_norms[0], rtol=1e-14)
        np.testing.assert_allclose(scaled[0], g_steps[0].astype(np.float64) * (clip / max(true_norms[0], clip)), rtol=1e-14)
    elif clipmode == "inactive":
        clip = f32(2.0 * max(true_norms))
    else:
        clip = 0.0
    norms32 = [np.float32(v) for v in true_norms]                      # the norm word the kernel reads
    ref = rmsprop_reference(np.float64, p0, g_steps, ms0, mom0, momentum, clip, norms32)
    r32 = rmsprop_reference(np.float32, p0, g_steps, ms0, mom0, momentum, clip, norms32)
    P, MS, MOM = to_dev(p0, cuda), to_dev(ms0, cuda), to_dev(mom0, cuda)
    for g, gn in zip(g_steps, norms32):
        gnorm = to_dev(np.array([gn]), cuda) if clipmode != "off" else None
        G = to_dev(g, cuda)
        call("ntk_rmsprop_clip_step", vptr(P), vptr(G), vptr(MS), vptr(MOM), n, f(HYPER["lr"]), f(HYPER["decay"]),
             f(momentum), f(HYPER["eps"]), f(clip), vptr(gnorm))
    name = "rmsprop n%d momentum%g clip_%s" % (n, momentum, clipmode)
    for what, got, want, w32 in zip(("param", "ms", "mom"), (P, MS, MOM), ref, r32):
        scale = max(1.0, float(np.max(np.abs(want))))
        assert gap(host(got), want) <= tol("%s %s" % (name, what), 1e-6 * scale, gap(w32, want)), (name, what)


@pytest.mark.parametrize("n", [1, 1000])
def test_rmsprop_checked_entry(cuda, n):
    import ctypes
    f = ctypes.c_float
    rng = np.random.default_rng(950 + n)
    p0, g = rng.standard_normal(n).astype(np.float32), rng.standard_normal(n).astype(np.float32)
    ms0, mom0 = rng.uniform(0.05, 2.0, n).astype(np.float32), (rng.standard_normal(n) * 0.05).astype(np.float32)
    hyper = (f(HYPER["lr"]), f(HYPER["decay"]), f(0.9), f(HYPER["eps"]), f(1.0))     # clip 1.0 < norm 3.0: the clip is active
    G = to_dev(g, cuda)

    def fresh():
        return to_dev(p0, cuda), to_dev(ms0, cuda), to_dev(mom0, cuda)

    # finite norm: the bits of the unchecked entry, `skipped` and `loss` untouched
    gnorm = to_dev(np.array([3.0]), cuda)
    P1, MS1, MOM1 = fresh()
    call("ntk_rmsprop_clip_step", vptr(P1), vptr(G), vptr(MS1), vptr(MOM1), n, *(hyper + (vptr(gnorm),)))
    P2, MS2, MOM2 = fresh()
    loss = to_dev(np.array([1.25]), cuda)
    skipped = torch.full((1,), 5, device=cuda, dtype=torch.int32)
    call("ntk_rmsprop_clip_step_checked", vptr(P2), vptr(G), vptr(MS2), vptr(MOM2), n, *(hyper + (vptr(gnorm), vptr(loss), vptr(skipped))))
    assert torch.equal(P1, P2) and torch.equal(MS1, MS2) and torch.equal(MOM1, MOM2)
    assert not torch.equal(P2, to_dev(p0, cuda))
    assert int(skipped.item()) == 5 and float(loss.item()) == 1.25
    P3, MS3, MOM3 = fresh()
    call("ntk_rmsprop_clip_step_checked", vptr(P3), vptr(G), vptr(MS3), vptr(MOM3), n, *(hyper + (vptr(gnorm), None, None)))
    assert torch.equal(P1, P3) and torch.equal(MS1, MS3) and torch.equal(MOM1, MOM3)
    # a NaN / +Inf norm word: nothing moves, the loss becomes NaN, exactly one skip is counted however many workgroups run
    for bad in (float("nan"), float("inf")):
        gbad = to_dev(np.array([bad]), cuda)
        P4, MS4, MOM4 = fresh()
        loss = to_dev(np.array([1.25]), cuda)
        skipped = torch.full((1,), 5, device=cuda, dtype=torch.int32)
        call("ntk_rmsprop_clip_step_checked", vptr(P4), vptr(G), vptr(MS4), vptr(MOM4), n, *(hyper + (vptr(gbad), vptr(loss), vptr(skipped))))
        for got, want in ((P4, p0), (MS4, ms0), (MOM4, mom0)):
            assert np.array_equal(host(got).view(np.uint32), want.view(np.uint32))
        assert np.isnan(float(loss.item())) and int(skipped.item()) == 6
        call("ntk_rmsprop_clip_step_checked", vptr(P4), vptr(G), vptr(MS4), vptr(MOM4), n, *(hyper + (vptr(gbad), None, None)))
        assert np.array_equal(host(P4).view(np.uint32), p0.view(np.uint32))


# ---------------------------------------------------------------------------------------------------------
# elementwise kernels
# ---------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("forget_bias", [0.0, 1.0])
@pytest.mark.parametrize("Bhid", [(1, 1), (3, 85), (1, 256), (1, 257)], ids=["n1", "n255", "n256", "n257"])
def test_lstm_step(cuda, Bhid, forget_bias):
    import ctypes
    B, hid = Bhid
    rng = np.random.default_rng(1000 + B * hid)
    pre = rng.standard_normal((B, 4 * hid)).astype(np.float32)
    c0 = rng.standard_normal((B, hid)).astype(np.float32)
    dh, dc = rng.standard_normal((B, hid)).astype(np.float32), rng.standard_normal((B, hid)).astype(np.float32)
    tp, tc0 = to_dev(pre, cuda), to_dev(c0, cuda)
    c, h, act = nan_tensor((B, hid), cuda), nan_tensor((B, hid), cuda), nan_tensor((B, 4 * hid), cuda)
    call("ntk_lstm_step_fwd", vptr(tp), vptr(tc0), ctypes.c_float(forget_bias), vptr(c), vptr(h), vptr(act), B, hid)
    cr, hr, ar, dpre_r, dc0_r = lstm_pointwise64(pre, c0, forget_bias, dh, dc)
    np.testing.assert_allclose(host(c), cr, atol=1e-6, rtol=0)
    np.testing.assert_allclose(host(h), hr, atol=1e-6, rtol=0)
    np.testing.assert_allclose(host(act), ar, atol=1e-6, rtol=0)
    c2, h2 = nan_tensor((B, hid), cuda), nan_tensor((B, hid), cuda)
    call("ntk_lstm_step_fwd", vptr(tp), vptr(tc0), ctypes.c_float(forget_bias), vptr(c2), vptr(h2), None, B, hid)   # act null
    assert torch.equal(c2, c) and torch.equal(h2, h)
    tdh, tdc = to_dev(dh, cuda), to_dev(dc, cuda)
    for use_dh, use_dc in ((True, True), (False, True), (True, False)):
        ref = lstm_pointwise64(pre, c0, forget_bias, dh if use_dh else None, dc if use_dc else None)
        dpre, dc0 = nan_tensor((B, 4 * hid), cuda), nan_tensor((B, hid), cuda)
        call("ntk_lstm_step_bwd", vptr(act), vptr(tc0), vptr(c), vptr(tdh) if use_dh else None, vptr(tdc) if use_dc else None,
             vptr(dpre), vptr(dc0), B, hid)
        np.testing.assert_allclose(host(dpre), ref[3], atol=2e-6, rtol=0)
        np.testing.assert_allclose(host(dc0), ref[4], atol=2e-6, rtol=0)


@pytest.mark.parametrize("act", [0, 1], ids=["tanh", "sigmoid"])
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_init_state_and_its_gradient(cuda, n, B, act):
    """out[b] = act(v); dv (+)= act'(v) sum_b dout[b].  Tolerances: outputs lie in [-1, 1] (base 1e-6); the gradient is a sum
    of B + 1 terms of size <= 4: base 1e-6 x that scale; widened only by 4 x the fp32-restatement gap if that is larger."""
    rng = np.random.default_rng(1100 + n + B)
    v = (rng.standard_normal(n) * 1.5).astype(np.float32)
    dout = rng.standard_normal((B, n)).astype(np.float32)
    dv0 = rng.standard_normal(n).astype(np.float32)

    def restated(dt):
        x = v.astype(dt)
        y = dt(1) / (dt(1) + np.exp(-x)) if act else np.tanh(x)
        dy = y * (dt(1) - y) if act else dt(1) - y * y
        return y, dout.astype(dt).sum(axis=0, dtype=dt) * dy

    y64, g64 = restated(np.float64)
    y32, g32 = restated(np.float32)
    tv, tdo = to_dev(v, cuda), to_dev(dout, cuda)
    out = nan_tensor((B + 1, n), cuda)
    call("ntk_ntm_init_state", vptr(tv), vptr(out), n, B, act)
    got = host(out)
    name = "init_state n%d B%d act%d" % (n, B, act)
    assert gap(got[:B], np.broadcast_to(y64, (B, n))) <= tol(name + " out", 1e-6, gap(y32, y64))
    assert still_guard(out[B])                                         # the row behind the batch is untouched
    for accumulate in (0, 1):
        dv = to_dev(dv0, cuda) if accumulate else nan_tensor(n, cuda)
        call("ntk_ntm_init_state_bwd", vptr(tv), vptr(tdo), vptr(dv), n, B, act, accumulate)
        want = g64 + (dv0.astype(np.float64) if accumulate else 0.0)
        w32 = g32 + (dv0 if accumulate else np.float32(0))
        scale = max(1.0, float(np.max(np.abs(want))))
        assert gap(host(dv), want) <= tol("%s dv acc%d" % (name, accumulate), 1e-6 * scale, gap(w32, want)), (name, accumulate)


@pytest.mark.parametrize("rows", [1, 31, 32, 33, 70])
def test_transpose_pad(cuda, rows):
    rng = np.random.default_rng(1200 + rows)
    for cols in (1, 31, 32, 33, 70):
        for ldi in (cols, cols + 5):
            src = rng.standard_normal((rows, ldi)).astype(np.float32)
            tin = to_dev(src, cuda)
            for ldo in (rows, rows + 3, rows + 40):                   # + 40: a whole tile that lies in the padding
                out = nan_tensor((cols + 1, ldo), cuda)
                call("ntk_transpose_pad", vptr(tin), ldi, vptr(out), ldo, rows, cols)
                got = host(out)
                assert np.array_equal(got[:cols, :rows], src[:, :cols].T), (rows, cols, ldi, ldo)
                assert not got[:cols, rows:].any() and np.isfinite(got[:cols]).all(), (rows, cols, ldi, ldo)
                assert still_guard(out[cols]), (rows, cols, ldi, ldo)


@pytest.mark.parametrize("shape", [(1, 2, 2, 4), (2, 6, 10, 8), (3, 4, 6, 12)], ids=["smallest", "modules_case", "C12"])
def test_maxpool2x2(cuda, shape):
    rng = np.random.default_rng(1300 + shape[3])
    n, H, W, C = shape
    for negative in (False, True):
        x = rng.standard_normal(shape).astype(np.float32)
        if negative:
            x = -np.abs(x) - 1.0                                      # a max that started from 0 would show
        out = nan_tensor((n + 1, H // 2, W // 2, C), cuda)
        tx = to_dev(x, cuda)
        call("ntk_maxpool2x2", vptr(tx), vptr(out), n, H, W, C)
        got = host(out)
        assert np.array_equal(got[:n], O.maxpool2x2(x)) and still_guard(out[n]), (shape, negative)


def test_maxpool2x2_grid_stride(cuda):
    """More 4-channel groups than 16384 workgroups x 256 threads: the grid-stride loop runs (about 270 MB in, generated on the
    device; the oracle runs on the host copy)."""
    n, H, W, C = 1, 1026, 1026, 64
    assert n * (H // 2) * (W // 2) * (C // 4) > 16384 * 256
    gen = torch.Generator(device=cuda).manual_seed(14)
    x = torch.randn((n, H, W, C), device=cuda, generator=gen)
    out = nan_tensor((n, H // 2, W // 2, C), cuda)
    call("ntk_maxpool2x2", vptr(x), vptr(out), n, H, W, C)
    assert np.array_equal(host(out), O.maxpool2x2(host(x)))
