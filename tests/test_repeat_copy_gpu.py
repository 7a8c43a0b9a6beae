"""GPU: the repeat-copy task (ntmtrack.repeat_copy) -- the pack kernel against the concatenation restatement, the masked sigmoid
cross entropy against its float64 restatement, loss and gradients of a training step against the autograd oracles of both cores,
and end to end: the DNC core LEARNS the task (forward, BPTT, clip and RMSProp), and a checkpoint resumes the same run."""
import ctypes

import numpy as np
import pytest
import torch

import repeat_copy_util as U
from small_kernel_util import INPUT_NAN, FlatGuarded, raw_bytes_equal

pytestmark = pytest.mark.gpu


def _lib():
    from ntmtrack import _lib as lib
    return lib


# --------------------------------------------------------------------------------------------------------------------- pack
def _pack(cuda, bits, lengths, repeats, ranges, nb, ldx, S, norm_max=10):
    """ntk_repeat_copy_pack straight through the C ABI into NaN-guarded outputs; the pattern rows past a sequence's length hold
    NaN (they may not be read).  -> (X, target, mask) on the host, after the checks of FlatGuarded.written()."""
    lib = _lib()
    B, ML = bits.shape[0], bits.shape[1]
    lo_l, hi_l, lo_r, hi_r = ranges
    held = bits.copy()
    for b, L in enumerate(U.clamp_table(lengths, lo_l, hi_l)):
        held[b, L:] = np.nan
    gb = FlatGuarded((B, ML, nb), cuda, init=held)
    table = torch.tensor([list(lengths), list(repeats)], dtype=torch.int32).to(cuda)
    X, T, M = FlatGuarded((B, S, ldx), cuda), FlatGuarded((B, S, nb + 1), cuda), FlatGuarded((B, S), cuda)
    ip = lambda t: ctypes.c_void_p(t.data_ptr())
    lib.check(lib.lib().ntk_repeat_copy_pack(gb.ptr, ip(table[0]), ip(table[1]), X.ptr, T.ptr, M.ptr, B, S, nb, ldx, lo_l, hi_l, lo_r,
                                             hi_r, float(norm_max), lib.stream()), "ntk_repeat_copy_pack")
    torch.cuda.synchronize()
    return X.written(), T.written(), M.written()


BATCHES = {"one": ((1,), (1,), (1, 1, 1, 1)), "three": ((1, 4, 2), (1, 1, 3), (1, 4, 1, 3))}


@pytest.mark.parametrize("extra", [0, 8])
@pytest.mark.parametrize("nb", [1, 4, 15])
@pytest.mark.parametrize("batch", sorted(BATCHES))
def test_pack_equals_the_concatenation_restatement(cuda, batch, nb, extra):
    lengths, repeats, ranges = BATCHES[batch]
    B, ML = len(lengths), ranges[1]
    bits = np.random.default_rng(nb + extra).integers(0, 2, (B, ML, nb)).astype(np.float32)
    ldx = (nb + 2 + 3) // 4 * 4 + extra
    S = max(L * (r + 1) + 3 for L, r in zip(lengths, repeats))
    assert S == (5 if batch == "one" else 11)
    want = U.layout(bits, lengths, repeats, S=S, ldx=ldx)
    got = _pack(cuda, bits, lengths, repeats, ranges, nb, ldx, S)
    for g, w, name in zip(got, want, ("X", "target", "mask")):
        assert raw_bytes_equal(g, w), name


def test_pack_pads_to_a_step_count_beyond_the_longest_sequence(cuda):
    lengths, repeats, ranges = BATCHES["three"]
    bits = np.random.default_rng(5).integers(0, 2, (3, 4, 4)).astype(np.float32)
    want = U.layout(bits, lengths, repeats, S=17, ldx=8)
    got = _pack(cuda, bits, lengths, repeats, ranges, 4, 8, 17)
    assert all(raw_bytes_equal(g, w) for g, w in zip(got, want))
    assert not got[0][:, 11:].any() and not got[1][:, 11:].any() and not got[2][:, 11:].any()


def test_pack_clamps_lengths_and_repeats_outside_their_ranges(cuda):
    """A bad table cannot index past the bits or the outputs: the result is the layout of the clamped table, guards intact."""
    ranges = (2, 3, 1, 2)
    lengths, repeats = (-5, 100, 3, 0), (7, -1, 2, 1 << 30)
    bits = np.random.default_rng(6).integers(0, 2, (4, 3, 4)).astype(np.float32)
    cl, cr = U.clamp_table(lengths, 2, 3), U.clamp_table(repeats, 1, 2)
    assert (cl, cr) == ([2, 3, 3, 2], [2, 1, 2, 2])
    S = 12                                                                   # 3 (2 + 1) + 3, the longest the ranges allow
    want = U.layout(bits, cl, cr, S=S, ldx=8)
    got = _pack(cuda, bits, lengths, repeats, ranges, 4, 8, S)
    assert all(raw_bytes_equal(g, w) for g, w in zip(got, want))


def test_dataset_call_is_one_batch_of_the_reference_shapes_and_reproducible(cuda):
    from ntmtrack.repeat_copy import RepeatCopy
    mk = lambda: RepeatCopy(num_bits=4, batch_size=16, min_length=1, max_length=2, min_repeats=1, max_repeats=2, device=cuda, seed=9)
    a, b = mk(), mk()
    for _ in range(3):
        da, db = a(), b()
        S = int((da.lengths * (da.repeats + 1) + 3).max())
        assert tuple(da.observations.shape) == (S, 16, 6) and tuple(da.target.shape) == (S, 16, 5) and tuple(da.mask.shape) == (S, 16)
        assert tuple(da.X.shape) == (16, S, 8) and da.observations.data_ptr() == da.X.data_ptr()      # views, not copies
        assert torch.equal(da.X, db.X) and torch.equal(da.target_bm, db.target_bm) and torch.equal(da.mask_bm, db.mask_bm)
        # the layout of the restatement, from the pattern the observations themselves carry
        X = da.X.cpu().numpy()
        bits = np.zeros((16, 2, 4), np.float32)
        for i, L in enumerate(da.lengths.tolist()):
            bits[i, :L] = X[i, 1:1 + L, :4]
        want = U.layout(bits, da.lengths.tolist(), da.repeats.tolist(), S=S, ldx=8)
        assert raw_bytes_equal(X, want[0]) and raw_bytes_equal(da.target_bm.cpu().numpy(), want[1])
        assert raw_bytes_equal(da.mask_bm.cpu().numpy(), want[2])
        assert set(np.unique(X[:, :, :4])) <= {0.0, 1.0}


# --------------------------------------------------------------------------------------------------------------------- loss
def _xent(cuda, x, z, m, ta, bits, want_grad=True):
    """ntk_masked_sigmoid_xent through the C ABI, guarded operands and outputs -> (loss, loss_batch, dlogits or None, score)."""
    lib = _lib()
    B, S, O = x.shape
    gx, gz, gm = FlatGuarded((B, S, O), cuda, init=x), FlatGuarded((B, S, O), cuda, init=z), FlatGuarded((B, S), cuda, init=m)
    loss, lb = FlatGuarded(1, cuda, pad=4), FlatGuarded(B, cuda, pad=4)
    d = FlatGuarded((B, S, O), cuda) if want_grad else None
    score = torch.full((B, 2), -7, device=cuda, dtype=torch.int32)
    lib.check(lib.lib().ntk_masked_sigmoid_xent(gx.ptr, gz.ptr, gm.ptr, loss.ptr, lb.ptr, d.ptr if d else None,
                                                ctypes.c_void_p(score.data_ptr()), B, S, O, int(ta), int(bits), lib.stream()),
              "ntk_masked_sigmoid_xent")
    torch.cuda.synchronize()
    assert loss.guards_intact() and lb.guards_intact() and (d is None or d.guards_intact())
    return loss.numpy()[0], lb.numpy(), (d.numpy() if d else None), score.cpu().numpy()


def _check_xent(cuda, x, z, m, ta, bits, label):
    """The bound of test_small_kernels_gpu.py: max(base, 4 x gap(float32 restatement, float64)); base 1e-5 relative for the loss,
    1e-6 absolute for dlogits (what ntk_log_loss is held to there)."""
    l64, lb64, d64, s64 = U.cost(x, z, m, ta, bits, np.float64)
    l32, lb32, d32, _ = U.cost(x, z, m, ta, bits, np.float32)
    loss, lb, d, score = _xent(cuda, x, z, m, ta, bits)
    err_l, bound_l = abs(float(loss) - l64), max(1e-5 * abs(l64), 4 * abs(float(l32) - l64))
    err_b = np.abs(lb.astype(np.float64) - lb64)
    bound_b = np.maximum(1e-5 * np.abs(lb64), 4 * np.abs(lb32.astype(np.float64) - lb64))
    err_d, bound_d = float(np.max(np.abs(d.astype(np.float64) - d64))), max(1e-6, 4 * float(np.max(np.abs(d32.astype(np.float64) - d64))))
    print("%s ta=%d bits=%d: loss %.7g err %.2e (bound %.2e), dlogits err %.2e (bound %.2e)" % (label, ta, bits, loss, err_l, bound_l, err_d, bound_d))
    assert np.isfinite(loss) and np.isfinite(d).all()
    assert err_l <= bound_l and (err_b <= bound_b).all() and err_d <= bound_d
    assert np.array_equal(score, s64)
    off = np.broadcast_to((m == 0)[:, :, None], d.shape)
    assert raw_bytes_equal(d[off], np.zeros(int(off.sum()), np.float32))      # +0.0, bit for bit
    return loss, lb, d, score


#: per-sequence element counts S * O at the edges of the kernel's loop (a wave, a workgroup's stride of 256, several strides)
SHAPES = {1: (1, 1), 63: (9, 7), 64: (16, 4), 65: (13, 5), 1025: (205, 5), 5000: (625, 8)}


@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n", sorted(SHAPES))
def test_xent_against_the_float64_restatement(cuda, n, B):
    S, O = SHAPES[n]
    rng = np.random.default_rng(n + B)
    x = (rng.standard_normal((B, S, O)) * 3).astype(np.float32)
    z = rng.integers(0, 2, (B, S, O)).astype(np.float32)
    m = (rng.random((B, S)) < 0.6).astype(np.float32)
    m[:, 0] = 1.0                                                             # every sequence scores something
    for ta in (0, 1):
        for bits in (0, 1):
            loss, lb, d, score = _check_xent(cuda, x, z, m, ta, bits, "n=%d B=%d" % (n, B))
            # loss only (null dlogits): the same loss bits; and a second run: the same bits throughout
            loss0, lb0, _, score0 = _xent(cuda, x, z, m, ta, bits, want_grad=False)
            assert raw_bytes_equal(loss0, loss) and raw_bytes_equal(lb0, lb) and np.array_equal(score0, score)
            loss2, lb2, d2, score2 = _xent(cuda, x, z, m, ta, bits)
            assert raw_bytes_equal(loss2, loss) and raw_bytes_equal(lb2, lb) and raw_bytes_equal(d2, d) and np.array_equal(score2, score)


def test_xent_is_finite_at_large_logits(cuda):
    """log(1 + exp(100)) overflows float32 when taken at its word; the stable form does not."""
    x = np.array([[[100.0, 100.0, -100.0, -100.0], [88.0, -88.0, 30.0, -30.0]]], np.float32)
    z = np.array([[[0.0, 1.0, 0.0, 1.0], [0.0, 1.0, 1.0, 0.0]]], np.float32)
    m = np.ones((1, 2), np.float32)
    for ta in (0, 1):
        loss, _, d, score = _check_xent(cuda, x, z, m, ta, 0, "large logits")
        assert 100.0 < loss < 400.0
        assert score.tolist() == [[8, 4]]


def test_xent_of_a_sequence_without_scored_steps_is_zero(cuda):
    rng = np.random.default_rng(3)
    x = rng.standard_normal((2, 6, 5)).astype(np.float32)
    z = rng.integers(0, 2, (2, 6, 5)).astype(np.float32)
    m = np.zeros((2, 6), np.float32)
    m[1, 2:5] = 1.0
    loss, lb, d, score = _check_xent(cuda, x, z, m, 1, 0, "empty mask")
    assert raw_bytes_equal(lb[:1], np.zeros(1, np.float32)) and raw_bytes_equal(d[0], np.zeros((6, 5), np.float32))
    assert score.tolist()[0] == [0, 0] and score[1, 0] == 15
    x0, z0, m0 = x[:1], z[:1], m[:1]                                          # the whole batch empty
    loss, lb, d, score = _check_xent(cuda, x0, z0, m0, 1, 1, "all empty")
    assert raw_bytes_equal(loss, np.float32(0.0)) and raw_bytes_equal(d, np.zeros_like(d))


def test_xent_selects_masked_steps_out_whatever_they_hold(cuda):
    rng = np.random.default_rng(4)
    x = (rng.standard_normal((3, 11, 5)) * 2).astype(np.float32)
    z = rng.integers(0, 2, (3, 11, 5)).astype(np.float32)
    m = (rng.random((3, 11)) < 0.5).astype(np.float32)
    m[:, 1] = 1.0; m[:, 2] = 0.0
    clean = _check_xent(cuda, x, z, m, 1, 1, "clean")
    xn = x.copy()
    xn[m == 0] = np.nan
    dirty = _check_xent(cuda, xn, z, m, 1, 1, "NaN at masked steps")
    assert all(raw_bytes_equal(a, b) for a, b in zip(clean, dirty))


def test_module_cost_takes_the_references_time_major_tensors(cuda):
    from ntmtrack.repeat_copy import RepeatCopy, masked_xent
    ds = RepeatCopy(num_bits=4, batch_size=3, max_length=2, device=cuda, time_average_cost=True, log_prob_in_bits=True)
    data = ds.from_arrays(np.random.default_rng(8).integers(0, 2, (3, 2, 4)), (1, 2, 2), (2, 1, 2))
    logits = torch.randn(data.target_bm.shape, device=cuda, generator=torch.Generator(device=cuda).manual_seed(1))
    loss, lb, d, score = masked_xent(logits, data.target_bm, data.mask_bm, True, True)
    l64, lb64, d64, s64 = U.cost(logits.cpu().numpy(), data.target_bm.cpu().numpy(), data.mask_bm.cpu().numpy(), True, True)
    got = ds.cost(logits.transpose(0, 1), data.target, data.mask)
    assert got.dim() == 0 and float(got) == float(loss[0]) and abs(float(got) - l64) <= 1e-5 * l64
    assert np.array_equal(score.cpu().numpy(), s64) and np.max(np.abs(d.cpu().numpy() - d64)) <= 1e-6


# --------------------------------------------------------------------------------------------------------------------- task
TASK_BITS = np.random.default_rng(21).integers(0, 2, (3, 2, 4)).astype(np.float32)
TASK_LENGTHS, TASK_REPEATS = (1, 2, 2), (2, 1, 2)


def _task_batch(cuda, time_average=False):
    from ntmtrack.repeat_copy import RepeatCopy
    ds = RepeatCopy(num_bits=4, batch_size=3, min_length=1, max_length=2, min_repeats=1, max_repeats=2, device=cuda,
                    time_average_cost=time_average)
    data = ds.from_arrays(TASK_BITS, TASK_LENGTHS, TASK_REPEATS)
    want = U.layout(TASK_BITS, TASK_LENGTHS, TASK_REPEATS, ldx=8)
    assert raw_bytes_equal(data.X.cpu().numpy(), want[0])
    return ds, data, want


@pytest.mark.parametrize("name,ta,R,W", [("default", False, 1, 16), ("time_average", True, 1, 16), ("two_reads_word6", False, 2, 6)])
def test_dnc_task_loss_and_gradients_match_the_autograd_oracle(cuda, name, ta, R, W):
    """Rule of test_dnc_gpu.py: relative error at most max(1e-4, 3 x the float32 oracle's own error), for the loss and per tensor."""
    from oracle import dnc_oracle as D
    from oracle import dnc_oracle_torch as DT
    from dnc_util import conditioned_params, gradient_errors
    from ntmtrack.repeat_copy import RepeatCopyTask
    ds, data, (X, target, mask) = _task_batch(cuda, ta)
    cfg = D.DNCConfig(6, 5, memory_size=16, word_size=W, num_reads=R, num_writes=1, hidden_size=64, clip_value=20.0)
    p = conditioned_params(cfg, np.random.default_rng(31), 4)
    task = RepeatCopyTask(ds, "dnc", memory_size=16, word_size=W, num_reads=R, num_writes=1, hidden_size=64, clip_value=20)
    task.core.load_state_dict({k: torch.from_numpy(v) for k, v in p.items()})
    task.core.poison_records = True
    res = {}
    for dtype in (torch.float64, torch.float32):
        t = lambda v: torch.tensor(np.asarray(v), dtype=dtype)
        pt = {k: t(v).requires_grad_(True) for k, v in p.items()}
        ys, _ = DT.run_model(cfg, pt, t(np.swapaxes(X[:, :, :6], 0, 1)))
        loss = U.cost_torch(ys.transpose(0, 1), t(target), t(mask), ta, False)
        loss.backward()
        res[dtype] = (float(loss.detach()), {k: v.grad.double().numpy() for k, v in pt.items()}, ys.detach().transpose(0, 1).double().numpy())
    (l64, g64, y64), (l32, g32, _) = res[torch.float64], res[torch.float32]
    loss, logits = task.loss_and_grads(data)
    got = {k: v.cpu().numpy() for k, v in task.core._unpack(grad=True).items()}
    torch.cuda.synchronize()
    assert task.core.last_cluster_k == 1 and task.core.last_cluster_bwd_k == 1     # a 16-slot memory: one workgroup per sequence
    np.testing.assert_allclose(logits.cpu().numpy(), y64, atol=5e-5)
    err, err32 = abs(float(loss.cpu()) - l64) / abs(l64), abs(l32 - l64) / abs(l64)
    worst, bad = gradient_errors(got, g64, g32)
    print("%s: loss %.6f (float64 %.6f) rel err %.1e (float32 oracle %.1e); gradients %s"
          % (name, float(loss.cpu()), l64, err, err32, {k: ("%.1e" % a, "%.1e" % b) for k, (a, b, _) in worst.items()}))
    assert err <= max(1e-4, 3 * err32)
    assert not bad, bad


def test_ntm_task_loss_and_gradients_match_the_autograd_oracle(cuda):
    """The bound of test_copy_task_gpu.py: 3e-3 relative per tensor.  The same batch as the DNC cases; the memory has 64 slots, the
    fewest the NTM sequence kernels take (a 16-slot memory is refused at construction)."""
    from oracle import ntm_oracle as O
    from oracle import ntm_oracle_torch as OT
    from ntmtrack import _lib
    from ntmtrack.repeat_copy import RepeatCopyTask
    ds, data, (X, target, mask) = _task_batch(cuda)
    with pytest.raises(_lib.NtkError, match="mem_size=16"):
        RepeatCopyTask(ds, "ntm", memory_size=16)
    task = RepeatCopyTask(ds, "ntm", memory_size=64, word_size=16, num_reads=1, num_writes=1, hidden_size=64, seed=2)
    sd = {k: v.numpy() for k, v in task.cell.state_dict().items()}
    cfg = O.NTMConfig(6, 5, mem_size=64, mem_dim=16, shift_range=1, controller_hidden_size=64, controller_num_layers=1,
                      write_head_size=1, read_head_size=1)
    pt = {k: torch.tensor(v, dtype=torch.float64, requires_grad=True) for k, v in sd.items()}
    t64 = lambda v: torch.tensor(v, dtype=torch.float64)
    ref_logits, _ = OT.loop(cfg, pt, t64(X[:, :, :6]))
    loss_ref = U.cost_torch(ref_logits, t64(target), t64(mask))
    loss_ref.backward()
    loss, logits = task.loss_and_grads(data)
    torch.cuda.synchronize()
    np.testing.assert_allclose(logits.cpu().numpy(), ref_logits.detach().numpy(), atol=2e-5)
    np.testing.assert_allclose(float(loss.cpu()), float(loss_ref.detach()), rtol=1e-5)
    got = task.cell.params.to_tf(grad=True)
    for k in sorted(sd):
        ref = pt[k].grad.numpy()
        err = np.max(np.abs(got[k].numpy() - ref)) / (np.max(np.abs(ref)) + 1e-30)
        assert err < 3e-3, (k, err)


STEPS, LEARNING_RATE = 300, 3e-3


def test_dnc_learns_repeat_copy(cuda):
    """train.py's task (bits 4, length 1-2, repeats 1-2, B = 16) at a raised learning rate, as test_copy_task_learns raises it: the
    mean of the last 10 losses is below 0.75 of the mean of the first 10 (the ratio the NTM copy test is held to), every loss is
    finite, and the trained task copies with a lower bit error rate than the untrained one."""
    from ntmtrack.repeat_copy import RepeatCopy, RepeatCopyTask
    mk = lambda seed: RepeatCopy(num_bits=4, batch_size=16, min_length=1, max_length=2, min_repeats=1, max_repeats=2, device=cuda, seed=seed)
    task = RepeatCopyTask(mk(5), "dnc", learning_rate=LEARNING_RATE, seed=3)
    _l0, ber0, _p0 = task.eval(4, mk(77))
    losses = [task.train_step() for _ in range(STEPS)]
    task.check_step()
    vals = torch.cat(losses).cpu().numpy()
    l1, ber1, perfect1 = task.eval(4, mk(77))                                  # the same four batches as before training
    first, last = float(np.mean(vals[:10])), float(np.mean(vals[-10:]))
    print("repeat copy, DNC, %d steps at lr %g: first 10 %.4f, last 10 %.4f, ratio %.3f; bit error rate %.4f -> %.4f, perfect copies %.3f"
          % (STEPS, LEARNING_RATE, first, last, last / first, ber0, ber1, perfect1))
    print("mean loss of every 25 steps: %s" % " ".join("%.3f" % v for v in vals.reshape(-1, 25).mean(1)))
    assert np.isfinite(vals).all()
    assert last < 0.75 * first, (first, last)
    assert ber1 < ber0, (ber0, ber1)
    assert task.opt.global_step == STEPS


def test_train_loop_reports_and_writes_checkpoints(cuda, tmp_path):
    from ntmtrack.repeat_copy import RepeatCopy, RepeatCopyTask, train
    ds = RepeatCopy(num_bits=4, batch_size=4, max_length=2, device=cuda, seed=1)
    task = RepeatCopyTask(ds, "dnc", seed=1)
    lines = []
    path = str(tmp_path / "rc.ckpt")
    reports = train(task, 6, 3, log=lines.append, checkpoint_path=path, checkpoint_interval=4)
    assert len(reports) == 2 and len(lines) == 2 and all(np.isfinite(reports))
    assert lines[0].startswith("2: Avg training loss %f.\n\nObservations:\n+" % reports[0]) and "Model Output:\n+" in lines[1]
    other = RepeatCopyTask(RepeatCopy(num_bits=4, batch_size=4, max_length=2, device=cuda, seed=1), "dnc", seed=9)
    assert other.load_checkpoint(path) == 4
    assert train(task, 6, 3, log=lines.append) == []                          # nothing left to do: the loop starts at the global step


def test_checkpoint_resumes_the_same_run(cuda, tmp_path):
    """Train 6 steps; then 3, save, 3 more; a fresh task that loads the checkpoint and trains 3 ends with the same parameters, bit
    for bit (on the NTM core, whose kernels sum in a fixed order: the DNC BPTT's LDS atomics do not, tests/test_dnc_gpu.py), having
    drawn the same batches (both generators' states travel in the checkpoint).  On the DNC core what is reproducible to the bit
    is checked: parameters, slots and step as saved, and the batch stream."""
    from ntmtrack.repeat_copy import RepeatCopy, RepeatCopyTask
    mk_ds = lambda: RepeatCopy(num_bits=4, batch_size=8, min_length=1, max_length=2, min_repeats=1, max_repeats=2, device=cuda, seed=4)
    for core in ("ntm", "dnc"):
        mem = dict(memory_size=64) if core == "ntm" else {}                    # the NTM kernels take no fewer than 64 slots
        task = RepeatCopyTask(mk_ds(), core, learning_rate=1e-3, seed=6, **mem)
        for _ in range(6 + 3):
            task.train_step()
        path = task.save_checkpoint(str(tmp_path / ("%s.ckpt" % core)))
        saved = [t.clone() for t in (task.params.flat, task.opt.ms, task.opt.mom)]
        batches = []
        for _ in range(3):
            task.train_step()
            batches.append(task.last_data)
        fresh = RepeatCopyTask(mk_ds(), core, learning_rate=1e-3, seed=99, **mem)     # other initial parameters, generators at their start
        assert not torch.equal(fresh.params.flat, task.params.flat)
        assert fresh.load_checkpoint(path) == 9 and fresh.opt.global_step == 9
        assert all(torch.equal(a, b) for a, b in zip(saved, (fresh.params.flat, fresh.opt.ms, fresh.opt.mom)))
        for k in range(3):
            fresh.train_step()
            assert torch.equal(fresh.last_data.X, batches[k].X) and torch.equal(fresh.last_data.target_bm, batches[k].target_bm)
        torch.cuda.synchronize()
        if core == "ntm":
            assert torch.equal(fresh.params.flat, task.params.flat) and torch.equal(fresh.opt.ms, task.opt.ms)
        else:
            scale = float(task.params.flat.abs().max())
            assert float((fresh.params.flat - task.params.flat).abs().max()) <= 1e-5 * scale
