"""Repeat-copy task of the vendored DNC (dnc/repeat_copy.py, dnc/train.py) on the HIP path: the one runnable demonstration the
reference's DNC ships, and the DNC-side counterpart of copy_task.py -- forward, BPTT, clip and RMSProp shown to LEARN a task, with no
VGG in the way.

A batch is laid out on the device, in ONE launch (ntk_repeat_copy_pack), directly in the layout the sequence kernels read:
observations X [B, S, ldx] batch-major with zero padding columns, target [B, S, num_bits + 1], mask [B, S].  The reference's
time-major tensors ([S, B, .]) are views of those.  Loss, gradient and copy score come from one pass of ntk_masked_sigmoid_xent;
nothing is read back per step.

Layout of a sequence with pattern length L and r repeats (repeat_copy.py:252-377): step 0 carries the start flag, steps 1..L the
pattern, step L + 1 the repeat count r / norm_max; the target holds the pattern r times on rows L + 2 .. L + 1 + L r and the end
marker on row L + 2 + L r; the mask is one on rows L + 2 .. L + 2 + L r.  S is the batch's longest own length L (r + 1) + 3.

One departure from the reference: a step whose mask is 0 is selected out of loss and gradient, not multiplied out (it adds exactly
0 whatever the logits there hold).  The sequence kernels run every sequence to S; what they emit after a sequence's own end is not
part of the task.  Not claimed: bit parity with TensorFlow's random streams, or any accuracy figure of the reference.
"""
import collections
import ctypes

import numpy as np
import torch

from . import _lib
from .ntm import gemm_nt

_P = _lib.ptr


def _iptr(t):
    """Device pointer of a contiguous int32 tensor (or None)."""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


class DatasetTensors(collections.namedtuple("DatasetTensors", ("observations", "target", "mask"))):
    """The reference's tuple: time-major observations [S, B, num_bits + 2], target [S, B, num_bits + 1], mask [S, B].  On a batch made
    by RepeatCopy these are views of the batch-major device buffers, reachable as attributes: ``X`` [B, S, ldx] (what the kernels
    read, padding columns zero), ``target_bm`` [B, S, num_bits + 1], ``mask_bm`` [B, S], and the host tables ``lengths`` /
    ``repeats`` (after clamping to the dataset's ranges).  A tuple built by hand, or by _replace, has them as None."""
    X = None
    target_bm = None
    mask_bm = None
    lengths = None
    repeats = None


def masked_xent(logits, target, mask, time_average=False, log_prob_in_bits=False, want_grad=True, want_score=True):
    """ntk_masked_sigmoid_xent on BATCH-major device tensors: logits, target [B, S, O], mask [B, S] ->
    (loss [1], loss_batch [B], dlogits [B, S, O] or None, score [B, 2] int32 or None)."""
    B, S, O = logits.shape
    if tuple(target.shape) != (B, S, O) or tuple(mask.shape) != (B, S):
        raise _lib.NtkError("masked_xent: logits %s, target %s, mask %s" % (tuple(logits.shape), tuple(target.shape), tuple(mask.shape)))
    dev = logits.device
    loss, loss_batch = torch.empty(1, device=dev), torch.empty(B, device=dev)
    dlogits = torch.empty((B, S, O), device=dev) if want_grad else None
    score = torch.empty((B, 2), device=dev, dtype=torch.int32) if want_score else None
    _lib.check(_lib.lib().ntk_masked_sigmoid_xent(_P(logits.contiguous()), _P(target.contiguous()), _P(mask.contiguous()), _P(loss),
                                                  _P(loss_batch), _P(dlogits), _iptr(score), B, S, O, 1 if time_average else 0,
                                                  1 if log_prob_in_bits else 0, _lib.stream()), "ntk_masked_sigmoid_xent")
    return loss, loss_batch, dlogits, score


def masked_sigmoid_cross_entropy(logits, target, mask, time_average=False, log_prob_in_bits=False):
    """repeat_copy.py:29-66 with the reference's TIME-major arguments (logits, target [S, B, O], mask [S, B]) -> the scalar loss (a
    0-dim device tensor).  Views of batch-major buffers (what this module hands out) are not copied."""
    bm = lambda t: t.transpose(0, 1).contiguous()
    return masked_xent(bm(logits), bm(target), bm(mask), time_average, log_prob_in_bits, want_grad=False, want_score=False)[0][0]


def _host(a):
    return a.detach().cpu().numpy() if torch.is_tensor(a) else np.asarray(a)


def bitstring_readable(data, batch_size, model_output=None, whole_batch=False):
    """The reference's text picture of a batch (repeat_copy.py:69-112): per sequence an "Observations:" block, a "Targets:" block and,
    with model_output [S, B, num_bits + 1], a "Model Output:" block; one line per channel, '+' at both ends, the steps separated by
    blanks, '-' for a zero and the integer value otherwise.  Only the first sequence unless whole_batch."""
    obs, targ = _host(data.observations), _host(data.target)
    out = None if model_output is None else _host(model_output)

    def line(values):
        return "+" + " ".join("-" if v == 0 else "%d" % v for v in values) + "+"

    def block(title, seq, channels):
        return title + ":\n" + "\n".join(line(seq[:, c]) for c in range(channels))

    texts = []
    for b in range(batch_size if whole_batch else 1):
        parts = [block("Observations", obs[:, b], obs.shape[2]), block("Targets", targ[:, b], targ.shape[2])]
        if out is not None:
            parts.append(block("Model Output", out[:, b], targ.shape[2]))
        texts.append("\n\n".join(parts))
    return "\n" + "\n\n\n\n".join(texts)


class RepeatCopy(object):
    """Generator of repeat-copy batches (repeat_copy.py:115-392) with the reference's constructor arguments and properties.
    Calling it returns the next batch as DatasetTensors: pattern lengths and repeat counts are sampled on the HOST from a seeded
    generator (so the padded step count S is known without waiting for the device), the pattern bits on the device from a seeded
    torch.Generator, then one pack launch.  ``from_arrays`` lays out given patterns (tests, evaluation sets)."""

    def __init__(self, num_bits=6, batch_size=1, min_length=1, max_length=1, min_repeats=1, max_repeats=2, norm_max=10,
                 log_prob_in_bits=False, time_average_cost=False, device="cuda", seed=0, name="repeat_copy"):
        ints = dict(num_bits=num_bits, batch_size=batch_size, min_length=min_length, max_length=max_length,
                    min_repeats=min_repeats, max_repeats=max_repeats)
        for k, v in ints.items():
            if int(v) != v:
                raise _lib.NtkError("RepeatCopy: %s=%r is not an integer" % (k, v))
        if num_bits < 1 or batch_size < 1:
            raise _lib.NtkError("RepeatCopy: num_bits=%d batch_size=%d (both >= 1)" % (num_bits, batch_size))
        if min_length < 1 or min_length > max_length:
            raise _lib.NtkError("RepeatCopy: length range [%d, %d] (1 <= min <= max)" % (min_length, max_length))
        if min_repeats < 0 or min_repeats > max_repeats:
            raise _lib.NtkError("RepeatCopy: repeats range [%d, %d] (0 <= min <= max)" % (min_repeats, max_repeats))
        if not norm_max > 0:
            raise _lib.NtkError("RepeatCopy: norm_max=%r (> 0)" % (norm_max,))
        self._num_bits, self._batch_size = int(num_bits), int(batch_size)
        self._min_length, self._max_length = int(min_length), int(max_length)
        self._min_repeats, self._max_repeats = int(min_repeats), int(max_repeats)
        self._norm_max = norm_max
        self._log_prob_in_bits, self._time_average_cost = bool(log_prob_in_bits), bool(time_average_cost)
        self.name = name
        self.device = torch.device(device)
        self.seed = int(seed or 0)
        #: leading dimension of X: num_bits + 2 channels rounded up to a multiple of 4, the ldx of a core built for them
        self.ldx = (self._num_bits + 2 + 3) // 4 * 4
        self._host_gen = torch.Generator().manual_seed(self.seed)
        self._dev_gen = None                       # made at the first draw: constructing a dataset touches no device

    time_average_cost = property(lambda self: self._time_average_cost)
    log_prob_in_bits = property(lambda self: self._log_prob_in_bits)
    num_bits = property(lambda self: self._num_bits)
    target_size = property(lambda self: self._num_bits + 1)
    batch_size = property(lambda self: self._batch_size)
    min_length = property(lambda self: self._min_length)
    max_length = property(lambda self: self._max_length)
    min_repeats = property(lambda self: self._min_repeats)
    max_repeats = property(lambda self: self._max_repeats)
    norm_max = property(lambda self: self._norm_max)

    def _normalise(self, val):
        return val / self._norm_max

    def _unnormalise(self, val):
        return val * self._norm_max

    # ---- sampling
    def sample_lengths(self):
        """The next (lengths, repeats) of a batch: int32 host tensors, uniform over the closed ranges, from the host generator."""
        B = self._batch_size
        lengths = torch.randint(self._min_length, self._max_length + 1, (B,), generator=self._host_gen, dtype=torch.int32)
        repeats = torch.randint(self._min_repeats, self._max_repeats + 1, (B,), generator=self._host_gen, dtype=torch.int32)
        return lengths, repeats

    def _device_gen(self):
        if self._dev_gen is None:
            self._dev_gen = torch.Generator(device=self.device).manual_seed(self.seed + 1)
        return self._dev_gen

    def rng_state(self):
        """Both generators' states (host byte tensors): with them restored, the same batch stream continues."""
        return {"host": self._host_gen.get_state(), "device": self._device_gen().get_state()}

    def set_rng_state(self, state):
        self._host_gen.set_state(state["host"])
        self._device_gen().set_state(state["device"])

    def __call__(self):
        lengths, repeats = self.sample_lengths()
        bits = torch.empty((self._batch_size, self._max_length, self._num_bits), device=self.device)
        bits.random_(0, 2, generator=self._device_gen())
        return self.from_arrays(bits, lengths, repeats)

    _build = __call__

    def from_arrays(self, bits, lengths, repeats, S=None, ldx=None):
        """Lay out given patterns: bits [B, max_length, num_bits] in {0, 1} (rows past a sequence's length are not read), lengths
        and repeats [B] host integers (values outside the dataset's ranges are clamped, here for S and in the kernel for the
        layout).  S: the padded step count, default the batch's longest own length; ldx: X's leading dimension, default self.ldx."""
        dev = self.device
        bits = torch.as_tensor(bits, dtype=torch.float32).to(dev).contiguous()
        if bits.dim() != 3 or bits.shape[1] != self._max_length or bits.shape[2] != self._num_bits:
            raise _lib.NtkError("RepeatCopy.from_arrays: bits %s, expected [B, %d, %d]" % (tuple(bits.shape), self._max_length, self._num_bits))
        B = bits.shape[0]
        lengths = torch.as_tensor(_host(lengths), dtype=torch.int32).reshape(-1)
        repeats = torch.as_tensor(_host(repeats), dtype=torch.int32).reshape(-1)
        if lengths.numel() != B or repeats.numel() != B:
            raise _lib.NtkError("RepeatCopy.from_arrays: %d patterns, %d lengths, %d repeats" % (B, lengths.numel(), repeats.numel()))
        cl = lengths.clamp(self._min_length, self._max_length)
        cr = repeats.clamp(self._min_repeats, self._max_repeats)
        own = cl.long() * (cr.long() + 1) + 3
        S = int(own.max()) if S is None else int(S)
        ldx = self.ldx if ldx is None else int(ldx)
        table = torch.stack([lengths, repeats])
        if dev.type == "cuda":
            table = table.pin_memory().to(dev, non_blocking=True)
        if S < 1 or ldx < 1:
            raise _lib.NtkError("RepeatCopy.from_arrays: S=%d ldx=%d" % (S, ldx))
        X = torch.empty((B, S, ldx), device=dev)
        target = torch.empty((B, S, self._num_bits + 1), device=dev)
        mask = torch.empty((B, S), device=dev)
        _lib.check(_lib.lib().ntk_repeat_copy_pack(_P(bits), _iptr(table[0]), _iptr(table[1]), _P(X), _P(target), _P(mask), B, S,
                                                   self._num_bits, ldx, self._min_length, self._max_length, self._min_repeats,
                                                   self._max_repeats, float(self._norm_max), _lib.stream()), "ntk_repeat_copy_pack")
        data = DatasetTensors(X[:, :, :self._num_bits + 2].transpose(0, 1), target.transpose(0, 1), mask.t())
        data.X, data.target_bm, data.mask_bm, data.lengths, data.repeats = X, target, mask, cl, cr
        return data

    # ---- cost and pictures
    def cost(self, logits, targ, mask):
        """repeat_copy.py:379-385: time-major logits / targ [S, B, num_bits + 1] and mask [S, B] -> the scalar loss."""
        return masked_sigmoid_cross_entropy(logits, targ, mask, time_average=self._time_average_cost,
                                            log_prob_in_bits=self._log_prob_in_bits)

    def cost_and_grad(self, logits_bm, data, want_grad=True):
        """The training step's form, on batch-major logits [B, S, num_bits + 1] and a batch of this module:
        (loss [1], loss_batch [B], dlogits or None, score [B, 2])."""
        return masked_xent(logits_bm, data.target_bm, data.mask_bm, self._time_average_cost, self._log_prob_in_bits, want_grad=want_grad)

    def to_human_readable(self, data, model_output=None, whole_batch=False):
        """repeat_copy.py:387-392: the repeat-count channel is shown as the count itself (un-normalised and rounded)."""
        obs = np.array(_host(data.observations), dtype=np.float32)
        obs[:, :, -1:] = self._unnormalise(obs[:, :, -1:]).round()
        shown = DatasetTensors(obs, _host(data.target), _host(data.mask))
        return bitstring_readable(shown, obs.shape[1] if whole_batch else 1, model_output, whole_batch)


def rounded_output(logits_bm, mask_bm):
    """train.py:104-105's round(mask * sigmoid(logits)), time-major [S, B, O]: 1 where a scored step's logit is positive (tf.round
    sends 0.5 to 0), 0 elsewhere -- by selection, so that what the kernels emit past a sequence's end cannot show."""
    one = (logits_bm > 0) & (mask_bm > 0).unsqueeze(-1)
    return one.to(torch.float32).transpose(0, 1)


class RepeatCopyTask(object):
    """train.py's model and optimiser around a RepeatCopy dataset (defaults: train.py:30-42): a DNC core (or, core="ntm", the
    single-layer NTM cell the way copy_task.CopyTask runs it), clip_by_global_norm(max_grad_norm) and RMSProp with TensorFlow's
    defaults (decay 0.9, momentum 0, train.py:123).  A shape the core's BPTT launcher refuses raises NtkError here, before anything
    is launched."""

    def __init__(self, dataset, core="dnc", memory_size=16, word_size=16, num_reads=1, num_writes=1, hidden_size=64, clip_value=20,
                 learning_rate=1e-4, optimizer_epsilon=1e-10, max_grad_norm=50, seed=0, similarity="as_coded"):
        from .tracker import RMSPropClip
        if core not in ("dnc", "ntm"):
            raise _lib.NtkError("RepeatCopyTask: core=%r (\"dnc\" or \"ntm\")" % (core,))
        self.dataset, self.kind = dataset, core
        self.device = dataset.device
        D, O = dataset.num_bits + 2, dataset.target_size
        if core == "dnc":
            self._refuse_dnc(dataset.batch_size, memory_size, word_size, num_reads, num_writes, hidden_size, O)
            from .dnc import DNC
            self.core = DNC({"memory_size": memory_size, "word_size": word_size, "num_reads": num_reads, "num_writes": num_writes},
                            {"hidden_size": hidden_size}, O, clip_value, input_dim=D, device=self.device, seed=seed or 0)
            self.cell = None
            params, ldx = self.core.params, self.core.ldx
        else:
            from .ntm import NTMCell, NTMDims, similarity_mode
            sim = similarity_mode(similarity)
            d = NTMDims(D, O, memory_size, word_size, 1, hidden_size, num_reads, num_writes)
            L = _lib.lib()
            if not L.ntk_ntm_seq_plan_sim(dataset.batch_size, d.N, d.Md, d.R, d.Wh, d.hid, d.shift_range, d.O, 0, sim, 0, 0,
                                          None, None, None, None) & 2:
                _lib.check(-3, "ntk_ntm_seq_bwd")
            self.cell = NTMCell(O, mem_size=memory_size, mem_dim=word_size, shift_range=1, controller_hidden_size=hidden_size,
                                controller_num_layers=1, write_head_size=num_writes, read_head_size=num_reads, input_dim=D,
                                device=self.device, seed=seed or 0, similarity=similarity)
            self.core = None
            params, ldx = self.cell.params, self.cell.dims.ldx
        if ldx != dataset.ldx:
            raise _lib.NtkError("RepeatCopyTask: the core reads rows of %d floats, the dataset packs %d" % (ldx, dataset.ldx))
        self.opt = RMSPropClip(params, learning_rate, 0.9, 0.0, optimizer_epsilon, max_grad_norm)
        self.last_data = self.last_logits = None

    @staticmethod
    def _refuse_dnc(B, N, word_size, R, Wn, hid, O):
        """Ask ntk_dnc_seq_bwd itself whether it takes the shape: with every pointer null it answers its shape clauses first and
        launches nothing (a shape it takes ends at the null-pointer clause)."""
        L = _lib.lib()
        W = (int(word_size) + 3) // 4 * 4
        K = R * W + hid
        rc = L.ntk_dnc_seq_bwd(int(B), 1, int(N), W, int(R), int(Wn), int(hid), int(O), 0.0, None, (K + 3) // 4 * 4, None,
                               (int(hid) + 3) // 4 * 4, *([None] * 30), 0, None)
        if rc != -2:                               # anything but "null pointer": a shape clause refused
            _lib.check(rc if rc != 0 else -1, "ntk_dnc_seq_bwd")

    params = property(lambda self: (self.core or self.cell).params)

    def _check_data(self, data):
        if data.X is None:
            raise _lib.NtkError("RepeatCopyTask: the batch has no packed buffers (make it with RepeatCopy() or from_arrays)")
        if data.X.shape[2] != self.dataset.ldx or data.target_bm.shape[2] != self.dataset.target_size:
            raise _lib.NtkError("RepeatCopyTask: batch rows of %d floats and %d target channels, the core takes %d and %d"
                                % (data.X.shape[2], data.target_bm.shape[2], self.dataset.ldx, self.dataset.target_size))

    def forward(self, data, record=False):
        """-> logits [B, S, num_bits + 1] batch-major (and, record=True, what BPTT needs, kept on the task)."""
        self._check_data(data)
        X = data.X
        B, S, ldx = X.shape
        if self.kind == "dnc":
            xproj = gemm_nt(X.view(B * S, ldx), self.core.WxT)
            out_tm, _ = self.core.run_projected(xproj, B, S, record=record)
            return out_tm.transpose(0, 1)                               # the kernel's own [B, S, O] buffer
        st0 = self.cell.zero_state(B)
        logits, _o, _n, rec = self.cell.run_sequence(X, st0, record=record, want_outputs=False)
        self._ntm = (st0, rec)
        return logits

    def loss_and_grads(self, data, dataset=None):
        """Forward, loss, BPTT: the gradient is in params.grad.  -> (loss [1] on the device, logits [B, S, num_bits + 1])."""
        ds = dataset or self.dataset
        logits = self.forward(data, record=True)
        loss, _lb, dlogits, _sc = ds.cost_and_grad(logits, data)
        if self.kind == "dnc":
            self.core.backward_sequence(data.X, dlogits, unpack=False)
            self.core.guard(loss, self.core.params.grad)
        else:
            st0, rec = self._ntm
            g0 = self.cell.backward_sequence(data.X, st0, rec, dlogits)
            self.cell.init_state_backward(g0, data.X.shape[0])
            self._ntm = None
        return loss, logits

    def train_step(self, data=None):
        """One optimiser step on `data` (default: the dataset's next batch) -> the loss before the update, [1] on the device."""
        data = self.dataset() if data is None else data
        loss, logits = self.loss_and_grads(data)
        self.opt.step(loss)
        self.last_data, self.last_logits = data, logits
        return loss

    def check_step(self):
        """Synchronises; raises if an optimiser step was skipped or a cluster launch aborted since the last check."""
        if self.core is not None:
            self.core.check_cluster()
        self.opt.check()

    def eval(self, n_batches, dataset=None):
        """Forward only over n_batches of `dataset` (default: the task's own; another one, e.g. with more repeats than trained on,
        is the reference's stated use of norm_max).  Loss and score accumulate on the device and are read back once.
        -> (mean loss, bit error rate, share of sequences copied without a wrong bit)."""
        ds = dataset or self.dataset
        if ds.num_bits != self.dataset.num_bits:
            raise _lib.NtkError("eval: the dataset has %d bits, the task %d" % (ds.num_bits, self.dataset.num_bits))
        acc = torch.zeros(4, device=self.device, dtype=torch.float64)      # loss, scored bits, wrong bits, perfect sequences
        nseq = 0
        for _ in range(int(n_batches)):
            data = ds()
            logits = self.forward(data)
            loss, _lb, _d, score = ds.cost_and_grad(logits, data, want_grad=False)
            acc[0] += loss[0]
            acc[1:3] += score.sum(0)
            acc[3] += (score[:, 1] == 0).sum()
            nseq += data.X.shape[0]
        a = acc.cpu().numpy()
        return float(a[0] / max(1, int(n_batches))), float(a[2] / max(1.0, a[1])), float(a[3] / max(1, nseq))

    # ---- checkpoints: parameters, optimiser slots, step and both generators' states
    FORMAT = "ntmtrack-repeat-copy-1"

    def save_checkpoint(self, path):
        P = self.params
        torch.save({"format": self.FORMAT, "core": self.kind, "numel": P.numel, "params": P.flat.detach().cpu(),
                    "ms": self.opt.ms.detach().cpu(), "mom": self.opt.mom.detach().cpu(), "global_step": int(self.opt.global_step),
                    "rng": self.dataset.rng_state()}, path)
        return path

    def load_checkpoint(self, path):
        ck = torch.load(path, map_location="cpu", weights_only=True)
        P = self.params
        if ck.get("format") != self.FORMAT or ck.get("core") != self.kind or ck.get("numel") != P.numel:
            raise _lib.NtkError("checkpoint %s: format %r core %r numel %r does not fit this task (%s, %s, %d)"
                                % (path, ck.get("format"), ck.get("core"), ck.get("numel"), self.FORMAT, self.kind, P.numel))
        P.flat.copy_(ck["params"])
        self.opt.ms.copy_(ck["ms"])
        self.opt.mom.copy_(ck["mom"])
        self.opt.global_step = int(ck["global_step"])
        self.dataset.set_rng_state(ck["rng"])
        return self.opt.global_step


def train(task, num_training_iterations, report_interval, log=print, checkpoint_path=None, checkpoint_interval=-1):
    """train.py:94-158's loop, from the task's global step to num_training_iterations.  The loss stays on the device between
    reports; a report reads back the interval's mean loss and prints the first sequence of the LAST TRAINING batch with the model's
    rounded, masked output on it (the reference draws one more batch for the picture).  -> the reported mean losses."""
    total = torch.zeros(1, device=task.device)
    reports = []
    for it in range(task.opt.global_step, int(num_training_iterations)):
        total += task.train_step()
        if (it + 1) % report_interval == 0:
            task.check_step()
            data = task.last_data
            text = task.dataset.to_human_readable(data, rounded_output(task.last_logits, data.mask_bm))
            reports.append(float(total.cpu()) / report_interval)
            log("%d: Avg training loss %f.\n%s" % (it, reports[-1], text))
            total.zero_()
        if checkpoint_interval > 0 and checkpoint_path and (it + 1) % checkpoint_interval == 0:
            task.save_checkpoint(checkpoint_path)
    return reports


def main(argv=None):
    """python -m ntmtrack.repeat_copy with train.py's flags (--checkpoint_dir holds one file, repeat_copy.ckpt, resumed if there)."""
    import argparse
    import os
    ap = argparse.ArgumentParser(description="Train the DNC (or NTM) core on the repeat-copy task.")
    for name, typ, default in (("hidden_size", int, 64), ("memory_size", int, 16), ("word_size", int, 16), ("num_write_heads", int, 1),
                               ("num_read_heads", int, 1), ("clip_value", int, 20), ("max_grad_norm", float, 50), ("learning_rate", float, 1e-4),
                               ("optimizer_epsilon", float, 1e-10), ("batch_size", int, 16), ("num_bits", int, 4), ("min_length", int, 1),
                               ("max_length", int, 2), ("min_repeats", int, 1), ("max_repeats", int, 2),
                               ("num_training_iterations", int, 100000), ("report_interval", int, 100), ("checkpoint_interval", int, -1),
                               ("seed", int, 0)):
        ap.add_argument("--" + name, type=typ, default=default)
    ap.add_argument("--checkpoint_dir", default=None)
    ap.add_argument("--core", default="dnc", choices=("dnc", "ntm"))
    ap.add_argument("--device", default="cuda")
    a = ap.parse_args(argv)
    dataset = RepeatCopy(a.num_bits, a.batch_size, a.min_length, a.max_length, a.min_repeats, a.max_repeats, device=a.device, seed=a.seed)
    task = RepeatCopyTask(dataset, a.core, a.memory_size, a.word_size, a.num_read_heads, a.num_write_heads, a.hidden_size, a.clip_value,
                          a.learning_rate, a.optimizer_epsilon, a.max_grad_norm, seed=a.seed)
    path = None
    if a.checkpoint_dir:
        os.makedirs(a.checkpoint_dir, exist_ok=True)
        path = os.path.join(a.checkpoint_dir, "repeat_copy.ckpt")
        if os.path.exists(path):
            print("resumed at step %d" % task.load_checkpoint(path))
    train(task, a.num_training_iterations, a.report_interval, checkpoint_path=path, checkpoint_interval=a.checkpoint_interval)


if __name__ == "__main__":
    main()
