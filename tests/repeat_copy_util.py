"""Restatements the repeat-copy tests compare against (test_repeat_copy_host.py, test_repeat_copy_gpu.py):
  * the batch layout, built sequence by sequence by CONCATENATION, the way dnc/repeat_copy.py:252-377 builds it -- deliberately not
    the index arithmetic of the pack kernel;
  * masked_sigmoid_cross_entropy (:29-66) with its gradient and the copy score in numpy, in float64 or float32, and in torch for
    autograd through an oracle core.
A step whose mask is 0 is selected out (the module's documented departure from the reference's multiplication)."""
import numpy as np
import torch

F32_EPS = float(np.finfo(np.float32).eps)         # a Python float: as a numpy float32 scalar, 2 + eps would round back to 2


def clamp_table(values, lo, hi):
    return [min(max(int(v), lo), hi) for v in values]


def layout(bits, lengths, repeats, norm_max=10, S=None, ldx=None):
    """bits [B, max_length, num_bits], lengths / repeats [B] (already inside their ranges) -> batch-major float32
    (X [B, S, ldx], target [B, S, num_bits + 1], mask [B, S]); S defaults to the longest own length, ldx to num_bits + 2."""
    bits = np.asarray(bits, np.float32)
    B, _, nb = bits.shape
    z = lambda *s: np.zeros(s, np.float32)
    obs_all, targ_all, mask_all = [], [], []
    for b in range(B):
        L, r = int(lengths[b]), int(repeats[b])
        pattern = bits[b, :L]
        start = z(1, nb + 2); start[0, nb] = 1.0
        count = z(1, nb + 2); count[0, nb + 1] = np.float32(r) / np.float32(norm_max)
        obs = np.concatenate([start, np.concatenate([pattern, z(L, 2)], 1), count, z(L * r + 1, nb + 2)], 0)
        tiled = np.tile(pattern.reshape(-1), r).reshape(L * r, nb)
        end = z(1, nb + 1); end[0, nb] = 1.0
        targ = np.concatenate([z(L + 2, nb + 1), np.concatenate([tiled, z(L * r, 1)], 1), end], 0)
        mask = np.concatenate([z(L + 2), np.ones(L * r + 1, np.float32)], 0)
        assert obs.shape[0] == targ.shape[0] == mask.shape[0] == L * (r + 1) + 3
        obs_all.append(obs); targ_all.append(targ); mask_all.append(mask)
    longest = max(o.shape[0] for o in obs_all)
    S = longest if S is None else S
    assert S >= longest
    ldx = nb + 2 if ldx is None else ldx
    X = np.stack([np.concatenate([np.concatenate([o, z(o.shape[0], ldx - nb - 2)], 1), z(S - o.shape[0], ldx)], 0) for o in obs_all])
    target = np.stack([np.concatenate([t, z(S - t.shape[0], nb + 1)], 0) for t in targ_all])
    mask = np.stack([np.concatenate([m, z(S - m.shape[0])], 0) for m in mask_all])
    return X, target, mask


def cost(logits, target, mask, time_average=False, log_prob_in_bits=False, dtype=np.float64):
    """Batch-major logits / target [B, S, O], mask [B, S], evaluated in `dtype` ->
    (loss, loss_batch [B], dlogits [B, S, O], score [B, 2] int64)."""
    x, zt, m = np.asarray(logits).astype(dtype), np.asarray(target).astype(dtype), np.asarray(mask).astype(dtype)
    B = x.shape[0]
    on = (m != 0)[:, :, None]
    with np.errstate(invalid="ignore", over="ignore"):
        e = np.exp(-np.abs(x))
        xent = np.where(on, np.maximum(x, 0) - x * zt + np.log1p(e), dtype(0))
        sig = np.where(x >= 0, 1 / (1 + e), e / (1 + e))
    loss_batch = (xent.sum(2) * m).sum(1)
    scale = np.full((B,), 1.0, dtype) / dtype(B)
    if time_average:
        count = m.sum(1) + dtype(F32_EPS)
        loss_batch = loss_batch / count
        scale = scale / count
    loss = loss_batch.sum() / dtype(B)
    if log_prob_in_bits:
        loss = loss / np.log(dtype(2))
        scale = scale / np.log(dtype(2))
    with np.errstate(invalid="ignore"):
        dlogits = np.where(on, (sig - zt) * m[:, :, None] * scale[:, None, None], dtype(0))
        wrong = ((x > 0) != (zt > 0.5)) & on
    score = np.stack([on.sum((1, 2)) * x.shape[2], wrong.sum((1, 2))], 1).astype(np.int64)
    return loss, loss_batch, dlogits, score


def cost_torch(logits, target, mask, time_average=False, log_prob_in_bits=False):
    """The same loss on batch-major torch tensors (any float dtype), differentiable."""
    xent = torch.clamp(logits, min=0) - logits * target + torch.log1p(torch.exp(-torch.abs(logits)))
    loss_batch = (torch.where(mask != 0, xent.sum(2), torch.zeros_like(mask)) * mask).sum(1)
    if time_average:
        loss_batch = loss_batch / (mask.sum(1) + float(F32_EPS))
    loss = loss_batch.sum() / logits.shape[0]
    if log_prob_in_bits:
        loss = loss / float(np.log(2.0))
    return loss


def readable(obs, targ, out=None):
    """The text picture of ONE sequence (time-major [S, channels] arrays), restated: per block a title line and one line per channel,
    '+' at both ends, '-' for zero."""
    row = lambda v: "+" + " ".join("-" if a == 0 else str(int(a)) for a in v) + "+"
    blocks = ["Observations:\n" + "\n".join(row(obs[:, c]) for c in range(obs.shape[1])),
              "Targets:\n" + "\n".join(row(targ[:, c]) for c in range(targ.shape[1]))]
    if out is not None:
        blocks.append("Model Output:\n" + "\n".join(row(out[:, c]) for c in range(targ.shape[1])))
    return "\n\n".join(blocks)
