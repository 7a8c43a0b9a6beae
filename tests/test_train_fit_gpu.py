"""GPU: train.fit -- the epoch loop over frame records (prefetcher -> one-launch input batches -> the two-stream pipeline) -- against
the same schedule written out by hand on the per-frame get_input, bit for bit; the validation losses against eval_loss; the same
loop on the DNC tracker; resuming from a checkpoint."""
import os

import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O

pytestmark = pytest.mark.gpu

B, T = 2, 2


@pytest.fixture(scope="module")
def vgg_weights():
    return O.init_vgg_weights(np.random.default_rng(0))


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """6 training and 2 validation sequences of T = 2 frame records each, PNG frames of two sizes."""
    from PIL import Image
    from ntmtrack import data
    root = tmp_path_factory.mktemp("records")
    rng = np.random.default_rng(11)
    for split, count in (("train", 6), ("val", 2)):
        for s in range(count):
            d = root / ("%s_seq%d_0" % (split, s))
            d.mkdir()
            for t in range(T):
                size = (48, 64, 3) if (s + t) % 2 == 0 else (40, 56, 3)
                png = str(d / ("frame%d.png" % t))
                Image.fromarray(rng.integers(0, 256, size=size, dtype=np.uint8)).save(png)
                stem = str(d / ("%06d" % t))
                rng.random((8, 8)).tofile(stem + ".bin")
                y1, x1 = [float(v) for v in rng.uniform(0.0, 0.3, size=2)]
                y2, x2 = [float(v) for v in rng.uniform(0.6, 1.0, size=2)]
                dy, dx = [0.0 if t == 0 else float(v) for v in rng.uniform(-0.4, 0.4, size=2)]
                with open(stem + ".txt", "w") as f:
                    f.write("%r,%r,%r,%r,0.3,0.3,0.6,0.6,%s,%r,%r" % (y1, x1, y2, x2, png, dy, dx))
    _all, train_seqs, val_seqs = data.get_valid_sequences(str(root), T)
    assert len(train_seqs) == 6 and len(val_seqs) == 2
    return train_seqs, val_seqs


def _state(trk):
    P = trk._ckpt_params()
    torch.cuda.synchronize()
    return P.flat.detach().cpu().numpy().copy(), trk.opt.ms.cpu().numpy().copy(), trk.opt.mom.cpu().numpy().copy()


def _same(a, b):
    return all(x.tobytes() == y.tobytes() for x, y in zip(a, b))


def test_fit_equals_the_hand_written_loop(cuda, vgg_weights, tree, tmp_path):
    from ntmtrack import data, tracker, train
    train_seqs, val_seqs = tree
    kw = dict(num_epochs=1, validation_interval=2, validation_batch=1, log_interval=1, seed=0)
    events = []
    trk = tracker.NTMOffsetTracker(B, T, vgg_weights=vgg_weights, device=cuda, seed=1)
    start = _state(trk)
    res = train.fit(trk, train_seqs, val_seqs, ckpt_dir=str(tmp_path / "ckpt"), on_event=events.append, **kw)
    assert res.steps == 3 and trk.opt.global_step == 3
    assert [s for s, _l in res.validation] == [0, 2, 3]                     # before steps 0 and 2, and the final one
    assert [s for s, _l in res.training] == [0, 1, 2]
    assert [os.path.basename(p) for p in res.checkpoints] == ["model-0.pt", "model-2.pt", "model-3.pt"]
    assert all(os.path.isfile(p) for p in res.checkpoints)
    assert [e[0] for e in events] == ["validate", "checkpoint", "train", "train", "validate", "checkpoint", "train", "validate",
                                      "checkpoint"]
    assert not _same(start, _state(trk))

    # the same run by hand: Schedule's order through the per-frame get_input and the same pipeline calls
    ref = tracker.NTMOffsetTracker(B, T, vgg_weights=vgg_weights, device=cuda, seed=1)
    assert _same(start, _state(ref))
    val_losses, train_losses = [], []
    for kind, step, payload in train.Schedule(len(train_seqs), len(val_seqs), B, seed=0, validation_interval=2, validation_batch=1,
                                              num_epochs=1):
        if kind == "validate":
            before = _state(ref)
            losses = [float(ref.eval_loss(*train.tracker_inputs(ref, *data.get_input(train.batch_names(val_seqs, b, T), device=cuda))))
                      for b in payload]
            assert _same(before, _state(ref)) and ref.opt.global_step == step          # eval_loss updates nothing
            val_losses.append((step, float(np.mean(losses))))
        else:
            frames, gts0, offsets = train.tracker_inputs(ref, *data.get_input(train.batch_names(train_seqs, payload, T), device=cuda))
            assert gts0.shape == (B, 64) and offsets.shape == (B, T, 2)
            ref.submit_features(frames)
            loss = ref.train_on_submitted(gts0, offsets)
            ref.check_step()
            train_losses.append((step, float(loss)))
    assert ref.opt.global_step == 3
    assert _same(_state(trk), _state(ref)), "fit and the hand-written loop ended with different parameters or slots"
    assert res.validation == val_losses
    assert res.training == train_losses
    assert all(np.isfinite(l) for _s, l in val_losses + train_losses)
    # the last checkpoint holds the final state
    ck = torch.load(res.checkpoints[-1], map_location="cpu", weights_only=True)
    assert ck["global_step"] == 3 and ck["params"].numpy().tobytes() == _state(trk)[0].tobytes()


def test_fit_without_the_prefetcher_and_with_flipped_images(cuda, vgg_weights, tree, tmp_path):
    """prefetch=False stages on the calling thread: same numbers.  reverse_image reaches the input path (other numbers)."""
    from ntmtrack import tracker, train
    train_seqs, val_seqs = tree
    kw = dict(num_epochs=1, validation_interval=2, validation_batch=1, log_interval=2, seed=0)
    runs = []
    for extra in (dict(), dict(prefetch=False), dict(reverse_image=True)):
        trk = tracker.NTMOffsetTracker(B, T, vgg_weights=vgg_weights, device=cuda, seed=1)
        res = train.fit(trk, train_seqs[:4], val_seqs, ckpt_dir=str(tmp_path / ("c%d" % len(runs))), **dict(kw, **extra))
        assert res.steps == 2 and [s for s, _l in res.training] == [0]          # log_interval 2: only step 0 is read
        runs.append((_state(trk), res.validation))
    assert _same(runs[0][0], runs[1][0]) and runs[0][1] == runs[1][1]
    assert not _same(runs[0][0], runs[2][0])


def test_fit_resumes_from_a_checkpoint(cuda, vgg_weights, tree, tmp_path):
    from ntmtrack import tracker, train
    train_seqs, val_seqs = tree
    kw = dict(num_epochs=1, validation_interval=100, validation_batch=1, log_interval=100, seed=0, ckpt_dir=str(tmp_path / "ckpt"))
    trk = tracker.NTMOffsetTracker(B, T, vgg_weights=vgg_weights, device=cuda, seed=1)
    first = train.fit(trk, train_seqs[:4], val_seqs, **kw)
    assert [os.path.basename(p) for p in first.checkpoints] == ["model-0.pt", "model-2.pt"]
    again = tracker.NTMOffsetTracker(B, T, vgg_weights=vgg_weights, device=cuda, seed=9)
    again.load_checkpoint(first.checkpoints[-1])
    assert again.opt.global_step == 2 and _same(_state(again), _state(trk))
    second = train.fit(again, train_seqs[:4], val_seqs, **kw)
    assert again.opt.global_step == 4 and second.steps == 2
    assert [os.path.basename(p) for p in second.checkpoints] == ["model-2.pt", "model-4.pt"]
    # same parameters and the same two validation sequences (their order within the batch may differ: a sum in another order)
    assert second.validation[0][1] == pytest.approx(first.validation[-1][1], rel=1e-5)


def test_fit_on_the_dnc_tracker(cuda, vgg_weights, tree, tmp_path):
    """One training step and one validation around it on the smallest memory the DNC core takes (4 words of 4)."""
    from ntmtrack import tracker, train
    train_seqs, val_seqs = tree
    trk = tracker.DNCOffsetTracker(B, T, vgg_weights=vgg_weights, mem_size=4, mem_dim=4, device=cuda, seed=3)
    res = train.fit(trk, train_seqs[:2], val_seqs, num_epochs=1, validation_interval=100, validation_batch=1, log_interval=1,
                    ckpt_dir=str(tmp_path / "ckpt"), seed=0)
    assert res.steps == 1 and trk.opt.global_step == 1
    assert [s for s, _l in res.validation] == [0, 1] and len(res.training) == 1
    assert all(np.isfinite(l) for _s, l in res.validation + res.training)
    trk.check_step()
