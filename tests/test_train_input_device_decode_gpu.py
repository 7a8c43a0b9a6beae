"""GPU: the training input with decode="device" -- JPEG frames decoded by ntk_jpeg_decode_batch into the pixel buffer the crop
kernel reads -- gives the bytes of decode="host" (Pillow on the decoder threads): get_input_batch, InputPrefetcher and train.fit,
on record trees whose batches mix JPEG files of two sizes with a PNG and a progressive JPEG (both decoded by the host into the
same staging set); a truncated file stops fit with an NtkError that names it."""
import os
import sys

import numpy as np
import pytest
import torch

from oracle import ntm_oracle as O

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import jpeg_util as J  # noqa: E402

pytestmark = pytest.mark.gpu

B, T = 2, 2
WHAT = ("batch_img", "batch_gt", "y_offsets", "x_offsets")


def _write_image(path_stem, index):
    """Frame `index` of a tree: JPEG 4:2:0 (60x80) / JPEG 4:2:2 with restart markers (45x37) / PNG / progressive JPEG / JPEG 4:4:4"""
    from PIL import Image
    kind = index % 5
    size = [(60, 80), (45, 37), (45, 37), (60, 80), (60, 80)][kind]
    arr = J.image(size[0], size[1], "noise" if index % 2 else "smooth", seed=index)
    if kind == 2:
        path = path_stem + ".png"
        Image.fromarray(arr).save(path)
        return path
    path = path_stem + ".jpg"
    kw = [dict(subsampling=2), dict(subsampling=1, restart_marker_blocks=2), None, dict(progressive=True), dict(subsampling=0)][kind]
    with open(path, "wb") as f:
        f.write(J.encode(arr, quality=90, **kw))
    return path


def _record(d, t, image, rng, box=None):
    stem = str(d / ("%06d" % t))
    rng.random((8, 8)).tofile(stem + ".bin")
    if box is None:
        y1, x1 = [float(v) for v in rng.uniform(0.0, 0.3, size=2)]
        y2, x2 = [float(v) for v in rng.uniform(0.6, 1.0, size=2)]
        box = "%r,%r,%r,%r" % (y1, x1, y2, x2)
    dy, dx = [0.0 if t == 0 else float(v) for v in rng.uniform(-0.4, 0.4, size=2)]
    with open(stem + ".txt", "w") as f:
        f.write("%s,0.3,0.3,0.6,0.6,%s,%r,%r" % (box, image, dy, dx))
    return stem


@pytest.fixture(scope="module")
def frames(tmp_path_factory):
    """Five frame records: two JPEG sizes, a PNG and a progressive JPEG among them, boxes inside, over and across the frame."""
    d = tmp_path_factory.mktemp("device_decode") / "train_seq_0"
    d.mkdir()
    rng = np.random.default_rng(5)
    boxes = ["0.1,0.15,0.9,0.8", "0.0,0.0,1.0,1.0", "-0.2,0.3,0.6,1.2", "0.45,0.4,0.75,0.7", "0.3,0.1,0.5,0.95"]
    return [_record(d, i, _write_image(str(d / ("img%d" % i)), i), rng, boxes[i]) for i in range(5)]


def _bytes_equal(got, ref):
    for g, r, what in zip(got, ref, WHAT):
        assert g.shape == r.shape and g.dtype == r.dtype, what
        assert g.cpu().numpy().tobytes() == r.cpu().numpy().tobytes(), "%s differs" % what


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("pack", ["rect", "full"])
def test_get_input_batch_device_decode_gives_the_bytes_of_host_decode(cuda, frames, reverse, pack):
    from ntmtrack import data
    ref = data.get_input_batch(frames, device=cuda, reverse_image=reverse, workers=2, pack=pack)
    staged = data.stage_batch(frames, pack=pack, decode="device")
    assert staged.packed.jpeg.on_device == [True, True, False, False, True]
    got = data.get_input_batch(frames, device=cuda, reverse_image=reverse, workers=2, pack=pack, decode="device")
    torch.cuda.synchronize()
    _bytes_equal(got, ref)


def test_prefetcher_device_decode_matches_over_three_batches_from_a_too_small_first_set(cuda, frames):
    from ntmtrack import data
    batches = [frames[:1], frames, frames[1:4]]                 # the first set is sized by one small frame, then outgrown
    refs = [data.get_input_batch(b, device=cuda, workers=1) for b in batches]
    with data.InputPrefetcher(batches, depth=2, workers=2, decode="device") as source:
        count = 0
        for staged, ref in zip(source, refs):
            got = data.upload_staged(staged, cuda)
            staged.check_status()
            _bytes_equal(got, ref)
            count += 1
    assert count == 3


def test_decode_keyword_is_checked(frames):
    from ntmtrack import data
    with pytest.raises(ValueError):
        data.stage_batch(frames, decode="gpu")


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """4 training and 2 validation sequences of T = 2 frame records; the frames cycle through _write_image's five kinds."""
    from ntmtrack import data
    root = tmp_path_factory.mktemp("device_decode_records")
    rng = np.random.default_rng(11)
    k = 0
    for split, count in (("train", 4), ("val", 2)):
        for s in range(count):
            d = root / ("%s_seq%d_0" % (split, s))
            d.mkdir()
            for t in range(T):
                _record(d, t, _write_image(str(d / ("frame%d" % t)), k), rng)
                k += 1
    _all, train_seqs, val_seqs = data.get_valid_sequences(str(root), T)
    assert len(train_seqs) == 4 and len(val_seqs) == 2
    return str(root), train_seqs, val_seqs


def _state(trk):
    P = trk._ckpt_params()
    torch.cuda.synchronize()
    return P.flat.detach().cpu().numpy().copy(), trk.opt.ms.cpu().numpy().copy(), trk.opt.mom.cpu().numpy().copy()


@pytest.fixture(scope="module")
def vgg_weights():
    return O.init_vgg_weights(np.random.default_rng(0))


def test_fit_device_decode_gives_the_losses_and_parameters_of_host_decode(cuda, vgg_weights, tree, tmp_path):
    from ntmtrack import tracker, train
    _root, train_seqs, val_seqs = tree
    runs = []
    for decode in ("host", "device"):
        trk = tracker.NTMOffsetTracker(B, T, vgg_weights=vgg_weights, device=cuda, seed=1)
        res = train.fit(trk, train_seqs, val_seqs, num_epochs=1, validation_interval=100, validation_batch=1, log_interval=1, seed=0,
                        ckpt_dir=str(tmp_path / decode), decode=decode)
        assert res.steps == 2 and len(res.training) == 2 and len(res.validation) == 2
        runs.append((res.training, res.validation, _state(trk)))
    assert runs[0][0] == runs[1][0] and runs[0][1] == runs[1][1], (runs[0][:2], runs[1][:2])
    assert all(a.tobytes() == b.tobytes() for a, b in zip(runs[0][2], runs[1][2])), "final parameters or optimiser slots differ"


def test_a_truncated_file_in_fit_raises_an_error_that_names_it(cuda, vgg_weights, tree, tmp_path):
    """The file is jpeg_util.truncated_file(), the one tests/test_jpeg_host.py decodes on the CPU under the sanitizers."""
    import shutil
    from ntmtrack import _lib, data, tracker, train
    root, _t, _v = tree
    copy = str(tmp_path / "copy")
    shutil.copytree(root, copy)
    cut = str(tmp_path / "cut.jpg")
    with open(cut, "wb") as f:
        f.write(J.truncated_file())
    record = os.path.join(copy, "train_seq1_0", "000001.txt")
    fields = open(record).read().split(",")
    fields[8] = cut
    with open(record, "w") as f:
        f.write(",".join(fields))
    _all, train_seqs, val_seqs = data.get_valid_sequences(copy, T)
    assert len(train_seqs) == 4 and len(val_seqs) == 2
    trk = tracker.NTMOffsetTracker(B, T, vgg_weights=vgg_weights, device=cuda, seed=1)
    with pytest.raises(_lib.NtkError) as e:
        train.fit(trk, train_seqs, val_seqs, num_epochs=1, validation_interval=100, validation_batch=1, log_interval=1, seed=0,
                  ckpt_dir=str(tmp_path / "ckpt"), decode="device")
    assert "cut.jpg" in str(e.value) and "status 2" in str(e.value), str(e.value)
