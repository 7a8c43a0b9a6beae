"""CPU: the host side of training from frame records -- data.crop_source_rect (the source rectangle a crop can touch),
data.pack_frames (the packed buffer and its frame table), train.Schedule (the event stream of a run) and data.InputPrefetcher (with
a fake staging function: no image is decoded and no device is touched)."""
import threading

import numpy as np
import pytest

f32 = np.float32


# ---- crop_source_rect: every tap of the composed fp32 sampling lies inside the rectangle -------------------------------------------

def _positions(lo, hi, R, n):
    """fp32 sample positions of one axis of the crop stage on a resized image of R rows, in the kernel's order of operations --
    and, since the compiler may contract either product of ``lo * (R-1) + k * step`` into an FMA, in both contracted forms too."""
    lo, hi, scale = f32(lo), f32(hi), f32(R - 1)
    if n == 1:
        return [np.array([f32(f32(f32(0.5) * f32(lo + hi)) * scale)], f32)]
    k = np.arange(n).astype(f32)
    step = f32(f32(f32(hi - lo) * scale) / f32(n - 1))
    base = f32(lo * scale)
    plain = (base + (k * step).astype(f32)).astype(f32)
    fma_k = (np.float64(base) + k.astype(np.float64) * np.float64(step)).astype(f32)
    fma_lo = (np.float64(lo) * np.float64(scale) + (k * step).astype(f32).astype(np.float64)).astype(f32)
    return [plain, fma_k, fma_lo]


def _source_taps(size, R, lo, hi, n):
    """Every source index the composed sampling reads on one axis (empty when every sample is outside the resized image)."""
    taps = set()
    ratio = f32(f32(size) / f32(R))
    for pos in _positions(lo, hi, R, n):
        pos = pos[(pos >= 0) & (pos <= f32(R - 1))]
        for r in np.unique(np.concatenate([np.floor(pos), np.ceil(pos)])).astype(np.int64):
            s0 = int(np.floor(f32(f32(r) * ratio)))
            taps.update((s0, min(s0 + 1, size - 1)))
    return taps


SOURCES = [(60, 80), (45, 37), (36, 64), (9, 200), (200, 9), (2, 2), (1, 1), (720, 1280), (1080, 1920), (480, 640)]
GEOMETRIES = [((36, 64), (24, 24)), ((720, 1280), (224, 224)), ((36, 64), (1, 1)), ((36, 64), (1, 24)), ((36, 64), (24, 1))]
EDGE_BOXES = [[0, 0, 1, 1], [-0.5, -0.25, 1.5, 1.25], [0.4, 0.1, 0.4, 0.9], [0.1, 0.4, 0.9, 0.4], [0.8, 0.9, 0.1, 0.2],
              [0.9, 0.1, 1.0, 1.0], [0.0, 0.9, 1.0, 1.0], [1.0, 1.0, 1.0, 1.0], [0, 0, 0, 0], [1.2, 1.3, 1.8, 1.9],
              [-0.9, -0.8, -0.1, -0.2], [-0.23, -0.1, 0.6, 1.3], [0.999, 0.999, 1.001, 1.001], [0.5, 0.5, 0.5, 0.5],
              [1.0, 0.0, 0.0, 1.0], [0.97, 0.97, 1.0, 1.0], [0.0, 0.0, 0.03, 0.03]]


def _boxes():
    rng = np.random.default_rng(7)
    rnd = rng.uniform(-0.4, 1.4, size=(300, 4))
    small = rng.uniform(0, 1, size=(100, 2))
    small = np.concatenate([small, small + rng.uniform(0.01, 0.3, size=(100, 2))], axis=1)     # preprocess.py-sized crops
    return EDGE_BOXES + rnd.tolist() + small.tolist()


@pytest.mark.parametrize("resize_to,crop", GEOMETRIES)
def test_crop_source_rect_covers_every_tap(resize_to, crop):
    from ntmtrack import data
    boxes = _boxes()
    checked = 0
    for bi, box in enumerate(boxes):
        H, W = SOURCES[bi % len(SOURCES)]
        for size in ((H, W), SOURCES[(bi + 3) % len(SOURCES)]):
            y0, x0, h, w = data.crop_source_rect(size, box, resize_to, crop, margin=2)
            assert h >= 1 and w >= 1 and 0 <= y0 and y0 + h <= size[0] and 0 <= x0 and x0 + w <= size[1], (size, box)
            rows = _source_taps(size[0], resize_to[0], box[0], box[2], crop[0])
            cols = _source_taps(size[1], resize_to[1], box[1], box[3], crop[1])
            if rows and cols:                       # a pixel is read only where both axes have a sample inside
                assert min(rows) >= y0 and max(rows) < y0 + h, (size, box, sorted(rows), (y0, h))
                assert min(cols) >= x0 and max(cols) < x0 + w, (size, box, sorted(cols), (x0, w))
            checked += 1
    assert checked == 2 * len(boxes)                # no box was skipped


def test_crop_source_rect_is_small_for_a_small_box_and_1x1_for_a_box_outside():
    from ntmtrack import data
    assert data.crop_source_rect((720, 1280), [1.2, 1.3, 1.8, 1.9]) == (0, 0, 1, 1)
    assert data.crop_source_rect((720, 1280), [-0.9, 0.1, -0.1, 0.9]) == (0, 0, 1, 1)
    y0, x0, h, w = data.crop_source_rect((720, 1280), [0.25, 0.25, 0.5, 0.5])
    assert h * w < 0.08 * 720 * 1280 and 170 <= y0 <= 180 and 310 <= x0 <= 320
    assert data.crop_source_rect((60, 80), [0, 0, 1, 1], (36, 64), (24, 24)) == (0, 0, 60, 80)


# ---- pack_frames -----------------------------------------------------------------------------------------------------------------

def _frames():
    rng = np.random.default_rng(3)
    return [rng.integers(0, 256, size=s + (3,), dtype=np.uint8) for s in [(60, 80), (45, 37), (9, 200)]]


@pytest.mark.parametrize("pack", ["rect", "full"])
@pytest.mark.parametrize("pad", [0, 1])
def test_pack_frames_table_and_bytes(pack, pad):
    from ntmtrack import data
    imgs = _frames()
    boxes = [[0.2, 0.25, 0.7, 0.8], [0, 0, 1, 1], [1.2, 1.3, 1.8, 1.9]]
    p = data.pack_frames(imgs, boxes, resize_to=(36, 64), crop=(24, 24), pack=pack, pad=pad)
    t = p.table.numpy()
    assert t.shape == (3, 7) and t.dtype == np.int64 and p.n == 3 and p.channels == 3
    np.testing.assert_array_equal(p.boxes.numpy(), np.asarray(boxes, np.float32))
    off = pad
    for i, img in enumerate(imgs):
        o, H, W, y0, x0, h, w = t[i]
        assert (o, H, W) == (off, img.shape[0], img.shape[1])
        want = (0, 0, H, W) if pack == "full" else data.crop_source_rect((H, W), boxes[i], (36, 64), (24, 24), 2)
        assert (y0, x0, h, w) == want
        np.testing.assert_array_equal(p.pixels.numpy()[o:o + h * w * 3].reshape(h, w, 3), img[y0:y0 + h, x0:x0 + w])
        off += h * w * 3
    assert p.nbytes == off == p.pixels.numel()
    if pack == "rect":
        assert tuple(t[2, 3:]) == (0, 0, 1, 1)


def test_pack_frames_reuses_and_grows_the_staging():
    from ntmtrack import data
    imgs = _frames()
    st = data.Staging()
    p1 = data.pack_frames(imgs[:1], [[0, 0, 1, 1]], (36, 64), (24, 24), pack="full", staging=st)
    base = st.pixels.data_ptr()
    p2 = data.pack_frames(imgs[:1], [[0.2, 0.2, 0.5, 0.5]], (36, 64), (24, 24), pack="rect", staging=st)
    assert p2.staging is st and st.pixels.data_ptr() == base and p1.staging is st          # smaller batch: same buffer
    p3 = data.pack_frames(imgs, [[0, 0, 1, 1]] * 3, (36, 64), (24, 24), pack="full", staging=st)
    assert p3.staging is st and st.pixels.numel() >= p3.nbytes and st.table.shape[0] >= 3
    other = data.Staging()
    p4 = data.pack_frames(imgs, [[0, 0, 1, 1]] * 3, (36, 64), (24, 24), pack="full", staging=other, grow=False)
    assert p4.staging is not other and other.pixels.numel() == 0                           # a set that must not grow is left alone


@pytest.mark.parametrize("col,value,named", [(0, -1, "leave the buffer"), (0, 10 ** 9, "leave the buffer"), (5, 0, "leaves the"),
                                             (6, 81, "leaves the"), (3, 1, "leaves the"), (4, -1, "leaves the"), (1, 0, "leaves the")])
def test_check_frame_table_refuses_a_row_outside_the_image_or_the_buffer(col, value, named):
    from ntmtrack import data
    table = np.array([[0, 60, 80, 0, 0, 60, 80], [14400, 45, 37, 2, 3, 10, 10]], np.int64)
    data.check_frame_table(table, 14400 + 300, 3)
    table[0, col] = value
    with pytest.raises(ValueError, match=named):
        data.check_frame_table(table, 14400 + 300, 3)
    with pytest.raises(ValueError, match="leave the buffer"):
        data.check_frame_table(np.array([[0, 60, 80, 0, 0, 60, 80]], np.int64), 14399, 3)


def test_pack_frames_refuses_what_it_cannot_pack():
    from ntmtrack import data
    imgs = _frames()
    with pytest.raises(ValueError):
        data.pack_frames(imgs, [[0, 0, 1, 1]] * 2)
    with pytest.raises(ValueError):
        data.pack_frames([imgs[0].astype(np.float32)], [[0, 0, 1, 1]])
    with pytest.raises(ValueError):
        data.pack_frames(imgs, [[0, 0, 1, 1]] * 3, pack="tiles")


def test_default_workers_follow_the_affinity_mask():
    import os
    from ntmtrack import data
    assert data.default_workers() == max(1, min(16, len(os.sched_getaffinity(0))))


# ---- Schedule --------------------------------------------------------------------------------------------------------------------

def _events(**kw):
    from ntmtrack import train
    args = dict(n_train=13, n_val=7, batch_size=2, seed=1, validation_interval=2, validation_batch=2, num_epochs=2)
    args.update(kw)
    return list(train.Schedule(**args))


def test_schedule_truncates_to_whole_batches_and_reshuffles_every_epoch():
    ev = _events()
    trains = [e for e in ev if e[0] == "train"]
    assert len(trains) == 12 and [e[1] for e in trains] == list(range(12))          # 13 // 2 = 6 batches per epoch, step counts on
    first, second = [i for e in trains[:6] for i in e[2]], [i for e in trains[6:] for i in e[2]]
    assert sorted(first) == sorted(second) == list(range(12))                        # sequence 12 is cut off; each epoch sees all
    assert first != second
    for e in ev:
        if e[0] == "validate":
            assert all(0 <= i < 6 for b in e[2] for i in b)                          # 7 // 2 * 2 = 6 validation sequences


def test_schedule_is_a_function_of_the_seed():
    assert _events() == _events()
    assert _events() != _events(seed=2)
    # the training order does not depend on how often validation runs
    assert [e for e in _events() if e[0] == "train"] == [e for e in _events(validation_interval=5) if e[0] == "train"]


def test_schedule_validation_cadence():
    ev = _events()
    kinds = [(e[0], e[1]) for e in ev]
    assert kinds[0] == ("validate", 0) and kinds[1] == ("train", 0)
    assert kinds[-1] == ("validate", 12) and kinds[-2] == ("train", 11)              # the final validation, after the last step
    assert [s for k, s in kinds if k == "validate"] == [0, 2, 4, 6, 8, 10, 12]
    for i, (k, s) in enumerate(kinds[:-1]):
        if k == "validate":
            assert kinds[i + 1] == ("train", s)                                      # before the batch of its step
    # an interval that does not divide the step count: the final validation is still there, once
    assert [e[1] for e in _events(validation_interval=5) if e[0] == "validate"] == [0, 5, 10, 12]
    assert [(e[0], e[1]) for e in _events(num_epochs=0)] == [("validate", 0)]


def test_schedule_validation_walks_distinct_batches_and_leaves_the_training_position_alone():
    ev = _events(validation_batch=2)
    vals = [e for e in ev if e[0] == "validate"]
    for e in vals:
        assert len(e[2]) == 2 and not set(e[2][0]) & set(e[2][1])                    # val_index moves on: two DISTINCT batches
    assert len(set(tuple(map(tuple, e[2])) for e in vals)) > 1                       # reshuffled before each validation
    assert all(len(e[2]) == 3 for e in _events(validation_batch=9) if e[0] == "validate")      # at most: only 3 batches exist
    # the deviation: validations every 2 steps inside 6-batch epochs, and every epoch still runs each of its batches once, in the
    # order of the run without them
    sparse = [e[2] for e in _events(validation_interval=1000) if e[0] == "train"]
    assert [e[2] for e in ev if e[0] == "train"] == sparse


def test_schedule_shards_are_disjoint_and_cover_the_batch():
    whole = _events(batch_size=4, n_train=16, n_val=8)
    r0, r1 = _events(batch_size=4, n_train=16, n_val=8, rank=0, world=2), _events(batch_size=4, n_train=16, n_val=8, rank=1, world=2)
    assert len(whole) == len(r0) == len(r1)
    for w, a, b in zip(whole, r0, r1):
        assert (w[0], w[1]) == (a[0], a[1]) == (b[0], b[1])
        if w[0] == "train":
            assert len(a[2]) == len(b[2]) == 2 and not set(a[2]) & set(b[2]) and a[2] + b[2] == w[2]
        else:
            for wb, ab, bb in zip(w[2], a[2], b[2]):
                assert not set(ab) & set(bb) and ab + bb == wb
    with pytest.raises(ValueError):
        _events(batch_size=3, world=2)


# ---- InputPrefetcher -------------------------------------------------------------------------------------------------------------

class Boom(Exception):
    pass


def test_prefetcher_keeps_order_surfaces_errors_at_their_batch_and_joins():
    from ntmtrack import data
    batches = [["b%d_f%d" % (i, j) for j in range(3)] for i in range(7)]
    threads, sets = set(), []

    def stage(names, staging):
        threads.add(threading.current_thread().name)
        sets.append(staging)
        if names[0].startswith("b3_"):
            raise Boom(names[0])
        return ("staged", tuple(names))

    before = threading.active_count()
    pf = data.InputPrefetcher(batches, depth=2, workers=1, stage=stage)
    assert len(pf) == 7 and pf._thread.daemon
    got = []
    for i in range(7):
        if i == 3:
            with pytest.raises(Boom, match="b3_f0"):
                next(pf)
            continue
        got.append(next(pf))
    with pytest.raises(StopIteration):
        next(pf)
    assert got == [("staged", tuple(b)) for i, b in enumerate(batches) if i != 3]
    assert threads == {"ntmtrack-input-prefetch"}                                   # staged off the consumer's thread
    assert len(set(map(id, sets))) == 2 and all(a is not b for a, b in zip(sets, sets[1:]))     # two sets, alternating
    pf.close()
    assert not pf._thread.is_alive() and threading.active_count() == before
    pf.close()                                                                      # idempotent


def test_prefetcher_close_before_the_end_joins_and_context_manager_closes():
    from ntmtrack import data
    batches = [["x%d" % i] for i in range(50)]
    with data.InputPrefetcher(batches, depth=2, workers=2, stage=lambda names, staging: names) as pf:
        assert next(pf) == ["x0"] and next(pf) == ["x1"]
        thread, pool = pf._thread, pf._pool
    assert not thread.is_alive() and pool._shutdown
    with pytest.raises(StopIteration):
        next(pf)
    with pytest.raises(ValueError):
        data.InputPrefetcher(batches, depth=0)


def test_prefetcher_consumes_a_generator_lazily_and_reports_its_failure():
    """The batches may come from a generator: it is advanced on the staging thread, no further ahead than the staging sets allow,
    and an exception it raises surfaces at the batch it could not make; nothing follows."""
    from ntmtrack import data
    made = []

    def batches():
        for i in range(5):
            if i == 3:
                raise Boom("batch 3")
            made.append(i)
            yield ["g%d" % i]

    pf = data.InputPrefetcher(batches(), depth=2, workers=1, stage=lambda names, staging: names)
    assert next(pf) == ["g0"]
    assert len(made) <= 3                                                           # batch 0 handed out, at most two more staged
    assert next(pf) == ["g1"] and next(pf) == ["g2"]
    with pytest.raises(Boom, match="batch 3"):
        next(pf)
    with pytest.raises(StopIteration):
        next(pf)
    with pytest.raises(TypeError):
        len(pf)
    pf.close()
    assert not pf._thread.is_alive()
