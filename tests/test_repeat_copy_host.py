"""CPU: the repeat-copy restatements (tests/repeat_copy_util.py) against hand-written cases, the text pictures of
ntmtrack.repeat_copy, and the host sampler's ranges and reproducibility.  Nothing here needs a device."""
import numpy as np
import torch

import repeat_copy_util as U


def test_layout_restatement_is_the_docstrings_picture():
    """repeat_copy.py's own picture: L = 7, r = 3, num_bits = 2 -> 31 steps."""
    top, bot = [1, 0, 1, 1, 0, 0, 1], [0, 1, 0, 1, 0, 1, 0]
    bits = np.array([list(zip(top, bot))], np.float32)                      # [1, 7, 2]
    X, target, mask = U.layout(bits, [7], [3], norm_max=10)
    assert X.shape == (1, 31, 4) and target.shape == (1, 31, 3) and mask.shape == (1, 31)
    assert "".join("%d" % v for v in mask[0]) == "0" * 9 + "1" * 22
    assert "".join("%d" % v for v in target[0, :, 0]) == "0" * 9 + "101100110110011011001" + "0"
    assert "".join("%d" % v for v in target[0, :, 1]) == "0" * 9 + "010101001010100101010" + "0"
    assert "".join("%d" % v for v in target[0, :, 2]) == "0" * 30 + "1"
    assert "".join("%d" % v for v in X[0, :, 0]) == "0" + "1011001" + "0" * 23
    assert "".join("%d" % v for v in X[0, :, 1]) == "0" + "0101010" + "0" * 23
    assert "".join("%d" % v for v in X[0, :, 2]) == "1" + "0" * 30
    count = np.zeros(31, np.float32); count[8] = np.float32(3) / np.float32(10)
    assert np.array_equal(X[0, :, 3], count)


def test_layout_restatement_pads_the_batch_and_the_columns():
    bits = np.array([[[1, 0], [0, 0]], [[0, 1], [1, 1]]], np.float32)
    X, target, mask = U.layout(bits, [1, 2], [1, 2], norm_max=4, ldx=8)
    assert X.shape == (2, 9, 8) and not X[:, :, 4:].any()
    # sequence 0: L = 1, r = 1 -> own length 5, rows 5.. zero everywhere
    assert not X[0, 5:].any() and not target[0, 5:].any() and not mask[0, 5:].any()
    assert X[0, :5, :4].tolist() == [[0, 0, 1, 0], [1, 0, 0, 0], [0, 0, 0, 0.25], [0, 0, 0, 0], [0, 0, 0, 0]]
    assert target[0, :5].tolist() == [[0, 0, 0], [0, 0, 0], [0, 0, 0], [1, 0, 0], [0, 0, 1]]
    assert mask[0].tolist() == [0, 0, 0, 1, 1, 0, 0, 0, 0]
    # sequence 1: L = 2, r = 2 -> fills all 9 steps
    assert target[1].tolist() == [[0, 0, 0]] * 4 + [[0, 1, 0], [1, 1, 0], [0, 1, 0], [1, 1, 0], [0, 0, 1]]
    assert mask[1].tolist() == [0, 0, 0, 0, 1, 1, 1, 1, 1]
    assert X[1, 3, 3] == 0.5


def test_cost_restatement_by_hand():
    """One sequence, two scored steps of one channel: xent(0, 1) = ln 2, xent(ln 3, 0) = ln 4."""
    x = np.array([[[5.0], [0.0], [np.log(3.0)]]])
    z = np.array([[[1.0], [1.0], [0.0]]])
    m = np.array([[0.0, 1.0, 1.0]])
    loss, lb, d, score = U.cost(x, z, m)
    assert abs(loss - (np.log(2) + np.log(4))) < 1e-12 and abs(lb[0] - loss) < 1e-15
    np.testing.assert_allclose(d[0, :, 0], [0.0, -0.5, 0.75], atol=1e-12)
    assert score.tolist() == [[2, 2]]                                       # logit 0 rounds to 0 (target 1), logit ln 3 to 1 (target 0)
    loss_b, _, d_b, _ = U.cost(x, z, m, time_average=True, log_prob_in_bits=True)
    assert abs(loss_b - 3.0 / (2 + U.F32_EPS)) < 1e-12                      # (1 + 2) bits over two steps
    np.testing.assert_allclose(d_b[0, :, 0], np.array([0.0, -0.5, 0.75]) / (2 + U.F32_EPS) / np.log(2), atol=1e-12)
    # a masked-out step is selected out: NaN there changes nothing
    x[0, 0, 0] = np.nan
    loss_n, _, d_n, _ = U.cost(x, z, m)
    assert loss_n == loss and np.array_equal(d_n, d)
    t = lambda a: torch.tensor(a, dtype=torch.float64)
    assert abs(float(U.cost_torch(t(np.nan_to_num(x)), t(z), t(m), True, True)) - loss_b) < 1e-12


def test_human_readable_strings():
    from ntmtrack.repeat_copy import DatasetTensors, RepeatCopy, bitstring_readable
    bits = np.array([[[1, 0], [0, 1]], [[1, 1], [0, 0]]], np.float32)
    X, target, mask = U.layout(bits, [2, 1], [1, 2], norm_max=10)
    tm = lambda a: np.ascontiguousarray(np.swapaxes(a, 0, 1))
    data = DatasetTensors(tm(X), tm(target), tm(mask))
    ds = RepeatCopy(num_bits=2, batch_size=2, max_length=2, norm_max=10)
    want0 = ("Observations:\n+- 1 - - - - -+\n+- - 1 - - - -+\n+1 - - - - - -+\n+- - - 1 - - -+\n\n"
             "Targets:\n+- - - - 1 - -+\n+- - - - - 1 -+\n+- - - - - - 1+")
    assert ds.to_human_readable(data) == "\n" + want0
    shown = tm(X).copy(); shown[:, :, -1] = np.round(shown[:, :, -1] * 10)
    out = tm(target) * tm(mask)[:, :, None]
    whole = ds.to_human_readable(data, model_output=out, whole_batch=True)
    assert whole == "\n" + "\n\n\n\n".join(U.readable(shown[:, b], tm(target)[:, b], out[:, b]) for b in range(2))
    assert "Model Output:\n+- - - 1 1 - -+" in whole and "+- - 2 - - - -+" in whole           # sequence 1: two repeats shown as 2
    # the module-level function shows the observations as they are (0.1 is printed by %d as 0)
    assert bitstring_readable(data, 2).startswith("\nObservations:\n+- 1 - - - - -+") and "\n+- - - 0 - - -+" in bitstring_readable(data, 2)


def test_host_sampler_ranges_and_reproducibility():
    from ntmtrack.repeat_copy import RepeatCopy
    mk = lambda seed: RepeatCopy(num_bits=3, batch_size=64, min_length=2, max_length=5, min_repeats=1, max_repeats=4, seed=seed)
    a, b, c = mk(11), mk(11), mk(12)
    seen_l, seen_r, same_as_c = set(), set(), True
    for _ in range(20):
        la, ra = a.sample_lengths()
        lb, rb = b.sample_lengths()
        lc, rc = c.sample_lengths()
        assert la.dtype == torch.int32 and tuple(la.shape) == (64,) and tuple(ra.shape) == (64,)
        assert torch.equal(la, lb) and torch.equal(ra, rb)
        same_as_c = same_as_c and torch.equal(la, lc) and torch.equal(ra, rc)
        seen_l |= set(la.tolist()); seen_r |= set(ra.tolist())
    assert seen_l == {2, 3, 4, 5} and seen_r == {1, 2, 3, 4}
    assert not same_as_c
    assert (a.num_bits, a.target_size, a.batch_size, a.time_average_cost, a.log_prob_in_bits) == (3, 4, 64, False, False)
    assert a.ldx == 8
