"""CPU: the supervised protocol's host side -- the NumPy restatement of its rules (tests/supervised_util.py) on a hand-worked
trajectory, evaluate.summarize_supervised on that table, and the refusal of an unknown protocol."""
import numpy as np
import pytest

import supervised_util as S

GT = (10.0, 10.0, 100.0, 80.0)
QUARTER = (30.0, 20.0, 50.0, 40.0)              # contained in GT: 2000 / 8000 = 0.25 exactly
AWAY = (110.0, 10.0, 40.0, 80.0)                # touches GT along x = 110: overlap exactly 0
ABSENT = (np.nan,) * 4


def hand_worked():
    """A 12-frame clip (frame 0 starts the tracker, frames 1..11 are walked) with skip = 3 and burn_in = 2."""
    #        frame  1        2     3   4   5       6   7        8        9        10  11
    pred = [QUARTER, AWAY, GT, GT, GT, GT, QUARTER, QUARTER, QUARTER, GT, AWAY]
    gt = [GT, GT, GT, GT, ABSENT, GT, GT, GT, GT, GT, GT]
    return np.array(pred)[:, None], np.array(gt)[:, None]


def test_the_restatement_on_a_hand_worked_trajectory():
    pred, gt = hand_worked()
    codes, ious, table, state = S.walk(pred, gt, [1], 3, skip=3, burn_in=2)
    # frame 1: tracked inside the burn-in of the start (since = 1).  frame 2: overlap 0, the first failure, after 1 judged frame.
    # frames 3, 4: the slot waits (countdown 2, 1).  frame 5: the countdown is 0 but the object is absent: the restart slips.
    # frame 6: restarted.  frames 7, 8: since = 1, 2, inside the burn-in.  frames 9, 10: since = 3, 4, valid: 0.25 + 1.0.
    # frame 11: the second failure, on the last frame: no restart follows.
    assert codes[:, 0].tolist() == [0, 2, 3, 3, 3, 1, 0, 0, 0, 0, 2]
    want = np.zeros((3, S.HEAD))
    want[:, S.FIRST_FAILURE] = -1
    want[1] = [2, 1.25, 2, 1, 7, 3, 1]          # VALID, SUM_IOU, FAILURES, RESTARTS, TRACKED, SKIPPED, FIRST_FAILURE
    np.testing.assert_array_equal(table, want)
    np.testing.assert_array_equal(ious[:, 0], [0.25, 0.0, np.nan, np.nan, np.nan, np.nan, 0.25, 0.25, 0.25, 1.0, 0.0])
    assert state[0].tolist() == [S.WAIT, 3, 4]


def test_an_absent_object_while_tracking_is_counted_nowhere_and_an_inactive_frame_changes_nothing():
    pred, gt = hand_worked()
    gt[7, 0] = ABSENT                            # frame 8, tracked: since still advances, so frames 9 and 10 stay valid
    active = np.ones((12, 1), dtype=np.uint8)
    pred2, gt2 = np.insert(pred, 3, pred[3], axis=0), np.insert(gt, 3, gt[3], axis=0)
    active[3, 0] = 0                             # an inactive frame between frames 3 and 4 of the wait
    codes, _ious, table, _state = S.walk(pred2, gt2, [0], 1, active=active, skip=3, burn_in=2)
    assert codes[:, 0].tolist() == [0, 2, 3, -1, 3, 3, 1, 0, 0, 0, 0, 2]
    assert table[0].tolist() == [2, 1.25, 2, 1, 6, 3, 1]


def test_summarize_supervised():
    from ntmtrack import evaluate as E
    _codes, _ious, table, _state = S.walk(*hand_worked(), [1], 3, skip=3, burn_in=2)
    table[2] = [0, 0.0, 1, 0, 1, 0, 0]          # one judged frame, a failure: no valid frame
    table[0] = [6, 4.5, 0, 0, 8, 0, -1]
    r = E.summarize_supervised(table)
    c = r["clips"]
    np.testing.assert_array_equal(c["accuracy"], [0.75, 0.625, np.nan])
    assert c["valid"].tolist() == [6, 2, 0] and c["failures"].tolist() == [0, 2, 1] and c["restarts"].tolist() == [0, 1, 0]
    assert c["tracked"].tolist() == [8, 7, 1] and c["skipped"].tolist() == [0, 3, 0] and c["first_failure"].tolist() == [-1, 1, 0]
    assert r["accuracy_clips"] == (0.75 + 0.625) / 2 and r["accuracy_frames"] == 5.75 / 8
    assert r["failures"] == 3 and r["restarts"] == 1 and r["tracked"] == 16 and r["skipped"] == 3 and r["valid"] == 8
    assert r["failures_per_100_frames"] == 100.0 * 3 / 16 and r["clips_never_failed"] == 1
    empty = E.summarize_supervised(S.new_table(2))
    assert np.isnan(empty["clips"]["accuracy"]).all() and np.isnan(empty["accuracy_clips"]) and np.isnan(empty["accuracy_frames"])
    assert np.isnan(empty["failures_per_100_frames"]) and empty["clips_never_failed"] == 0


def test_an_unknown_protocol_is_refused_without_a_device():
    from ntmtrack import evaluate as E
    clips = [E.Clip(np.zeros((3, 16, 24, 3), dtype=np.uint8), np.tile(np.array([4.0, 4.0, 8.0, 8.0]), (3, 1)))]
    with pytest.raises(ValueError, match="nonsense"):
        E.validate(None, clips, 2, 2, protocol="nonsense", device="cpu")
    with pytest.raises(ValueError):
        E.Supervisor(2, 3, skip=0, device="cpu")
    with pytest.raises(ValueError):
        E.Supervisor(2, 3, burn_in=-1, device="cpu")
    s = E.Supervisor(2, 3, device="cpu")
    assert s.state.shape == (2, E.SUP_STATE_INTS) and (s.state == 0).all()
    assert (s.table[:, E.SUP_FIRST_FAILURE] == -1).all() and (s.table[:, :E.SUP_FIRST_FAILURE] == 0).all()
