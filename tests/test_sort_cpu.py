"""SORT on the host (poserisk_release_amd/sort.py): one Kalman step against hand-derived numbers, identities over time, the
reporting rule, the squared boxes, and the hand-off to tracks.target_track."""
import numpy as np

from poserisk_release_amd import sort, tracks


def test_one_kalman_predict_and_update_against_hand_derived_numbers():
    """A 20 x 40 box at (0, 0): z = (10, 20, 800, 0.5).  predict: x unchanged (zero velocity), P = F P0 F' + Q, so for a position
    p with its velocity v: P_pp = 10 + 1e4 + 1 = 10011, P_pv = 1e4, P_vv = 1e4 + 0.01; for the aspect: 10 + 1 = 11.
    update with the box moved by (+2, +4) and unchanged size, z = (12, 24, 800, 0.5): the gain of cx is
    P_pp / (P_pp + R) = 10011 / 10012, so cx = 10 + 2 * 10011 / 10012 and its velocity 2 * 1e4 / 10012; the area's R is 10:
    gain 10011 / 10021, innovation 0."""
    t = sort.KalmanBoxTracker(np.array([0.0, 0.0, 20.0, 40.0]), 1)
    assert np.array_equal(t.x, [10, 20, 800, 0.5, 0, 0, 0])
    box = t.predict()
    assert np.allclose(box, [0, 0, 20, 40], rtol=0, atol=1e-12) and t.time_since_update == 1 and t.age == 1
    assert np.isclose(t.P[0, 0], 10011.0) and np.isclose(t.P[0, 4], 1e4) and np.isclose(t.P[4, 4], 1e4 + 0.01)
    assert np.isclose(t.P[3, 3], 11.0) and np.isclose(t.P[2, 2], 10011.0) and np.isclose(t.P[6, 6], 1e4 + 1e-4)
    t.update(np.array([2.0, 4.0, 22.0, 44.0]))
    assert t.time_since_update == 0 and t.hits == 1 and t.hit_streak == 1
    g = 10011.0 / 10012.0
    np.testing.assert_allclose(t.x, [10 + 2 * g, 20 + 4 * g, 800, 0.5, 2 * 1e4 / 10012, 4 * 1e4 / 10012, 0], rtol=1e-12, atol=1e-12)
    np.testing.assert_allclose(t.P[0, 0], 10011.0 * (1 - g), rtol=1e-9)
    np.testing.assert_allclose(t.P[2, 2], 10011.0 * (1 - 10011.0 / 10021.0), rtol=1e-9)


def _moving(n, x0, y0, dx, dy, w=40.0, h=80.0):
    return [np.array([x0 + dx * f, y0 + dy * f, x0 + dx * f + w, y0 + dy * f + h, 0.9]) for f in range(n)]


def test_two_separated_moving_boxes_keep_their_ids():
    a, b = _moving(12, 10, 20, 3, 1), _moving(12, 300, 40, -2, 2)
    dets = [np.stack([p, q]) if f % 2 else np.stack([q, p]) for f, (p, q) in enumerate(zip(a, b))]      # the order in a frame does not matter
    out = sort.track_frames(dets)
    assert sorted(out) == [1, 2]
    first = out[1] if out[1]["bbox"][0, 0] < 150 else out[2]
    second = out[2] if first is out[1] else out[1]
    for t, path in ((first, a), (second, b)):
        assert t["frames"].tolist() == list(range(12)) and t["bbox"].dtype == np.float32
        centres = np.array([[(p[0] + p[2]) / 2, (p[1] + p[3]) / 2] for p in path])
        assert np.abs(t["bbox"][:, :2] - centres).max() < 2.0
    assert out == out and all(np.array_equal(sort.track_frames(dets)[k]["bbox"], out[k]["bbox"]) for k in out)      # deterministic


def test_a_late_track_is_reported_from_its_third_hit_and_gone_after_max_age_misses():
    early, late = _moving(14, 10, 20, 1, 0), _moving(14, 300, 40, 0, 1)
    dets = []
    for f in range(14):
        d = [early[f]]
        if 5 <= f <= 10:
            d.append(late[f])
        dets.append(np.stack(d))
    out = sort.track_frames(dets, max_age=1, min_hits=3)
    assert out[1]["frames"].tolist() == list(range(14))                # present from frame 0: reported at once (frame <= min_hits)
    # created at frame 5 (no hit yet), hits at 6, 7, 8: reported from the third; last seen at 10, never reported afterwards
    assert out[2]["frames"].tolist() == [8, 9, 10]
    s = sort.Sort(max_age=1, min_hits=3)
    for f in range(14):
        s.update(dets[f])
        if f == 11:
            assert len(s.trackers) == 2                                # one miss: kept (time_since_update 1 <= max_age)
        if f == 12:
            assert len(s.trackers) == 1                                # two misses: gone
    gap = [d if f != 7 else d[:1] for f, d in enumerate(dets)]        # a miss resets the streak: hits at 6, (miss 7), 8, 9, 10
    assert sort.track_frames(gap)[2]["frames"].tolist() == [10]


def test_no_detections_give_no_tracks_and_empty_frames_are_accepted():
    assert sort.track_frames([np.zeros((0, 5)) for _ in range(4)]) == {}
    out = sort.track_frames([np.zeros((0, 5))] + [d[None] for d in _moving(5, 0, 0, 1, 1)])
    # created at frame 1 and reported while frame <= min_hits (frames 1, 2 = the 2nd and 3rd); at frame 3 its streak is 2: not yet
    assert out[1]["frames"].tolist() == [1, 2, 4, 5]


def test_degenerate_detections_are_ignored_without_warnings():
    import warnings
    good = _moving(6, 10, 10, 1, 0)
    flat = np.array([300.0, 0.0, 340.0, 0.0, 0.9])                 # clipped to the frame's top edge: no height
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        out = sort.track_frames([np.stack([g, flat + f]) for f, g in enumerate(good)])
    assert list(out) == [1] and out[1]["frames"].tolist() == list(range(6))


def test_boxes_come_out_squared_and_pass_target_track():
    tall, wide = _moving(6, 10, 10, 1, 0, w=30, h=90), _moving(6, 200, 50, 0, 1, w=120, h=40)
    out = sort.track_frames([np.stack([p, q]) for p, q in zip(tall, wide)])
    for t, side in ((out[1], 90.0), (out[2], 120.0)):
        assert np.array_equal(t["bbox"][:, 2], t["bbox"][:, 3]) and np.abs(t["bbox"][:, 2] - side).max() < 1.0
    bbox, frames = tracks.target_track(out, 6)
    assert bbox.dtype == np.float32 and bbox.shape == (6, 4) and frames.tolist() == list(range(6))
    assert np.array_equal(bbox, out[2]["bbox"])                        # the larger mean area
