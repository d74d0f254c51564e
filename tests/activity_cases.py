"""Seeded cases for pr_activity_tracks, shared by tests/test_activity_cpu.py, tests/test_activity_native.py and
tests/test_activity_gpu.py, and the one comparison with tests/activity_ref.py that the native and the GPU test apply: EQUAL.

A case is a dict: rotmat f32[N,24,3,3], frame_no i32[N], track_start i64[T+1], H, R, G, E, dot_static, dot_move, dot_rapid, and
what the case plants (`planted`, read by tests/test_activity_cpu.py).  Every joint of a track turns about z from a random base
rotation by an angle per row, so the angle between two rows of a joint is the difference of their angles."""
import functools
import math

import numpy as np

import activity_ref
from smooth_cases import frames_with_gaps, rodrigues

TILE, CHUNK = 64, 32        # pr_activity_tile_rows(), pr_activity_chunk_rows(); the GPU and the native test assert that they still are
H0, R0, G0, E0 = 24, 3, 2, 3
DEG0 = (10.0, 15.0, 45.0)   # static, move, rapid
JITTER = 0.2                # degrees: far below every threshold


def thresholds(static_deg, move_deg, rapid_deg):
    return tuple(1.0 + 2.0 * math.cos(math.radians(float(d))) for d in (static_deg, move_deg, rapid_deg))


def track(rng, theta, jitter=JITTER):
    """theta: degrees about z per row, [n] (every joint alike) or [n,24] -> rotmat f32[n,24,3,3]."""
    theta = np.asarray(theta, np.float64)
    if theta.ndim == 1:
        theta = np.repeat(theta[:, None], 24, axis=1)
    n = len(theta)
    base = rodrigues(rng.uniform(-1.0, 1.0, (24, 3)))
    aa = np.zeros((n, 24, 3))
    aa[..., 2] = np.deg2rad(theta + rng.normal(0.0, jitter, (n, 24)) if jitter else theta)
    return (rodrigues(aa) @ base[None]).astype(np.float32)


def build(seed, tracks, H=H0, R=R0, G=G0, E=E0, deg=DEG0, **planted):
    """tracks: a list of (frame numbers int[n], theta) pairs, one per track (n = 0: an empty track)."""
    rng = np.random.default_rng(seed)
    parts = [track(rng, th) for _, th in tracks]
    ds, dm, dr = thresholds(*deg)
    return dict(rotmat=np.concatenate(parts) if parts else np.zeros((0, 24, 3, 3), np.float32),
                frame_no=(np.concatenate([np.asarray(f, np.int64) for f, _ in tracks]) if tracks else np.zeros(0, np.int64)).astype(np.int32),
                track_start=np.cumsum([0] + [len(f) for f, _ in tracks]).astype(np.int64), H=H, R=R, G=G, E=E, dot_static=ds, dot_move=dm,
                dot_rapid=dr, planted=planted)


def still(n, start=0):
    return np.arange(start, start + n), np.zeros(n)


def swinging(n, start=0, amp=40.0, period=10.0):
    return np.arange(start, start + n), amp * np.sin(2.0 * np.pi * np.arange(n) / period)


def ramp(n, step):
    return step * np.arange(n, dtype=np.float64)


def _empty():
    return build(1, [])


def _lengths():
    # tracks of 0, 1, H, H + 1 and H + G rows, all still and all starting at frame 0
    return build(2, [still(n) for n in (0, 1, H0, H0 + 1, H0 + G0, 0, 2)])


def _adjacent():
    # still | swinging | still, the frame numbers running on across the boundaries: a window that crossed one would look whole
    return build(3, [still(70), swinging(70, 70), still(70, 140)], planted_tracks=[(0, 70), (70, 140), (140, 210)])


def _still_segment():
    # 12 degrees a row (more than static, less than rapid over R rows), exactly H + 1 still rows, then on
    q, n = 40, 40 + H0 + 1 + 40
    th = np.concatenate([ramp(q, 12.0), np.full(H0 + 1, 12.0 * q), 12.0 * q + ramp(40, 12.0) + 12.0])
    return build(4, [(np.arange(n), th)], E=1000, first_still=q, last_still=q + H0)


def _oscillation():
    # a still track in which joints toggle by 20 degrees every second row, E times in the first track and E + 1 in the second
    tracks = []
    for n_events in (E0, E0 + 1):
        n = 3 * H0
        th = np.zeros((n, 24))
        for t in range(n_events):
            th[H0 + 2 * t:, list(activity_ref.JOINT_INDEX[4:8])] += 20.0 if t % 2 == 0 else -20.0
        tracks.append((np.arange(n), th))
    return build(5, tracks, first_event=H0, last_event=(H0 + 2 * (E0 - 1), H0 + 2 * E0))


def _jump():
    n, r = 60, 30
    th = np.zeros((n, 24))
    th[r:, activity_ref.JOINT_INDEX[1]] = 60.0
    return build(6, [(np.arange(n), th)], jump_row=r)


def _gaps():
    # a step of G frames keeps a window whole, a step of G + 1 breaks it and resets the anchor; both tracks still
    n = 3 * H0
    return build(7, [(frames_with_gaps(n, {20: G0, 21: G0}), np.zeros(n)), (frames_with_gaps(n, {20: G0 + 1}, start=5), np.zeros(n))],
                 gap_row=20)


def _edges():
    # track starts on tile and chunk boundaries and one row to either side of them
    lengths = (TILE, CHUNK, CHUNK - 1, 1, TILE + CHUNK, TILE - 1, 2, 2 * TILE + 1, 5)
    return build(8, [swinging(n, period=7.0 + t) if t % 2 else still(n) for t, n in enumerate(lengths)])


def _nan():
    c = build(9, [still(80), swinging(50)])
    c["rotmat"][30, activity_ref.JOINT_INDEX[0]] = np.nan          # one joint of one row
    c["rotmat"][50] = np.nan                                       # a whole row
    c["rotmat"][100, activity_ref.JOINT_INDEX[5], 1, 2] = np.nan   # one element
    return c


def _wild_frames():
    rng = np.random.default_rng(10)
    c = build(10, [swinging(90), still(70)])
    f = rng.integers(0, 40, 160)
    f[10:20] = np.sort(f[10:20])[::-1]
    f[40:60] = 7
    f[[3, 64, 100, 159]] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, np.iinfo(np.int32).min, np.iinfo(np.int32).max]
    f[110:150] = 1000 + np.arange(40)                               # ... and one stretch in order, so that something is held
    c["frame_no"] = f.astype(np.int32)
    return c


KNIFE = dict(k=10, i=40, b=2)


def _knife():
    # a track without jitter, every row the same bits except row k, whose joint b is 8 degrees off: dot_b(k, i) is the one number
    # below 3 in every window that holds k.  All three thresholds are set to it: held needs >=, an event and rapid need <
    n = 80
    th = np.zeros((n, 24))
    th[KNIFE["k"], activity_ref.JOINT_INDEX[KNIFE["b"]]] = 8.0
    rng = np.random.default_rng(11)
    c = build(11, [], H=H0 + 16, R=H0 + 16)
    c["rotmat"] = track(rng, th, jitter=0.0)
    c["frame_no"], c["track_start"] = np.arange(n, dtype=np.int32), np.array([0, n], np.int64)
    c["dot_static"] = c["dot_move"] = c["dot_rapid"] = activity_ref.dot_pair(c["rotmat"], KNIFE["k"], KNIFE["i"], KNIFE["b"])
    return c


def _big():
    # the one case whose window spans many LDS chunks and many tiles: H = 700 over 1 500 rows
    n1, n2 = 1150, 350
    th1 = np.concatenate([ramp(100, 12.0), np.full(n1 - 100, 1200.0)])
    th1 = np.repeat(th1[:, None], 24, axis=1)
    th1[400:, activity_ref.JOINT_INDEX[6]] += 30.0                  # the left elbow moves once, later
    for t in range(12):
        th1[900 + 3 * t:, activity_ref.JOINT_INDEX[11]] += 20.0 if t % 2 == 0 else -20.0
    return build(12, [(np.arange(n1), th1), swinging(n2, 3)], H=700, R=30, G=6, E=8)


def _many_tracks():
    return build(13, [still(3, 5 * t) for t in range(300)], H=2, R=1, G=1, E=0)


CASES = {"empty": _empty, "lengths": _lengths, "adjacent": _adjacent, "still_segment": _still_segment, "oscillation": _oscillation,
         "jump": _jump, "gaps": _gaps, "edges": _edges, "nan": _nan, "wild_frames": _wild_frames, "knife": _knife, "big": _big,
         "many_tracks": _many_tracks}
NAMES = list(CASES)
PARAMS = ("H", "R", "G", "E", "dot_static", "dot_move", "dot_rapid")


@functools.lru_cache(maxsize=None)
def case(name):
    c = CASES[name]()
    c["name"] = name
    for k in ("rotmat", "frame_no", "track_start"):
        c[k].setflags(write=False)
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """The reference of a case, computed once a process and shared; nobody writes into it."""
    c = case(name)
    ref = activity_ref.activity(c["rotmat"], c["frame_no"], c["track_start"], *(c[k] for k in PARAMS), threads=8 if name == "big" else 1)
    for v in ref.values():
        v.setflags(write=False)
    return ref


def check(name, got):
    """`got`: dict(flags, adds) of numpy arrays as the kernel wrote them: equal to reference(name), every row of every case."""
    ref = reference(name)
    for key in ("flags", "adds"):
        g = np.asarray(got[key])
        assert g.shape == ref[key].shape and g.dtype == np.int32, (name, key, g.shape, g.dtype)
        bad = np.argwhere(g != ref[key])
        assert bad.size == 0, f"{name}: {key} differs at (row, column) {bad[:6].tolist()}: got {g[tuple(bad[0])]:#x}, want {ref[key][tuple(bad[0])]:#x}"


def write_case(path, name):
    """The file tests/native/activity_host.cc reads: int32 N T H R G E, f64 dot_static dot_move dot_rapid, then track_start
    i32[T+1], frame_no i32[N], rotmat."""
    c = case(name)
    N, T = len(c["frame_no"]), len(c["track_start"]) - 1
    with open(path, "wb") as f:
        f.write(np.array([N, T, c["H"], c["R"], c["G"], c["E"]], np.int32).tobytes())
        f.write(np.array([c["dot_static"], c["dot_move"], c["dot_rapid"]], np.float64).tobytes())
        f.write(c["track_start"].astype(np.int32).tobytes() + c["frame_no"].tobytes() + c["rotmat"].tobytes())
    return path


def read_outputs(path, name):
    """What the driver wrote: flags i32[N,4], adds i32[N,4]."""
    N = len(case(name)["frame_no"])
    raw = np.fromfile(path, np.int32)
    assert raw.size == 8 * N
    return dict(flags=raw[:4 * N].reshape(N, 4), adds=raw[4 * N:].reshape(N, 4))
