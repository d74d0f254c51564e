"""Seeded cases for pr_activity_tracks, shared by tests/test_activity_cpu.py, tests/test_activity_native.py and
tests/test_activity_gpu.py, and the one comparison with tests/activity_ref.py that the native and the GPU test apply: EQUAL.

A case is a dict: rotmat f32[N,24,3,3], frame_no i32[N], track_start i64[T+1], H, R, G, E, dot_static, dot_move, dot_rapid, and
what the case plants (`planted`, read by tests/test_activity_cpu.py).  Every joint of a track turns about z from a random base
rotation by an angle per row, so the angle between two rows of a joint is the difference of their angles.  Besides CASES there
is a seeded sweep: `sweep_problem(q)` draws problem q, and case() / reference() / check() take its name `sweep_<q>` like any
other."""
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


I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
LATTICE = ((31, 31), (32, 1), (33, 33), (63, 40), (64, 64), (65, 33), (96, 96), (100, 50))
LATTICE_ROWS = (200, 130, 70)


def wild_frame_numbers(rng, n):
    """Frame numbers that obey nothing, as in wild_frames: drawn from 0..39, a descending and a constant stretch, the int32
    extremes, and the last third (24 rows at the most) in order so that something can be held."""
    f = rng.integers(0, 40, n).astype(np.int64)
    f[10:20] = np.sort(f[10:20])[::-1]
    f[22:30] = 7
    if n > 3:
        f[[3, n // 2]] = I32_MIN, I32_MAX
    tail = min(24, n // 3)
    f[n - tail:] = 1000 + np.arange(tail)
    return f


def walk(rng, n, still=(), jumps=(), sd=1.0):
    """Degrees [n,24]: a random walk of `sd` degrees a row per joint that stands still over the row ranges `still` and jumps at
    `jumps`, a list of (row, degrees, scored-joint bits)."""
    step = rng.normal(0.0, sd, (n, 24))
    for a, b in still:
        step[a + 1:b] = 0.0
    for row, deg, bits in jumps:
        step[row, [activity_ref.JOINT_INDEX[b] for b in bits]] += deg
    return np.cumsum(step, axis=0)


def _lattice(H, R):
    # (H, R) on and beside CHUNK and TILE.  Track 0 (rows 0 .. 199): a still stretch longer than every H; at row 108 three
    # joints jump by 58 degrees and then walk slowly; row 128, the first of the third tile, repeats row 127's frame number -- a
    # hole.  So for R > CHUNK the rows from 139 on are rapid only through row 107, CHUNK rows or more back, in a window that is
    # not covered: the lane has to ask for an older chunk although it has given up on held and repeated.  Then six events
    # in 16 rows (repeated), steps of G frames and further jumps.  Track 1 (rows 200 .. 329) has the same figure with its hole
    # on row 256 and ends still.  Track 2 has wild frame numbers
    def make():
        rng = np.random.default_rng(20)
        n0, n1, n2 = LATTICE_ROWS
        shakes = [(132 + 3 * t, 20.0 if t % 2 == 0 else -20.0, (4, 7)) for t in range(6)]
        th0 = walk(rng, n0, still=[(0, 101)], jumps=[(108, 58.0, (0, 5, 9)), *shakes, (170, -35.0, (1, 6)), (185, 22.0, (2, 3, 7))], sd=0.4)
        f0 = frames_with_gaps(n0, {128: 0, 150: G0, 151: G0, 160: 2, 176: G0 + 1})
        th1 = walk(rng, n1, still=[(70, 130)], jumps=[(8, 45.0, (0, 10)), (20, 28.0, (6,)), (36, -58.0, (4, 8, 11))], sd=0.4)
        f1 = frames_with_gaps(n1, {6: G0 + 1, 25: G0, 56: 0, 100: 2}, start=17)
        th2 = walk(rng, n2, still=[(46, 70)], jumps=[(12, 50.0, (0, 1, 2)), (35, -40.0, (5, 6))], sd=2.0)
        return build(20, [(f0, th0), (f1, th1), (wild_frame_numbers(rng, n2), th2)], H=H, R=R)
    return make


def _span_edge():
    # every track still; what differs is the span frame_no[i] - frame_no[p] of each track's LAST window, planted on H - G
    # (not whole: nothing in the track is held) and on H - G + 1 (whole: held, spread back over the window)
    s = H0 - G0
    plain = lambda span: np.arange(span + 1)                                     # gap-free from the track's start
    stepped = lambda span: np.concatenate([np.arange(span - 1), [span]])          # ... the last step one of G = 2 frames
    behind = lambda span: np.concatenate([np.arange(10), 1000 + np.arange(span + 1)])      # p is not the track's first row
    twos = lambda span: np.arange(0, span + 1, 2)                                 # every step G frames (s is even)
    tracks, planted = [], dict(not_whole=[], whole=[], untouched=[])
    row = 0
    for make in (plain, stepped, behind):
        for span, key in ((s, "not_whole"), (s + 1, "whole")):
            f = make(span)
            tracks.append((f, np.zeros(len(f))))
            if make is behind:
                planted["untouched"].extend(range(row, row + 10))
            row += len(f)
            planted[key].append(row - 1)
    for span, key in ((s, "not_whole"), (s + 2, "whole")):
        f = twos(span)
        tracks.append((f, np.zeros(len(f))))
        row += len(f)
        planted[key].append(row - 1)
    return build(21, tracks, **planted)


def _g_huge():
    # G = INT32_MAX: no step is too long, H - G is far below 0 (in 64 bits), so every window without a step < 1 is whole
    n = 3 * H0
    return build(22, [(frames_with_gaps(n, {20: 2, 21: 1000, 40: 2 ** 30}), np.zeros(n)), swinging(50, 5), still(1, 9),
                      (np.array([4, 4, 5, 6, 5, 6, 7]), np.zeros(7))], G=I32_MAX)


def _g_gt_h():
    # G > H: every covered window is whole, even a one-row one
    return build(23, [still(1), still(2, 7), (frames_with_gaps(40, {9: H0 + 5, 20: H0 + 6}), np.zeros(40)), swinging(30)], G=H0 + 5)


MANY_UNALIGNED_TRACKS = 310


def _many_unaligned():
    rng = np.random.default_rng(24)
    tracks = []
    for t in range(MANY_UNALIGNED_TRACKS):
        n = int(rng.integers(0, 11))
        f = int(rng.integers(0, 100)) + np.cumsum(rng.choice([1, 1, 1, 2, 3], n))
        tracks.append((f, np.zeros(n) if t % 3 else 30.0 * rng.integers(0, 2, n)))
    return build(24, tracks, H=5, R=2, G=2, E=1)


SPREAD_BACK = dict(i=10, e=34)


def _spread_back():
    # a still track whose frame numbers run 100 .. 110 and then start again at 50: row e = 34 (frame 73) ends the first whole
    # window of the second stretch and is held in stage B; it lies within H rows behind row i = 10 (frame 110), but BEFORE it in
    # frames, and must not spread to it
    f = np.concatenate([100 + np.arange(11), 50 + np.arange(45)])
    return build(25, [(f, np.zeros(len(f)))], **SPREAD_BACK)


BOUNDS = dict(ulp_row=30, ulp_bit=2, flip_row=50, flip_bit=5)


def _thresholds_at_bounds():
    # every joint of every row the identity, so that dot(k, i) = 3 exactly where rows are bit-equal.  dot_static = 3: one ulp
    # less in one element (row 30) is not still.  dot_move = 3: the same ulp is an event, and so is the way back.
    # dot_rapid = -1: a half turn (row 50, dot = -1 exactly) is not < -1 -- rapid never fires
    n = 80
    c = build(26, [still(n)])
    rot = np.tile(np.eye(3, dtype=np.float32), (n, 24, 1, 1))
    rot[BOUNDS["ulp_row"], activity_ref.JOINT_INDEX[BOUNDS["ulp_bit"]], 0, 0] = np.nextafter(np.float32(1.0), np.float32(0.0))
    rot[BOUNDS["flip_row"], activity_ref.JOINT_INDEX[BOUNDS["flip_bit"]]] = np.diag([1.0, -1.0, -1.0]).astype(np.float32)
    c.update(rotmat=rot, dot_static=3.0, dot_move=3.0, dot_rapid=-1.0)
    return c


SWEEP = 60


def sweep_problem(q):
    """Problem q of the seeded sweep: H in 1..110, R in 1..H, G in 1..5, E in 0..4, thresholds from random degrees, 1-3 tracks
    of 0..160 rows, wild frame numbers in a fifth of the tracks."""
    rng = np.random.default_rng(8000 + q)
    H = int(rng.integers(1, 111))
    R, G, E = int(rng.integers(1, H + 1)), int(rng.integers(1, 6)), int(rng.integers(0, 5))
    deg = (float(rng.uniform(2.0, 20.0)), float(rng.uniform(5.0, 40.0)), float(rng.uniform(20.0, 90.0)))
    tracks = []
    for _ in range(int(rng.integers(1, 4))):
        n = int(rng.integers(0 if tracks else 1, 161))               # (the first track has a row: N = 0 is the case `empty`)
        a = int(rng.integers(0, max(n, 1)))
        jumps = [(int(r), float(rng.uniform(-70.0, 70.0)), tuple(rng.choice(12, 3, replace=False))) for r in rng.integers(0, max(n, 1), 4)] if n else []
        th = walk(rng, n, still=[(a, min(a + int(rng.integers(1, 130)), n))], jumps=jumps, sd=float(rng.uniform(0.2, 4.0)))
        if rng.random() < 0.2:
            f = wild_frame_numbers(rng, n)
        else:
            f = int(rng.integers(0, 1000)) + np.cumsum(rng.choice([1, 1, 1, 1, 1, 1, 2, 3, G, G + 1, 7], n))
        tracks.append((f, th))
    return build(8000 + q, tracks, H=H, R=R, G=G, E=E, deg=deg)


def sweep_name(q):
    return f"sweep_{q}"


CASES = {"empty": _empty, "lengths": _lengths, "adjacent": _adjacent, "still_segment": _still_segment, "oscillation": _oscillation,
         "jump": _jump, "gaps": _gaps, "edges": _edges, "nan": _nan, "wild_frames": _wild_frames, "knife": _knife, "big": _big,
         "many_tracks": _many_tracks,
         **{f"lattice_H{H}_R{R}": _lattice(H, R) for H, R in LATTICE},
         "span_edge": _span_edge, "G_huge": _g_huge, "G_gt_H": _g_gt_h, "many_unaligned": _many_unaligned, "spread_back": _spread_back,
         "thresholds_at_bounds": _thresholds_at_bounds}
NAMES = list(CASES)
LATTICE_NAMES = [f"lattice_H{H}_R{R}" for H, R in LATTICE]
SWEEP_NAMES = [sweep_name(q) for q in range(SWEEP)]
PARAMS = ("H", "R", "G", "E", "dot_static", "dot_move", "dot_rapid")


@functools.lru_cache(maxsize=None)
def case(name):
    c = sweep_problem(int(name[6:])) if name.startswith("sweep_") else CASES[name]()
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
