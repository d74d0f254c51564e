"""Seeded cases for pr_smooth_tracks, shared by tests/test_smooth_cpu.py, tests/test_smooth_native.py and
tests/test_smooth_gpu.py, and the one comparison with tests/smooth_ref.py that the native and the GPU test apply.

A case is a dict: rotmat f32[N,24,3,3], betas f32[N,10] | None, cam f32[N,3] | None, frame_no i32[N], track_start i64[T+1], m,
sigma, and what the case plants: `isolated` (rows that must come back unchanged), `outlier` ((row, joint) or None),
`fallback` / `no_fallback` (lists of (row, joint)), `rotations` (every joint of every row is a rotation: False only where
non-finite values are planted).  Besides CASES there is a seeded sweep: `sweep_problem(q)` draws problem q, and case() /
reference() / check() take its name `sweep_<q>` like any other."""
import functools

import numpy as np

import smooth_ref

TILE = 32          # pr_smooth_tile_rows(); the GPU and the native test assert that it still is
NEAR_TIE = 1e-9    # relative gap between the best and the second-best cost under which an item may be left out
ROT_TOL = 2.0 ** -24


def rodrigues(aa):
    """axis-angle f64[...,3] -> rotation matrices f64[...,3,3]."""
    aa = np.asarray(aa, np.float64)
    th = np.linalg.norm(aa, axis=-1)[..., None, None]
    k = aa / np.maximum(np.linalg.norm(aa, axis=-1)[..., None], 1e-300)
    K = np.zeros(aa.shape[:-1] + (3, 3))
    K[..., 0, 1], K[..., 0, 2], K[..., 1, 0] = -k[..., 2], k[..., 1], k[..., 2]
    K[..., 1, 2], K[..., 2, 0], K[..., 2, 1] = -k[..., 0], -k[..., 1], k[..., 0]
    return np.eye(3) + np.sin(th) * K + (1.0 - np.cos(th)) * (K @ K)


def rot_z(deg):
    return rodrigues(np.array([0.0, 0.0, np.deg2rad(deg)]))


def jittery_track(rng, frames, jitter=0.03):
    """A slowly moving pose with per-frame jitter at the given frame numbers -> (rotmat f32[n,24,3,3], betas, cam)."""
    f = np.asarray(frames, np.float64)
    n = len(f)
    base = rng.uniform(-0.8, 0.8, (1, 24, 3))
    amp, phase = rng.uniform(0.0, 0.4, (1, 24, 3)), rng.uniform(0, 6.28, (1, 24, 3))
    aa = base + amp * np.sin(f[:, None, None] / 17.0 + phase) + rng.normal(0, jitter, (n, 24, 3))
    betas = (rng.normal(0, 1, (1, 10)) + rng.normal(0, 0.05, (n, 10))).astype(np.float32)
    cam = (np.array([[0.9, 0.0, 0.1]]) + rng.normal(0, 0.02, (n, 3))).astype(np.float32)
    return rodrigues(aa).astype(np.float32), betas, cam


def frames_with_gaps(n, gaps, start=0):
    """n frame numbers from `start`, consecutive except that row r is `gaps[r]` frames after row r - 1."""
    step = np.ones(n, np.int64)
    for r, g in gaps.items():
        step[r] = g
    step[0] = 0
    return start + np.cumsum(step)


def build(seed, tracks, m, sigma, with_betas=True, with_cam=True, **planted):
    """tracks: a list of frame-number arrays, one per track (an empty one is an empty track)."""
    rng = np.random.default_rng(seed)
    parts = [jittery_track(rng, f) for f in tracks]
    cat = lambda i, tail: np.concatenate([p[i] for p in parts]) if parts else np.zeros((0,) + tail, np.float32)
    case = dict(rotmat=cat(0, (24, 3, 3)), betas=cat(1, (10,)) if with_betas else None, cam=cat(2, (3,)) if with_cam else None,
                frame_no=np.concatenate([np.asarray(f, np.int64) for f in tracks]).astype(np.int32),
                track_start=np.cumsum([0] + [len(f) for f in tracks]).astype(np.int64), m=int(m), sigma=float(sigma),
                isolated=[], outlier=None, fallback=[], no_fallback=[], rotations=True)
    case.update(planted)
    return case


def _short(m, sigma):
    # tracks shorter than the window, every one starting at frame 0: neighbouring tracks' frame numbers overlap, so a window
    # that crossed a boundary would find members there
    return build(11, [np.arange(n) for n in (1, 2, 3, 2 * max(m, 1), 0, 7, 1)], m, sigma)


def _gaps(m, sigma):
    g = max(smooth_ref.gaussian_radius(sigma), 1)
    mm = max(m, 1)
    # gaps of 1 frame (a step of 2), of exactly m and g (the far side is just inside the window) and one more (just outside),
    # and of more than 15 on both sides of row 50: an isolated row
    gaps = {5: 2, 12: mm, 18: mm + 1, 26: g, 33: g + 1, 50: 20, 51: 17, 60: 2, 61: 2}
    return build(12, [frames_with_gaps(70, gaps, start=100), np.arange(95, 120)], m, sigma, with_cam=False,
                 isolated=[50])


def _tile(n):
    def make(m, sigma):
        if n == 2 * TILE + 1:      # a track boundary on the first tile edge, a gap on the second
            tracks = [np.arange(TILE), frames_with_gaps(TILE + 1, {TILE: 3}, start=7)]
        elif n == TILE + 1:        # a gap on the tile edge
            tracks = [frames_with_gaps(n, {TILE: 2})]
        else:
            tracks = [np.arange(n)]
        return build(20 + n, tracks, m, sigma, with_betas=(n % 2 == 0))
    return make


def _mixed(m, sigma):
    gaps = {9: 3, 40: 2, 41: 2, 77: 6}
    return build(13, [frames_with_gaps(90, gaps), np.arange(40, 75), np.arange(3), frames_with_gaps(31, {15: 16}, start=10)],
                 m, sigma)


def _outlier(m, sigma):
    case = build(14, [np.arange(40), np.arange(10, 30)], m, sigma, with_betas=False, with_cam=False)
    row, joint = 17, 3
    R = case["rotmat"][row, joint].astype(np.float64)
    case["rotmat"][row, joint] = (rodrigues(np.array([np.deg2rad(150.0), 0.0, 0.0])) @ R).astype(np.float32)
    case["outlier"] = (row, joint)
    return case


def _fallback(m, sigma):
    # a track of three rows at frames f - 1, f, f + 1: joint 5 turns 120, 0, 240 degrees about z (their weighted sum all but
    # loses its in-plane part: c comes to 2e-8), joint 7 turns -60, 0, 60 (c = 0.89: no fallback)
    case = build(15, [np.arange(30, 33), np.arange(25)], m, sigma, with_betas=False)
    for k, (far, near) in enumerate(((120.0, -60.0), (0.0, 0.0), (240.0, 60.0))):
        case["rotmat"][k, 5] = rot_z(far).astype(np.float32)
        case["rotmat"][k, 7] = rot_z(near).astype(np.float32)
    case["fallback"] = [(k, 5) for k in range(3)]
    case["no_fallback"] = [(k, 7) for k in range(3)]
    return case


I32_MIN, I32_MAX = np.iinfo(np.int32).min, np.iinfo(np.int32).max
WILD_TRACKS = (60, 45, 38)
WILD_TIE_ROW = sum(WILD_TRACKS) - 1


def wild_frame_numbers(rng, lengths):
    """Frame numbers that obey nothing, for tracks of these lengths: drawn from 0..39 (duplicates are certain), with a
    descending and a constant stretch in every track of 30 rows or more and both int32 extremes planted."""
    out = []
    for n in lengths:
        f = rng.integers(0, 40, n).astype(np.int64)
        if n >= 30:
            f[8:18] = np.sort(f[8:18])[::-1]
            f[20:28] = 7
            f[[3, n - 5]] = I32_MIN, I32_MAX
        out.append(f)
    return out


def _wild(m, sigma):
    # the header's "ANY frame_no content".  The last track ends ..., INT32_MAX, 5, 5: the last row's window holds the two rows
    # at frame 5 and nobody else, their costs are the same number and so are their frame distances -- the one way to the
    # second tie rule, "then to the smaller k"
    rng = np.random.default_rng(31)
    frames = wild_frame_numbers(rng, WILD_TRACKS)
    frames[2][-3:] = I32_MAX, 5, 5
    case = build(31, [np.arange(n) for n in WILD_TRACKS], m, sigma)
    case["frame_no"] = np.concatenate(frames).astype(np.int32)
    return case


MANY_TRACKS = 310
MANY_SEED = 36      # (seed 32's smallest cost gap at m = 15 was 1.7e-8, too near the 1e-9 census for comfort; this one's is 1.4e-5)


def _many(m, sigma):
    # more tracks than one launch carries, of 0..12 rows with gaps and starts of their own; the second launch starts at the
    # first row of track 256, which is no multiple of TILE (tests/test_smooth_cpu.py asserts it)
    rng = np.random.default_rng(MANY_SEED)
    tracks = []
    for _ in range(MANY_TRACKS):
        n = int(rng.integers(0, 13))
        steps = rng.choice([1, 1, 1, 2, 3, 6, 17], n)
        tracks.append(int(rng.integers(0, 1000)) + np.cumsum(steps) - (steps[0] if n else 0))
    return build(MANY_SEED, tracks, m, sigma)


THIRD = 1.0 / 3.0
# 3 * (1/3) and 3 * nextafter(1/3, 1) both round to 1.0 in float64 (each product lies halfway and goes to the even neighbour):
# radius 1.  The first sigma whose 3 sigma lies above 1 is two steps up: radius 2
SIGMAS = {"1e-200": 1e-200, "1e300": 1e300, "1e-3": 1e-3, "third": THIRD, "third_up": float(np.nextafter(THIRD, 1.0)),
          "third_up2": float(np.nextafter(np.nextafter(THIRD, 1.0), 1.0)), "1": 1.0, "1_up": float(np.nextafter(1.0, 2.0)),
          "4.999999999": 4.999999999, "5": 5.0}
SIGMA_GAP_ROW = 20


def _sigma(m, sigma):
    # a track with steps of 2, 3, 4, 15 and 16 frames, and one without.  Behind the step of 2 at SIGMA_GAP_ROW cam and betas
    # are a thousand times larger, so that even the weight exp(-18) of a radius-2 neighbour at sigma = 1/3 moves them by far
    # more than the tolerance: the radius decides.  Row 40 has 16 frames on either side: isolated at every radius
    gaps = {SIGMA_GAP_ROW: 2, 28: 3, 33: 4, 40: 16, 41: 16, 47: 15, 52: 2, 53: 2}
    case = build(33, [frames_with_gaps(60, gaps, start=50), np.arange(20)], m, sigma, isolated=[40])
    for key in ("cam", "betas"):
        case[key][SIGMA_GAP_ROW:30] *= np.float32(1000.0)
    if smooth_ref.gaussian_radius(sigma) < 2:
        case["isolated"].append(52)                    # two frames on either side
    return case


KNIFE_AXIS = np.array([0.3, -0.5, 0.8]) / np.linalg.norm([0.3, -0.5, 0.8])
KNIFE_JOINT, KNIFE_SIGMA = 9, 5.0


def _pair_c(theta_deg):
    """The reference's c of a two-row track's joint that turns by theta about KNIFE_AXIS between frames f and f + 1, row 0's."""
    R0, R1 = np.eye(3, dtype=np.float32), rodrigues(KNIFE_AXIS * np.deg2rad(theta_deg)).astype(np.float32)
    w = np.exp(-1.0 / (2.0 * KNIFE_SIGMA * KNIFE_SIGMA))
    return float(smooth_ref.fallback_measure(R0.astype(np.float64) + w * R1.astype(np.float64)))


@functools.lru_cache(maxsize=None)
def knife_theta():
    """theta* in degrees at which _pair_c crosses FALLBACK_C (c falls as theta grows), by bisection: about 168.631."""
    lo, hi = 150.0, 179.0
    assert _pair_c(lo) > smooth_ref.FALLBACK_C > _pair_c(hi)
    for _ in range(60):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _pair_c(mid) > smooth_ref.FALLBACK_C else (lo, mid)
    return 0.5 * (lo + hi)


def _knife_c(offset_deg):
    def make(m, sigma):
        assert sigma == KNIFE_SIGMA and m == 0
        case = build(34, [np.arange(2), np.arange(9)], m, sigma, with_betas=False)
        case["rotmat"][0, KNIFE_JOINT] = np.eye(3, dtype=np.float32)
        case["rotmat"][1, KNIFE_JOINT] = rodrigues(KNIFE_AXIS * np.deg2rad(knife_theta() + offset_deg)).astype(np.float32)
        case["fallback" if offset_deg > 0 else "no_fallback"] = [(0, KNIFE_JOINT), (1, KNIFE_JOINT)]
        return case
    return make


NEWTON_SIGMA = 50.0
NEWTON_AXES = np.array([[0.3, -0.5, 0.8], [-0.7, 0.2, 0.4]])


def _newton_rows(theta_deg):
    ax = NEWTON_AXES / np.linalg.norm(NEWTON_AXES, axis=1, keepdims=True)
    return np.stack([rodrigues(ax[0] * np.deg2rad(theta_deg)), np.eye(3), rodrigues(ax[1] * np.deg2rad(theta_deg))]).astype(np.float32)


def _newton_c(theta_deg):
    w = np.exp(-1.0 / (2.0 * NEWTON_SIGMA * NEWTON_SIGMA))
    Y = _newton_rows(theta_deg).astype(np.float64)
    return float(smooth_ref.fallback_measure(w * Y[0] + Y[1] + w * Y[2]))


def _knife_c_newton(m, sigma):
    # three members about different axes whose sum all but cancels: c = 0.055 in the middle row, the ill-conditioned end of
    # what the scaled Newton iteration is given
    assert sigma == NEWTON_SIGMA and m == 0
    thetas = np.arange(90.0, 180.0, 0.25)
    cs = np.array([_newton_c(t) for t in thetas])
    first = int(np.argmax(cs < 0.055))
    assert first > 0 and cs[first - 1] >= 0.055 > cs[first]
    lo, hi = thetas[first - 1], thetas[first]
    for _ in range(50):
        mid = 0.5 * (lo + hi)
        lo, hi = (mid, hi) if _newton_c(mid) >= 0.055 else (lo, mid)
    case = build(35, [np.arange(3), np.arange(9)], m, sigma, with_betas=False)
    case["rotmat"][:3, KNIFE_JOINT] = _newton_rows(lo)
    case["no_fallback"] = [(k, KNIFE_JOINT) for k in range(3)]
    return case


NONFINITE = dict(element=(5, 7, 1, 2), joint=(104, 3), cam=(50, 1), rows=(19, 39, 65, 85))


def _nonfinite(m, sigma):
    # three tracks of 40, 45 and 30 rows (from rows 0, 40 and 85); the first two have a gap of 20 frames, wider than any
    # radius, before rows 20 and 65.  Whole NaN rows: 19 (the last before track 0's gap), 39 (the last of track 0), 65 (the
    # first behind track 1's gap) and 85 (the first of track 2): each lies directly on ONE side of a gap or a boundary; the
    # rows on the other side are finite and must stay so.  Neighbouring tracks' frame numbers overlap
    tracks = [frames_with_gaps(40, {20: 20}), frames_with_gaps(45, {25: 20}, start=3), np.arange(10, 40)]
    case = build(36, tracks, m, sigma, rotations=False)
    r, j, a, b = NONFINITE["element"]
    case["rotmat"][r, j, a, b] = np.nan
    r, j = NONFINITE["joint"]
    case["rotmat"][r, j] = np.nan
    r, e = NONFINITE["cam"]
    case["cam"][r, e] = np.inf
    for r in NONFINITE["rows"]:
        for key in ("rotmat", "betas", "cam"):
            case[key][r] = np.nan
    return case


def nonfinite_clean_rows(case):
    """-> bool[N]: the rows that no window of radius max(m, g) connects with a planted non-finite value, in either stage: their
    outputs must be finite and their status 0."""
    N = len(case["frame_no"])
    lo, hi = smooth_ref.track_bounds(case["track_start"], N)
    bad = np.zeros(N, bool)
    for key in ("rotmat", "betas", "cam"):
        bad |= ~np.isfinite(case[key].reshape(N, -1)).all(1)
    for r in (case["m"], smooth_ref.gaussian_radius(case["sigma"])):           # stage 1 spreads it by m, stage 2 by g more
        kc, mem, _ = smooth_ref.members(case["frame_no"], lo, hi, r)
        bad = (mem & bad[kc]).any(1)
    return ~bad


SWEEP = 60
SWEEP_RESEEDED = {}     # problem -> the seed that replaced its own, where that one's census exceeded the cap (none did)


def sweep_problem(q):
    """Problem q of the seeded sweep: m in 0..15, sigma in {0} or (0, 6], betas and cam present or absent, 1-4 tracks of 0..80
    rows with gaps, wild frame numbers in a fifth of the tracks."""
    seed = SWEEP_RESEEDED.get(q, 7000 + q)
    rng = np.random.default_rng(seed)
    m = 0 if rng.random() < 0.15 else int(rng.integers(0, 16))      # (m = 0, stage 2 alone, more often than one in 16)
    sigma = 0.0 if rng.random() < 0.25 else float(6.0 * (1.0 - rng.random()))
    with_betas, with_cam = bool(rng.integers(0, 2)), bool(rng.integers(0, 2))
    tracks = []
    for _ in range(int(rng.integers(1, 5))):
        n = int(rng.integers(0 if tracks else 1, 81))                # (the first track has a row: N = 0 is the callers' early return)
        if rng.random() < 0.2:
            tracks.append(wild_frame_numbers(rng, [n])[0])
        else:
            steps = rng.choice([1, 1, 1, 1, 2, 3, 5, 16, 40], n)
            tracks.append(int(rng.integers(0, 500)) + np.cumsum(steps))
    return build(seed, tracks, m, sigma, with_betas=with_betas, with_cam=with_cam)


def sweep_name(q):
    return f"sweep_{q}"


# name -> (maker, m, sigma)
CASES = {
    "short_m2_s1.5": (_short, 2, 1.5),
    "short_m15_s5": (_short, 15, 5.0),
    "gaps_m2_s1.5": (_gaps, 2, 1.5),
    "gaps_m3_s0": (_gaps, 3, 0.0),
    "tile-1": (_tile(TILE - 1), 2, 1.5),
    "tile": (_tile(TILE), 2, 1.5),
    "tile+1": (_tile(TILE + 1), 2, 1.5),
    "2tile+1": (_tile(2 * TILE + 1), 2, 1.5),
    "2tile+1_m15_s5": (_tile(2 * TILE + 1), 15, 5.0),
    "mixed_m0_s1.5": (_mixed, 0, 1.5),
    "mixed_m2_s0": (_mixed, 2, 0.0),
    "mixed_m0_s0": (_mixed, 0, 0.0),
    "mixed_m15_s5": (_mixed, 15, 5.0),
    "mixed_m2_s1.5": (_mixed, 2, 1.5),
    "outlier_m1_s0": (_outlier, 1, 0.0),
    "outlier_m2_s1.5": (_outlier, 2, 1.5),
    "fallback_m0_s50": (_fallback, 0, 50.0),      # (with m >= 1 the three equidistant rotations would be a planted near-tie)
    "wild_m2_s1.5": (_wild, 2, 1.5),
    "wild_m15_s5": (_wild, 15, 5.0),
    "wild_m3_s0": (_wild, 3, 0.0),
    "wild_m0_s2": (_wild, 0, 2.0),
    "many_m2_s1.5": (_many, 2, 1.5),
    "many_m15_s5": (_many, 15, 5.0),
    **{f"sigma_{label}": (_sigma, 0, value) for label, value in SIGMAS.items()},
    "knife_c_below": (_knife_c(+1e-4), 0, KNIFE_SIGMA),      # theta* + 1e-4 degrees: c just below 0.05, the joint falls back
    "knife_c_above": (_knife_c(-1e-4), 0, KNIFE_SIGMA),
    "knife_c_newton": (_knife_c_newton, 0, NEWTON_SIGMA),
    "nonfinite_m2_s0": (_nonfinite, 2, 0.0),
    "nonfinite_m0_s1.5": (_nonfinite, 0, 1.5),
    "nonfinite_m2_s1.5": (_nonfinite, 2, 1.5),
}
NAMES = list(CASES)
SWEEP_NAMES = [sweep_name(q) for q in range(SWEEP)]


@functools.lru_cache(maxsize=None)
def case(name):
    if name.startswith("sweep_"):
        c = sweep_problem(int(name[6:]))
    else:
        maker, m, sigma = CASES[name]
        c = maker(m, sigma)
    c["name"] = name
    return c


@functools.lru_cache(maxsize=None)
def reference(name):
    """The float64 reference of a case, computed once a process and shared; nobody writes into it."""
    c = case(name)
    ref = smooth_ref.smooth(c["rotmat"], c["frame_no"], c["track_start"], c["m"], c["sigma"], c["betas"], c["cam"])
    for v in (ref["rotmat"], ref["betas"], ref["cam"], ref["status"], ref["replaced"]):
        if v is not None:
            v.setflags(write=False)
    return ref


def near_ties(ref):
    """-> {tensor: bool[N,G]} of the stage-1 items whose best and second-best costs differ by less than NEAR_TIE relative
    without being bit-equal, and the number of items."""
    out, items = {}, 0
    for name, (c1, c2, _, _) in ref["ties"].items():
        with np.errstate(invalid="ignore"):
            out[name] = np.isfinite(c2) & (c1 != c2) & ((c2 - c1) < NEAR_TIE * np.abs(c2))
        items += c1.size
    return out, items


def smallest_gap(ref):
    """The smallest relative gap between a best and a distinct second-best cost over the case's stage-1 items (inf without any)."""
    gap = np.inf
    for c1, c2, _, _ in ref["ties"].values():
        ok = np.isfinite(c2) & (c1 != c2)
        if ok.any():
            gap = min(gap, float(np.min((c2[ok] - c1[ok]) / np.abs(c2[ok]))))
    return gap


def bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.int32)


def check(name, got):
    """`got`: dict(rotmat, betas, cam, status, replaced) of numpy arrays as the kernel wrote them -- against reference(name) by
    the contract's tolerances.  Asserts; returns the largest rotation error seen (0 where stage 2 did not run)."""
    c, ref = case(name), reference(name)
    N = len(c["frame_no"])
    near, items = near_ties(ref)
    n_near = sum(int(v.sum()) for v in near.values())
    assert n_near <= 0.001 * max(items, 1), f"{name}: {n_near} near-ties among {items} items"
    if n_near == 0:
        np.testing.assert_array_equal(got["replaced"], ref["replaced"], err_msg=f"{name}: replaced")
    np.testing.assert_array_equal(got["status"], ref["status"], err_msg=f"{name}: status")
    worst = 0.0
    for key, G in (("rotmat", 24), ("cam", 1), ("betas", 1)):
        if c[key] is None:
            assert got.get(key) is None
            continue
        x, r = np.asarray(got[key]).reshape(N, G, -1), np.asarray(ref[key]).reshape(N, G, -1)
        if c["sigma"] == 0:
            same = (bits(x) == bits(r)).all(-1)
            if n_near and key in near:
                _, _, second, _ = ref["ties"][key]
                alt = np.take_along_axis(c[key].reshape(N, G, -1), np.clip(second, 0, N - 1)[:, :, None], axis=0)
                same |= near[key] & (bits(x) == bits(alt)).all(-1)
            assert same.all(), f"{name}: {key} differs in bits at (row, group) {np.argwhere(~same)[:5].tolist()}"
            continue
        assert n_near == 0, f"{name}: the committed seeds have no near-tie (tests/test_smooth_cpu.py asserts it)"
        xd = x.astype(np.float64)
        with np.errstate(invalid="ignore"):
            err = np.abs(xd - r)
        same = (np.isnan(xd) & np.isnan(r)) | (xd == r)        # NaNs compare as equal (and equal infinities are equal)
        err = np.where(same, 0.0, err)                         # elsewhere a NaN or an inf on one side fails what follows
        if key == "rotmat":
            worst = float(err.max()) if err.size else 0.0
            assert (err <= ROT_TOL).all(), f"{name}: rotation entry off by {err.max():.3e} > 2^-24"
        else:
            y = np.abs(ref["stage1"][key])
            ymax = float(y[np.isfinite(y)].max()) if np.isfinite(y).any() else 0.0
            tol = np.where(np.isfinite(r), ROT_TOL * np.abs(r) + 1e-13 * ymax, 0.0)
            assert (err <= tol).all(), f"{name}: {key} off by {err.max():.3e}"
    # what the case plants
    for row in c["isolated"]:
        for key in ("rotmat", "cam", "betas"):
            if c[key] is not None:
                assert np.array_equal(bits(got[key][row]), bits(c[key][row])), f"{name}: isolated row {row} changed ({key})"
        assert got["status"][row] == 0 and got["replaced"][row] == 0
    if c["outlier"] is not None and c["m"] >= 1:
        row, j = c["outlier"]
        assert got["replaced"][row] >> j & 1, f"{name}: the planted outlier survived stage 1"
        if c["sigma"] == 0:
            mine = bits(got["rotmat"][row, j])
            assert any(np.array_equal(mine, bits(c["rotmat"][k, j])) for k in (row - 1, row + 1)), \
                f"{name}: the outlier's replacement is no neighbour's bits"
    for row, j in c["fallback"]:
        assert got["status"][row] >> j & 1, f"{name}: row {row} joint {j} did not fall back"
        assert np.array_equal(bits(got["rotmat"][row, j]), bits(ref["stage1"]["rotmat"][row, j]))
    for row, j in c["no_fallback"]:
        assert not got["status"][row] >> j & 1, f"{name}: row {row} joint {j} fell back"
    return worst


def write_case(path, name):
    """The file tests/native/smooth_host.cc reads: int32 N T m has_betas has_cam 0, f64 sigma, then track_start i32[T+1],
    frame_no i32[N], rotmat, betas, cam."""
    c = case(name)
    N, T = len(c["frame_no"]), len(c["track_start"]) - 1
    with open(path, "wb") as f:
        f.write(np.array([N, T, c["m"], c["betas"] is not None, c["cam"] is not None, 0], np.int32).tobytes())
        f.write(np.float64(c["sigma"]).tobytes())
        f.write(c["track_start"].astype(np.int32).tobytes() + c["frame_no"].tobytes() + c["rotmat"].tobytes())
        for key in ("betas", "cam"):
            if c[key] is not None:
                f.write(c[key].tobytes())
    return path


def read_outputs(path, name):
    """What the driver wrote: rotmat, betas, cam, status, replaced."""
    c = case(name)
    N = len(c["frame_no"])
    raw, pos = np.fromfile(path, np.uint8), 0
    got = {}
    for key, shape, dt in (("rotmat", (N, 24, 3, 3), np.float32), ("betas", (N, 10), np.float32), ("cam", (N, 3), np.float32),
                           ("status", (N,), np.int32), ("replaced", (N,), np.int32)):
        if key in ("betas", "cam") and c[key] is None:
            got[key] = None
            continue
        n = int(np.prod(shape)) * 4
        got[key] = raw[pos:pos + n].view(dt).reshape(shape)
        pos += n
    assert pos == raw.size
    return got
