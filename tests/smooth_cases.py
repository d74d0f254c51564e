"""Seeded cases for pr_smooth_tracks, shared by tests/test_smooth_cpu.py, tests/test_smooth_native.py and
tests/test_smooth_gpu.py, and the one comparison with tests/smooth_ref.py that the native and the GPU test apply.

A case is a dict: rotmat f32[N,24,3,3], betas f32[N,10] | None, cam f32[N,3] | None, frame_no i32[N], track_start i64[T+1], m,
sigma, and what the case plants: `isolated` (rows that must come back unchanged), `outlier` ((row, joint) or None),
`fallback` / `no_fallback` (lists of (row, joint))."""
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
                isolated=[], outlier=None, fallback=[], no_fallback=[])
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
}
NAMES = list(CASES)


@functools.lru_cache(maxsize=None)
def case(name):
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
        err = np.abs(x.astype(np.float64) - r)
        if key == "rotmat":
            worst = float(err.max()) if err.size else 0.0
            assert (err <= ROT_TOL).all(), f"{name}: rotation entry off by {err.max():.3e} > 2^-24"
        else:
            ymax = float(np.abs(ref["stage1"][key]).max()) if N else 0.0
            tol = ROT_TOL * np.abs(r) + 1e-13 * ymax
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
