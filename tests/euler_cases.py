"""Inputs on the edges of the Euler stage (pose_to_euler_kernel, csrc/frame_kernels.hip), the oracle's view of them, and the
per-angle criterion the GPU file holds the kernel to.

Everything is seeded numpy, float32 axis-angle [N, 24, 3], with one label per joint:

  gimbal     Rz(yaw) Ry(+-pi/2 + eps) Rx(roll) in float64 -> rodrigues_cv.rotmat_to_rotvec -> float32.  sy = sqrt(R00^2 + R10^2)
             is |eps| up to the ~1e-7 the float32 rounding of the vector moves the rotation by, so |eps| <= 9e-7 lands in the
             reference's gimbal-lock branch (sy < 1e-6) and |eps| >= 1.1e-6 does not.  Two further |eps| (GIMBAL_NEAR) are
             drawn again until sy lies in a window next to the threshold; every joint is drawn again while sy is within twice
             LOCK_MARGIN of it.  Plus the closed-form vectors (0, +-fl32(pi/2), 0) and +-fl32(2 pi / (3 sqrt 3)) (1, 1, 1) in
             all eight sign patterns: turns by 120 degrees about a cube diagonal, the ones that map x onto +-z are locks in
             which yaw and roll mix into ex.  And ORDER_PER_VARIANT joints just outside the lock for each other order of
             Rodrigues' double operations (ORDER_VARIANTS), kept when that order moves one of their angles: there ex and ez
             are quotients of entries that cancelled from 0.3 to 1e-6, so the last ulp of a double decides a float32
             rounding about once in 600 entries.  The same rotations are there as float32 matrices.
  tiny       theta from 1e-20 to 1e-6 about +-x, +-y, +-z and random axes, on both sides of rodrigues_vec2mat's
             `theta < DBL_EPSILON` cut (the float32 neighbours of 2^-52 about the coordinate axes; 2^-52 (1 -+ 2^-20) about
             random ones, where the float32 rounding of the components moves theta by 6e-8 relative).
  large      theta around 2 pi and up to 1e30, and (3e38, 3e38, 3e38).
  nonfinite  a finite base batch and plants (frame, joint, component, value) placed for the kernel's workgroup geometry: 24
             joint threads OR into one of 8 per-frame flags in LDS, and status[8 block + t] is written after the barrier.

`detail` is the oracle taken apart (the float32 matrix, sy, the branch, the isRotationMatrix norm, the round-trip sum), in
coord_ref's own operations; tests/test_euler_edges_cpu.py holds it to coord_ref.axis_angle_to_euler_angle bit for bit.
"""
import math

import numpy as np

from oracle import coord_ref, rodrigues_cv

LOCK = 1e-6                       # coord_utils.py:73, `if sy < 1e-6`
LOCK_MARGIN = 1e-4                # no gimbal joint's sy within this (relative) of LOCK; see test_euler_edges_cpu.py
DBL_EPS = float(np.finfo(np.float64).eps)
PI_2_F32 = np.float32(np.pi / 2)
DIAG_F32 = np.float32(2 * np.pi / (3 * math.sqrt(3.0)))

GIMBAL_EPS = (0.0, 2e-7, -2e-7, 5e-7, -5e-7, 9e-7, -9e-7, 1.1e-6, -1.1e-6, 2e-6, -2e-6, 1e-5, -1e-5, 1e-3, -1e-3)
# |eps| -> the window sy is drawn into: just below and just above the threshold (a threshold moved by 5 % crosses them)
GIMBAL_NEAR = {9.7e-7: (0.955e-6, 0.9995e-6), 1.03e-6: (1.0005e-6, 1.045e-6)}
GIMBAL_FRAMES = 16
GIMBAL_SEED = 20263
MAX_DRAWS = 400

TINY_THETAS = (("1e-20", 1e-20), ("below_cut", None), ("at_cut", None), ("above_cut", None), ("1e-15", 1e-15),
               ("1e-12", 1e-12), ("1e-10", 1e-10), ("1e-8", 1e-8), ("1e-6", 1e-6))
TINY_RANDOM_AXES = 10
TINY_SEED = 20264

LARGE_THETAS = (("2pi-ulp", None), ("2pi", None), ("2pi+ulp", None), ("10", 10.0), ("1e2", 1e2), ("1e4", 1e4), ("1e6", 1e6),
                ("1e12", 1e12), ("1e30", 1e30))
LARGE_RANDOM_AXES = 17
LARGE_SEED = 20265

NONFINITE_N = (1, 7, 8, 9, 17)
NONFINITE_SEED = 20266
NAN_PAYLOAD = np.array([0x7FC12345], np.uint32).view(np.float32)[0]
NONFINITE_VALUES = (np.float32(np.nan), np.float32(np.inf), np.float32(-np.inf), NAN_PAYLOAD)


# ---------------------------------------------------------------------------------------------------------------------
# the oracle, taken apart
# ---------------------------------------------------------------------------------------------------------------------
def detail(aa):
    """float32 axis-angle [..., 3] -> per joint (flattened, n joints), every number formed as oracle/coord_ref.py forms it:
    R f32[n,3,3]; norm: isRotationMatrix's float32 Frobenius norm; raises: where axis_angle_to_euler_angle would raise; and,
    where it does not, sy (the float64 root of the float32 sum), lock (sy < 1e-6), dsum (the signed round-trip sum) and
    euler f64[n,3] in degrees."""
    flat = np.ascontiguousarray(aa, np.float32).reshape(-1, 3)
    n = len(flat)
    out = dict(R=np.empty((n, 3, 3), np.float32), norm=np.empty(n), raises=np.zeros(n, bool), sy=np.full(n, np.nan),
               lock=np.zeros(n, bool), dsum=np.full(n, np.nan), euler=np.full((n, 3), np.nan))
    with np.errstate(invalid="ignore"):                            # cos(inf) for the planted infinities
        for k, rv in enumerate(flat):
            R = rodrigues_cv.rotvec_to_rotmat(rv)
            out["R"][k] = R
            out["norm"][k] = np.linalg.norm(np.identity(3, dtype=R.dtype) - np.dot(R.T, R))
            if not coord_ref.is_rotation_matrix(R):
                out["raises"][k] = True
                continue
            sy = math.sqrt(R[0, 0] * R[0, 0] + R[1, 0] * R[1, 0])
            e = coord_ref.rotation_matrix_to_euler(R)
            dsum = (R - coord_ref.euler_to_rotmat(e[2], e[1], e[0])).sum()
            out["sy"][k], out["lock"][k], out["dsum"][k] = sy, sy < LOCK, dsum
            out["raises"][k] = dsum > 0.1
            out["euler"][k] = e * 180 / math.pi
    return out


def oracle_euler(aa):
    """coord_ref.axis_angle_to_euler_angle frame by frame: f32[N,24,3] -> f64[N,24,3] degrees (raises where it raises)."""
    with np.errstate(invalid="ignore"):
        return np.stack([coord_ref.axis_angle_to_euler_angle(f) for f in np.asarray(aa, np.float32)])


# ---------------------------------------------------------------------------------------------------------------------
# the per-angle criterion
# ---------------------------------------------------------------------------------------------------------------------
def _ulp32(x):
    return np.spacing(np.abs(np.asarray(x, np.float32))).astype(np.float64)


def _sy_of(r00, r10):
    """sy as coord_ref.rotation_matrix_to_euler forms it: float32 products and sum, float64 root."""
    r00, r10 = np.asarray(r00, np.float32), np.asarray(r10, np.float32)
    return np.sqrt((r00 * r00 + r10 * r10).astype(np.float64))


def flip_allowance(R):
    """How far one float32 ulp in the arguments of each angle's atan2(a, b) can move it, in degrees: f32[n,3,3] -> f64[n,3].

    Kernel and oracle do the same double operations on the same float32 matrix, but the matrix comes out of cos / sin / sqrt
    of two libms and two orders of double roundings, which can differ in the last double ulp; where that straddles a float32
    rounding boundary an entry comes out as its float32 neighbour.  d atan2(a, b) = (b da - a db) / (a^2 + b^2), so the
    bound is (|b| ulp32(a) + |a| ulp32(b)) / (a^2 + b^2), times 1 + 1e-6 for the second order (da / hypot(a, b) is at most
    a float32 ulp, 1.2e-7, relative).  That is never more than (ulp32(a) + ulp32(b)) / hypot(a, b), and much less where one
    argument dwarfs the other: for a rotation of 1e-12 about x, ex = atan2(1e-12, 1) may move by ulp32(1e-12), not ulp32(1).
    ey = atan2(-R20, sy): sy is not an entry, the flip is in R00 and R10 under it, and what it does to sy is evaluated (all
    nine combinations of -1, 0, +1 ulp), not estimated.  In the lock ez is the constant 0 and has no allowance."""
    R = np.asarray(R, np.float32)
    r00, r10, r20 = R[:, 0, 0], R[:, 1, 0], R[:, 2, 0]
    sy = _sy_of(r00, r10)
    lock = sy < LOCK
    ax = np.where(lock, -R[:, 1, 2], R[:, 2, 1]).astype(np.float32)
    bx = np.where(lock, R[:, 1, 1], R[:, 2, 2]).astype(np.float32)
    up, down = np.float32(np.inf), np.float32(-np.inf)
    dsy = np.zeros(len(R))
    for p in (r00, np.nextafter(r00, up), np.nextafter(r00, down)):
        for q in (r10, np.nextafter(r10, up), np.nextafter(r10, down)):
            dsy = np.maximum(dsy, np.abs(_sy_of(p, q) - sy))
    tiny = 1e-300

    def bound(a, b, da, db):
        a, b = np.abs(np.asarray(a, np.float64)), np.abs(np.asarray(b, np.float64))
        return np.degrees((b * da + a * db) / np.maximum(a * a + b * b, tiny) * (1 + 1e-6))
    ex = bound(ax, bx, _ulp32(ax), _ulp32(bx))
    ey = bound(r20, sy, _ulp32(r20), dsy)
    ez = np.where(lock, 0.0, bound(r10, r00, _ulp32(r10), _ulp32(r00)))
    return np.stack([ex, ey, ez], axis=1)


def compare(got, want, R, absolute=1e-9):
    """The criterion of tests/test_euler_edges_gpu.py on n joints: got, want f64[n,3] degrees, R the oracle's f32[n,3,3].
    -> (d, tight, flipped, bad): d the difference modulo 360; tight: d <= max(`absolute` degrees, 1e-12 |want|), what
    identical double operations on an identical matrix give with room for two libms' last ulps (absolute = 0 for the tiny
    family, whose angles lie below 1e-9 degrees: the relative part alone); flipped: not tight, but within flip_allowance;
    bad: neither (a NaN is bad)."""
    got, want = np.asarray(got, np.float64).reshape(-1, 3), np.asarray(want, np.float64).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        d = np.abs(got - want)
        d = np.minimum(d, np.abs(360 - d))
        tight = d <= np.maximum(absolute, 1e-12 * np.abs(want))
        flipped = ~tight & (d <= flip_allowance(R))
    return d, tight, flipped, ~(tight | flipped)


FLIP_SHARE = 1e-3                 # at most this share of a family's angles may need the flip allowance


# ---------------------------------------------------------------------------------------------------------------------
# Rodrigues' formula in another order of its double operations
# ---------------------------------------------------------------------------------------------------------------------
if hasattr(math, "fma"):
    fma = math.fma
else:
    def fma(a, b, c):
        """a * b + c rounded once (finite arguments)."""
        from fractions import Fraction
        return float(Fraction(a) * Fraction(b) + Fraction(c))


def rodrigues_in_order(v, r_first=True, fused=False):
    """rodrigues_cv.rotvec_to_rotmat's float32 matrix of one float32 vector (theta >= DBL_EPSILON) in Python floats.  The
    defaults are its order, OpenCV's: c I + c1 (r r^T) + s [r]x, the products of r's components first, every operation
    rounded on its own.  r_first = False takes c1 rx before the second component; fused rounds the last product and the sum
    of each entry once, as a contracting compiler does."""
    x, y, z = (float(c) for c in np.asarray(v, np.float32))
    theta = math.sqrt(x * x + y * y + z * z)
    c, s = math.cos(theta), math.sin(theta)
    c1, it = 1.0 - c, 1.0 / theta
    x, y, z = x * it, y * it, z * it
    mad = fma if fused else (lambda p, q, r: p * q + r)

    def entry(a, b, add):
        return mad(c1, a * b, add) if r_first else mad(c1 * a, b, add)
    return np.array([entry(x, x, c), entry(x, y, -(s * z)), entry(x, z, s * y), entry(x, y, s * z), entry(y, y, c),
                     entry(y, z, -(s * x)), entry(x, z, -(s * y)), entry(y, z, s * x), entry(z, z, c)]).astype(np.float32).reshape(3, 3)


# name -> the order: pose_to_euler_kernel had the first (`c1 * rx * ry - s * rz` under -ffp-contract=fast)
ORDER_VARIANTS = (("c1rx_first_and_fused", dict(r_first=False, fused=True)), ("c1rx_first", dict(r_first=False)),
                  ("fused", dict(fused=True)))
ORDER_PER_VARIANT = 4
ORDER_MAX_DRAWS = 20000


# ---------------------------------------------------------------------------------------------------------------------
# gimbal
# ---------------------------------------------------------------------------------------------------------------------
def _pad(vectors, labels, mats=None):
    """-> f32[N,24,3], labels[N,24] (and f32[N,24,3,3]), padded to whole frames with the zero rotation."""
    n = -len(vectors) % 24
    aa = np.array(list(vectors) + [(0.0, 0.0, 0.0)] * n, np.float32).reshape(-1, 24, 3)
    lab = np.array(list(labels) + ["pad_zero"] * n, dtype=object).reshape(-1, 24)
    if mats is None:
        return aa, lab
    return aa, lab, np.array(list(mats) + [np.eye(3)] * n, np.float64).astype(np.float32).reshape(-1, 24, 3, 3)


_CACHE = {}


def gimbal():
    """-> (aa f32[16,24,3], labels[16,24], rotmat f32[16,24,3,3]: the same rotations, the float64 matrix rounded to float32)."""
    if "gimbal" in _CACHE:
        return _CACHE["gimbal"]
    vectors, labels, mats = [], [], []
    for s in (1.0, -1.0):
        vectors.append((0.0, s * float(PI_2_F32), 0.0))
        labels.append(f"exact_y{'+' if s > 0 else '-'}")
        mats.append(coord_ref.euler_to_rotmat(0.0, s * math.pi / 2, 0.0))
    for sx in (1.0, -1.0):
        for sy in (1.0, -1.0):
            for sz in (1.0, -1.0):
                vectors.append((sx * float(DIAG_F32), sy * float(DIAG_F32), sz * float(DIAG_F32)))
                labels.append("diagonal" + "".join("+" if v > 0 else "-" for v in (sx, sy, sz)))
                mats.append(rodrigues_cv.rotvec_to_rotmat(np.array([sx, sy, sz]) * (2 * np.pi / (3 * math.sqrt(3.0)))))
    # joints that tell the order of Rodrigues' double operations: just outside the lock ex and ez are quotients of entries
    # that cancelled to 1e-6, and a joint is kept when the variant's matrix moves one of its angles
    for vi, (name, kw) in enumerate(ORDER_VARIANTS):
        rng = np.random.default_rng([GIMBAL_SEED, vi])
        kept = 0
        for _ in range(ORDER_MAX_DRAWS):
            yaw, roll = rng.uniform(-3.0, 3.0, 2)
            eps, s = rng.uniform(1.1e-6, 3e-6) * rng.choice((-1.0, 1.0)), rng.choice((-1.0, 1.0))
            R = coord_ref.euler_to_rotmat(yaw, s * (math.pi / 2) + eps, roll)
            v = rodrigues_cv.rotmat_to_rotvec(R).astype(np.float32)
            d = detail(v)
            other = rodrigues_in_order(v, **kw)
            if d["lock"][0] or abs(d["sy"][0] / LOCK - 1.0) <= 2 * LOCK_MARGIN or np.array_equal(other, d["R"][0]):
                continue
            moved = coord_ref.rotation_matrix_to_euler(other) * 180 / math.pi
            if not compare(moved[None], d["euler"], d["R"])[2].any():
                continue
            vectors.append(tuple(float(c) for c in v))
            labels.append(f"order:{name}:{kept}")
            mats.append(R)
            kept += 1
            if kept == ORDER_PER_VARIANT:
                break
        else:
            raise AssertionError(("no joints for", name))
    combos = [(eps, s) for eps in GIMBAL_EPS + tuple(v * g for v in GIMBAL_NEAR for g in (1.0, -1.0)) for s in (1.0, -1.0)]
    rng = np.random.default_rng(GIMBAL_SEED)
    k = 0
    while len(vectors) < GIMBAL_FRAMES * 24:
        eps, s = combos[k % len(combos)]
        k += 1
        window = GIMBAL_NEAR.get(abs(eps), None)
        for _ in range(MAX_DRAWS):
            yaw, roll = rng.uniform(-3.0, 3.0, 2)
            R = coord_ref.euler_to_rotmat(yaw, s * (math.pi / 2) + eps, roll)
            v = rodrigues_cv.rotmat_to_rotvec(R).astype(np.float32)
            sy = float(detail(v)["sy"][0])
            if abs(sy / LOCK - 1.0) <= 2 * LOCK_MARGIN:
                continue
            if window is None or window[0] < sy < window[1]:
                break
        else:
            raise AssertionError(("no draw for", eps, s))
        vectors.append(tuple(float(c) for c in v))
        labels.append(f"eps={eps:+.3g},pitch={'+' if s > 0 else '-'}pi/2")
        mats.append(R)
    _CACHE["gimbal"] = _pad(vectors, labels, mats)
    return _CACHE["gimbal"]


# ---------------------------------------------------------------------------------------------------------------------
# tiny and large
# ---------------------------------------------------------------------------------------------------------------------
def _unit_axes(rng, n):
    u = rng.standard_normal((n, 3))
    return u / np.linalg.norm(u, axis=1, keepdims=True)


def tiny():
    """-> (aa f32[N,24,3], labels[N,24])."""
    if "tiny" in _CACHE:
        return _CACHE["tiny"]
    cut = np.float32(DBL_EPS)                                      # 2^-52 is a float32
    near = {"below_cut": (np.nextafter(cut, np.float32(0)), DBL_EPS * (1 - 2.0 ** -20)), "at_cut": (cut, None),
            "above_cut": (np.nextafter(cut, np.float32(1)), DBL_EPS * (1 + 2.0 ** -20))}
    rng = np.random.default_rng(TINY_SEED)
    vectors, labels = [], []
    for name, theta in TINY_THETAS:
        on_axis, off_axis = near[name] if theta is None else (np.float32(theta), theta)
        for axis in range(3):
            for s in (1.0, -1.0):
                v = [0.0, 0.0, 0.0]
                v[axis] = s * float(on_axis)
                vectors.append(tuple(v))
                labels.append(f"{name},{'+' if s > 0 else '-'}{'xyz'[axis]}")
        if off_axis is not None:
            for i, u in enumerate(_unit_axes(rng, TINY_RANDOM_AXES)):
                vectors.append(tuple(float(c) for c in (u * off_axis).astype(np.float32)))
                labels.append(f"{name},random{i}")
    _CACHE["tiny"] = _pad(vectors, labels)
    return _CACHE["tiny"]


def theta64(aa):
    """The rotation angle as rodrigues_cv.rotvec_to_rotmat forms it (float64) -> [...]."""
    r = np.asarray(aa, np.float32).astype(np.float64)
    return np.sqrt(r[..., 0] * r[..., 0] + r[..., 1] * r[..., 1] + r[..., 2] * r[..., 2])


def large():
    """-> (aa f32[N,24,3], labels[N,24])."""
    if "large" in _CACHE:
        return _CACHE["large"]
    two_pi = np.float32(2 * np.pi)
    near = {"2pi-ulp": np.nextafter(two_pi, np.float32(0)), "2pi": two_pi, "2pi+ulp": np.nextafter(two_pi, np.float32(10))}
    rng = np.random.default_rng(LARGE_SEED)
    vectors, labels = [(3e38, 3e38, 3e38)], ["3e38_diagonal"]
    for name, theta in LARGE_THETAS:
        theta = float(near[name]) if theta is None else float(np.float32(theta))
        for axis in range(3):
            v = [0.0, 0.0, 0.0]
            v[axis] = theta if axis != 1 else -theta
            vectors.append(tuple(v))
            labels.append(f"{name},{'+-+'[axis]}{'xyz'[axis]}")
        for i, u in enumerate(_unit_axes(rng, LARGE_RANDOM_AXES)):
            vectors.append(tuple(float(c) for c in (u * theta).astype(np.float32)))
            labels.append(f"{name},random{i}")
    _CACHE["large"] = _pad(vectors, labels)
    return _CACHE["large"]


# ---------------------------------------------------------------------------------------------------------------------
# nonfinite
# ---------------------------------------------------------------------------------------------------------------------
def nonfinite_base(N):
    """The finite batch the plants go into: f32[N,24,3], the first N frames of one seeded batch."""
    return np.random.default_rng(NONFINITE_SEED).standard_normal((max(NONFINITE_N), 24, 3)).astype(np.float32)[:N].copy()


def nonfinite_cases(N):
    """-> [(name, [(frame, joint, component, value), ...])]: the positions (frame 0 joint 0, frame 0 joint 23, frame 7 joint
    23, frame 8 joint 0, frame N-1 joint 23) that exist in N frames, dealt into as few batches as keep one plant to a frame;
    values and components in turn.  For N = 9, one more batch plants two joints of frame 8 (the only frame of the second
    workgroup)."""
    positions = []
    for p in ((0, 0), (0, 23), (7, 23), (8, 0), (N - 1, 23)):
        if p[0] < N and p not in positions:
            positions.append(p)
    start = NONFINITE_N.index(N) if N in NONFINITE_N else N
    batches = []
    for k, (f, j) in enumerate(positions):
        plant = (f, j, (k + start) % 3, NONFINITE_VALUES[(k + start) % len(NONFINITE_VALUES)])
        for b in batches:
            if all(q[0] != f for q in b):
                b.append(plant)
                break
        else:
            batches.append([plant])
    cases = [(f"N{N}_batch{i}", b) for i, b in enumerate(batches)]
    if N == 9:
        cases.append(("N9_two_joints_of_frame_8", [(8, 0, 1, NONFINITE_VALUES[0]), (8, 23, 2, NONFINITE_VALUES[2])]))
    return cases


def planted(N, plants):
    a = nonfinite_base(N)
    for f, j, c, v in plants:
        a[f, j, c] = v
    return a
