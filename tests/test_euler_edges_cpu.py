"""The inputs of tests/euler_cases.py held to the oracle, without a GPU: conditions on the fixture that let
tests/test_euler_edges_gpu.py assert branches, status bits and exact zeros with no allowances of its own -- and, in emulation,
that the criterion it applies does reject the one-line mutants of the Euler stage it is there for."""
import math

import numpy as np
import pytest

import euler_cases as ec
from conftest import measured
from oracle import coord_ref, rodrigues_cv


@pytest.fixture(scope="module")
def families():
    """name -> (aa f32[N,24,3], labels[N*24], detail): every finite family, the oracle run once."""
    out = {}
    for name, aa in (("gimbal", ec.gimbal()[0]), ("tiny", ec.tiny()[0]), ("large", ec.large()[0]),
                     ("nonfinite_base", ec.nonfinite_base(max(ec.NONFINITE_N)))):
        out[name] = (aa, ec.detail(aa))
    # the matrices of the gimbal family, through the oracle's own matrix -> vector stage
    rot = ec.gimbal()[2]
    aa = np.stack([rodrigues_cv.rotmat_to_rotvec(m) for m in rot.reshape(-1, 3, 3)]).reshape(-1, 24, 3)
    assert aa.dtype == np.float32
    out["gimbal_matrices"] = (aa, ec.detail(aa))
    return out


def test_detail_is_the_oracle(families):
    """ec.detail takes coord_ref.axis_angle_to_euler_angle apart; its angles are that function's, bit for bit, and it raises
    on no finite case."""
    for name, (aa, d) in families.items():
        assert not d["raises"].any(), (name, np.nonzero(d["raises"])[0])
        want = ec.oracle_euler(aa).reshape(-1, 3)
        assert np.array_equal(want.view(np.int64), d["euler"].view(np.int64)), name


def test_gimbal_branch_margin_coverage_and_counts(families):
    aa, labels, rot = ec.gimbal()
    assert aa.shape == (ec.GIMBAL_FRAMES, 24, 3) and rot.shape == (ec.GIMBAL_FRAMES, 24, 3, 3) and aa.dtype == np.float32
    d = families["gimbal"][1]
    sy, lock = d["sy"], d["lock"]
    # margin: one ulp between two libms' cos / sin can flip the float32 rounding of R00 or R10 and move sy by ~1.2e-7
    # relative; outside a band of 1e-4 the kernel and the oracle must take the same branch
    rel = np.abs(sy / ec.LOCK - 1.0)
    measured("euler gimbal fixture: smallest |sy / 1e-6 - 1|", rel.min())
    assert rel.min() > ec.LOCK_MARGIN
    below, above = int(((sy > 0.95e-6) & (sy < 1e-6)).sum()), int(((sy > 1e-6) & (sy < 1.05e-6)).sum())
    measured("euler gimbal fixture: joints with sy in (0.95e-6, 1e-6)", below)
    measured("euler gimbal fixture: joints with sy in (1e-6, 1.05e-6)", above)
    assert below >= 8 and above >= 8
    assert int(lock.sum()) >= 150 and int((~lock).sum()) >= 150, (lock.sum(), (~lock).sum())
    # a threshold moved by a decade either way changes the branch of many joints
    assert int(((sy >= 1e-7) & (sy < 1e-6)).sum()) >= 50 and int(((sy >= 1e-6) & (sy < 1e-5)).sum()) >= 50
    # in the lock ez is the integer 0 of the reference: +0.0, not an atan2
    ez = d["euler"][lock, 2]
    assert np.all(ez == 0) and not np.signbit(ez).any()
    # ... and every other joint's ez tells the branch: it is not zero
    assert np.all(d["euler"][~lock, 2] != 0)
    # both signs of pi/2, every eps, and both exact vectors in the lock
    lab = labels.reshape(-1)
    for eps in ec.GIMBAL_EPS + tuple(v * g for v in ec.GIMBAL_NEAR for g in (1.0, -1.0)):
        for s in "+-":
            assert (lab == f"eps={eps:+.3g},pitch={s}pi/2").sum() >= 5, (eps, s)
    for name, want in (("exact_y+", (-0.0, 89.9999975, 0.0)), ("exact_y-", (0.0, -89.9999975, 0.0))):
        i = int(np.nonzero(lab == name)[0][0])
        assert lock[i] and abs(sy[i] - 4.37e-8) < 1e-10
        np.testing.assert_allclose(d["euler"][i], want, atol=1e-7)
        assert np.signbit(d["euler"][i, 0]) == np.signbit(want[0])
    diag = np.array([str(v).startswith("diagonal") for v in lab])
    assert diag.sum() == 8 and lock[diag].sum() == 4
    assert np.all(np.abs(np.abs(d["euler"][diag & lock, 0]) - 90) < 1e-5)      # yaw and roll mix into ex: not 0


def test_gimbal_matrices_are_the_same_rotations(families):
    """The float32 matrices name the rotations of the float32 vectors: the oracle's vector of each is the family's vector to
    the float32 rounding of the matrix (entries rounded at 6e-8, a lock's entries of 1e-6 included), and both branches are
    as well populated.  (Which branch the kernel must take on this path is decided on ITS axis-angle, in the GPU file.)"""
    aa = ec.gimbal()[0].reshape(-1, 3)
    am, d = families["gimbal_matrices"]
    assert np.abs(am.reshape(-1, 3).astype(np.float64) - aa).max() < 2e-6
    assert int(d["lock"].sum()) >= 150 and int((~d["lock"]).sum()) >= 150


def test_status_margins(families):
    """Bit 0 (isRotationMatrix): the oracle's float32 norm stays below 5e-7 on every finite case, against the threshold of
    1e-6, so neither numpy's nor the kernel's summation order decides it.  Bit 1 (round trip): the signed sum stays below
    1e-5 against 0.1 -- R always comes out of Rodrigues' formula, so the round trip reproduces it to float32 rounding, and no
    input reaches the bit."""
    for name, (aa, d) in families.items():
        measured(f"euler {name} fixture: isRotationMatrix norm (threshold 1e-6)", d["norm"].max(), 5e-7)
        measured(f"euler {name} fixture: signed round-trip sum (threshold 0.1)", d["dsum"].max(), 1e-5)
        assert d["norm"].max() < 5e-7, name
        assert d["dsum"].max() < 1e-5, name


def test_tiny_sits_on_both_sides_of_the_cut(families):
    aa, labels = ec.tiny()
    d = families["tiny"][1]
    theta, lab = ec.theta64(aa).reshape(-1), labels.reshape(-1)
    below = theta < ec.DBL_EPS
    # the cut is decided in double from a sum of three squares, which a compiler may fuse: theta is the cut itself (the
    # coordinate axes, where the sum is exact) or at least 1e-12 (relative) away from it
    rel = np.abs(theta / ec.DBL_EPS - 1.0)
    assert np.all((rel == 0) | (rel > 1e-12))
    on_axis = np.array(["random" not in str(v) and v != "pad_zero" for v in lab])
    assert np.all(theta[on_axis] == np.abs(aa.reshape(-1, 3)[on_axis]).max(axis=1))
    for name, want_below in (("1e-20", True), ("below_cut", True), ("at_cut", False), ("above_cut", False), ("1e-15", False)):
        sel = np.array([str(v).startswith(name + ",") for v in lab])
        assert sel.sum() >= 6 and np.all(below[sel] == want_below), name
    # the float32 neighbours of 2^-52 are in
    assert np.float32(ec.DBL_EPS) == ec.DBL_EPS
    assert theta[lab == "below_cut,+x"][0] == np.nextafter(np.float32(ec.DBL_EPS), np.float32(0))
    assert theta[lab == "above_cut,+x"][0] == np.nextafter(np.float32(ec.DBL_EPS), np.float32(1))
    # below the cut the oracle's matrix is the identity and its angles are (0, -0, 0), signs included
    e = d["euler"][below]
    assert np.all(e == 0) and np.array_equal(np.signbit(e), np.tile([False, True, False], (len(e), 1)))
    # above it every rotation shows: the largest angle of a joint is theta in degrees to float32 rounding -- from 1.3e-14
    # degrees, far below the 1e-9 an absolute tolerance would forgive
    big = np.abs(d["euler"][~below]).max(axis=1)
    assert np.all(big > 0.5 * np.degrees(theta[~below])) and np.all(big <= np.degrees(theta[~below]) * (1 + 1e-6))
    assert big.min() < 1.3e-14
    for name, _ in ec.TINY_THETAS:
        assert np.array([str(v).startswith(name + ",") for v in lab]).sum() >= 6, name


def test_large_reaches_every_magnitude(families):
    aa, labels = ec.large()
    theta, lab = ec.theta64(aa).reshape(-1), labels.reshape(-1)
    two_pi = np.float32(2 * np.pi)
    assert theta[lab == "2pi-ulp,+x"][0] == np.nextafter(two_pi, np.float32(0))
    assert theta[lab == "2pi+ulp,+x"][0] == np.nextafter(two_pi, np.float32(10))
    for name, want in (("10", 10.0), ("1e2", 1e2), ("1e4", 1e4), ("1e6", 1e6), ("1e12", 1e12), ("1e30", 1e30)):
        sel = np.array([str(v).startswith(name + ",") for v in lab])
        assert sel.sum() >= 3 + ec.LARGE_RANDOM_AXES and np.all(np.abs(theta[sel] / want - 1) < 1e-6), name
    i = int(np.nonzero(lab == "3e38_diagonal")[0][0])
    assert np.all(aa.reshape(-1, 3)[i] == np.float32(3e38)) and np.isfinite(theta[i])
    # (The sum under theta cannot tell a fused multiply-add: the square of a float32 is exact in double.  Its order can: at
    # 1e30 an ulp of theta is 1e14 rad, so z z + y y + x x in place of x x + y y + z z is another rotation on some vector.)
    flat = aa.reshape(-1, 3).astype(np.float64)
    swapped = np.sqrt(flat[:, 2] * flat[:, 2] + flat[:, 1] * flat[:, 1] + flat[:, 0] * flat[:, 0])
    hit = (swapped != theta) & (theta >= 1e11)
    assert hit.sum() >= 1 and np.all(np.abs(np.cos(swapped[hit]) - np.cos(theta[hit])) > 1e-6)


def test_gimbal_tells_the_order_of_the_double_operations(families):
    """Next to the lock R00, R10, R21 and R22 cancel from 0.3 to 1e-6, so the last ulp of a double is 1/600 of a float32 ulp
    of theirs, and an order of operations other than OpenCV's (c1 rx first, or a fused multiply-add) rounds some entry to the
    neighbouring float32.  Each flip is within the GPU file's allowance by construction; what rejects these orders is the
    cap on the share of angles that need it, so the family holds ORDER_PER_VARIANT joints chosen for each order: four and
    more of 1152 angles against a cap of one.  pose_to_euler_kernel did have `c1 * rx * ry`, contracted; on the joints drawn
    without looking at any order that was 2 of 1152 angles."""
    aa, d = families["gimbal"]
    flat = aa.reshape(-1, 3)
    assert all(np.array_equal(ec.rodrigues_in_order(v), R) for v, R in zip(flat, d["R"]))
    lab = ec.gimbal()[1].reshape(-1)
    for name, kw in ec.ORDER_VARIANTS:
        R = np.stack([ec.rodrigues_in_order(v, **kw) for v in flat])
        _, tight, flipped, bad = ec.compare(_euler_stage(R), d["euler"], d["R"])
        measured(f"euler gimbal fixture: angles that need the flip allowance under '{name}'", int(flipped.sum()))
        assert not bad.any(), name
        chosen = np.array([str(v).startswith(f"order:{name}:") for v in lab])
        assert chosen.sum() == ec.ORDER_PER_VARIANT and flipped[chosen].any(axis=1).all(), name
        assert flipped.mean() > 3 * ec.FLIP_SHARE, (name, int(flipped.sum()))


def test_nonfinite_plants_raise_and_the_base_does_not(families):
    """Every plant, alone in its frame, makes coord_ref.axis_angle_to_euler_angle raise RotationAssertion for that frame (a
    NaN or an infinity makes theta, so R, NaN, and isRotationMatrix compares a NaN norm); the unplanted batch does not."""
    assert not families["nonfinite_base"][1]["raises"].any()
    values, positions = set(), set()
    for N in ec.NONFINITE_N:
        base = ec.nonfinite_base(N)
        assert base.shape == (N, 24, 3) and np.isfinite(base).all()
        cases = ec.nonfinite_cases(N)
        for name, plants in cases:
            frames = [p[0] for p in plants]
            assert len(set(frames)) == len(frames) or name == "N9_two_joints_of_frame_8", name
            got = ec.planted(N, plants)
            for f, j, c, v in plants:
                assert 0 <= f < N and 0 <= j < 24 and not np.isfinite(v)
                values.add(int(np.array([v], np.float32).view(np.uint32)[0]))
                positions.add((N, f, j))
                alone = base[f].copy()
                alone[j, c] = v
                with pytest.raises(coord_ref.RotationAssertion, match="not a rotation matrix"):
                    ec.oracle_euler(alone[None])
                with pytest.raises(coord_ref.RotationAssertion):
                    ec.oracle_euler(got[f][None])
            for f in set(range(N)) - set(frames):
                assert np.array_equal(got[f], base[f])
        for f, j in ((0, 0), (0, 23), (7, 23), (8, 0), (N - 1, 23)):
            assert f >= N or (N, f, j) in positions, (N, f, j)
    assert len(values) == 4                                      # NaN, +inf, -inf and a NaN with a payload
    assert sum(name == "N9_two_joints_of_frame_8" for N in ec.NONFINITE_N for name, _ in ec.nonfinite_cases(N)) == 1


# ---------------------------------------------------------------------------------------------------------------------
# the criterion against mutants, in emulation
# ---------------------------------------------------------------------------------------------------------------------
def _euler_stage(R, threshold=ec.LOCK, r12_sign=-1.0, ez_from_other_branch=False):
    """rotationMatrixToEulerAngles as the kernel writes it, on float32 matrices, with the mutations as parameters."""
    out = np.empty((len(R), 3))
    for k, M in enumerate(R):
        sy = math.sqrt(M[0, 0] * M[0, 0] + M[1, 0] * M[1, 0])
        if not sy < threshold:
            e = (math.atan2(M[2, 1], M[2, 2]), math.atan2(-M[2, 0], sy), math.atan2(M[1, 0], M[0, 0]))
        else:
            e = (math.atan2(r12_sign * M[1, 2], M[1, 1]), math.atan2(-M[2, 0], sy),
                 math.atan2(M[1, 0], M[0, 0]) if ez_from_other_branch else 0.0)
        out[k] = np.array(e) * 180 / math.pi
    return out


def test_criterion_passes_the_stage_and_rejects_its_mutants(families):
    """ec.compare on the gimbal family: the unmutated stage is the oracle exactly; each mutant of the branch is `bad` on
    joints, and by more than the flip share could excuse."""
    d = families["gimbal"][1]
    R, want = d["R"], d["euler"]
    assert np.array_equal(_euler_stage(R).view(np.int64), want.view(np.int64))
    mutants = {"branch never taken": dict(threshold=0.0), "threshold 1e-7": dict(threshold=1e-7),
               "threshold 1e-5": dict(threshold=1e-5), "threshold -5 %": dict(threshold=0.95e-6),
               "threshold +5 %": dict(threshold=1.05e-6), "atan2(R[5], R[4])": dict(r12_sign=1.0),
               "ez left from the other branch": dict(ez_from_other_branch=True)}
    for name, kw in mutants.items():
        _, tight, flipped, bad = ec.compare(_euler_stage(R, **kw), want, R)
        joints = int(bad.any(axis=1).sum())
        measured(f"euler gimbal fixture: joints that reject the mutant '{name}'", joints)
        assert joints >= 8, name


def test_criterion_rejects_a_cut_at_flt_epsilon(families):
    """A kernel that returned the identity below FLT_EPSILON gives (0, -0, 0) for every tiny rotation: within 1e-9 degrees of
    the oracle up to theta = 1e-12, and `bad` all the same under the relative criterion."""
    aa, d = families["tiny"]
    theta = ec.theta64(aa).reshape(-1)
    cut = aa.reshape(-1, 3).copy()
    cut[theta < np.finfo(np.float32).eps] = 0
    mutant = ec.detail(cut)["euler"]
    dd, tight, flipped, bad = ec.compare(mutant, d["euler"], d["R"], absolute=0.0)
    hit = (theta >= ec.DBL_EPS) & (theta < np.finfo(np.float32).eps)
    assert hit.sum() >= 60 and np.all(bad[hit].any(axis=1))
    assert np.all(dd[hit & (theta < 1e-11)] < 1e-9)               # what the absolute criterion alone would have passed
    assert not bad[~hit].any()
