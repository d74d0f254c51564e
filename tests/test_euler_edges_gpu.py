"""pose_to_euler_kernel (csrc/frame_kernels.hip) on the edges of tests/euler_cases.py: the gimbal-lock branch, the status
bits and their per-frame attribution, rodrigues_vec2mat's `theta < DBL_EPSILON` cut, rotations far below and far above the
generic ones -- against oracle/coord_ref.py applied to the float32 axis-angle the kernel itself read or produced.

The criterion (euler_cases.compare) is derived, not measured.  Both sides do the same double operations on the same float32
matrix, so an angle agrees to max(1e-9 degrees, 1e-12 relative) -- unless a float32 entry under its atan2 came out as its
neighbour on one side, which moves the angle by at most euler_cases.flip_allowance; at most 0.1 % of a family's angles may
need that (the project's share in test_pose_to_euler_matches_golden).  tests/test_euler_edges_cpu.py holds the fixture to the
margins that make the branch, the zeros and the status bits of every case exact expectations."""
import numpy as np
import pytest
import torch

import euler_cases as ec
from conftest import measured
from oracle import rodrigues_cv
from poserisk_release_amd import _lib, ops

pytestmark = pytest.mark.gpu

POS_ZERO, NEG_ZERO = 0, np.int64(-2 ** 63)


def _t(a, dev):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev)


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64 if a.dtype == np.float64 else np.int32)


@pytest.fixture(scope="module")
def oracle():
    """name -> (aa, labels[n], detail, coord_ref's angles [n,3]), the oracle run once for every test here."""
    out = {}
    for name, (aa, labels) in (("gimbal", ec.gimbal()[:2]), ("tiny", ec.tiny()), ("large", ec.large())):
        out[name] = (aa, labels.reshape(-1), ec.detail(aa), ec.oracle_euler(aa).reshape(-1, 3))
    return out


def _run_axis_angle(aa, dev):
    """ops.axis_angle_to_euler on a float32 batch -> (euler f64[n,3], status int[N]); the input's bytes must survive."""
    a = _t(aa, dev)
    assert a.dtype == torch.float32 and a.is_contiguous()
    eul, st = ops.axis_angle_to_euler(a)
    back = a.cpu().numpy()
    assert np.array_equal(_bits(back), _bits(np.ascontiguousarray(aa))), "the entry wrote into its read-only input"
    return eul.cpu().numpy().reshape(-1, 3), st.cpu().numpy()


def _criterion(tag, got, want, R, absolute=1e-9, select=None):
    """ec.compare, asserted: no angle beyond the flip allowance, and at most FLIP_SHARE of them in need of it."""
    d, tight, flipped, bad = ec.compare(got, want, R, absolute=absolute)
    if select is not None:
        d, tight, flipped, bad = d[select], tight[select], flipped[select], bad[select]
    share = float(flipped.mean())
    measured(f"{tag}: Euler vs the oracle's Euler stage, angles within max(1e-9 deg, 1e-12 rel)", d[tight].max(initial=0.0),
             unit="deg")
    measured(f"{tag}: Euler vs the oracle's Euler stage, angles under the one-ulp flip allowance",
             d[flipped].max(initial=0.0), unit="deg")
    measured(f"{tag}: share of angles that need the flip allowance", share, ec.FLIP_SHARE)
    assert not bad.any(), (tag, np.argwhere(bad)[:8].tolist(), d[bad][:8].tolist())
    assert share <= ec.FLIP_SHARE, (tag, share)


def _assert_branch(tag, got, d, labels):
    """Every joint took the oracle's branch: in the lock ez is +0.0 bit for bit; outside it ez is an atan2 that is not 0."""
    lock = d["lock"]
    ez = _bits(got[:, 2])
    wrong_in = np.nonzero(lock & (ez != POS_ZERO))[0]
    wrong_out = np.nonzero(~lock & (got[:, 2] == 0))[0]
    assert len(wrong_in) == 0, (tag, "lock not taken", [(labels[i], d["sy"][i], got[i].tolist()) for i in wrong_in[:6]])
    assert len(wrong_out) == 0, (tag, "lock taken", [(labels[i], d["sy"][i], got[i].tolist()) for i in wrong_out[:6]])


def test_gimbal_axis_angle(gpu_device, oracle):
    """Mutants of pose_to_euler_kernel this is there for: the `else` branch never taken (182 joints expect ez = +0.0 and
    ex = atan2(-R[5], R[4])); its threshold at 1e-7 or 1e-5 (over 50 joints a side between) or moved by +-5 % (at least 8
    joints with sy in (0.95e-6, 1e-6) and 8 in (1e-6, 1.05e-6): _assert_branch names them); `atan2(R[5], R[4])` (ex changes
    sign, the diagonal vectors have ex = +-90); ez left from the other branch (the bits of +0.0 are asked for); root rows
    skipped (joint 0 of every frame is a case like the others); a write into the read-only input.  And of
    rodrigues_vec2mat: `c1 * rx * ry` in place of c1 (rx ry), or the contraction pragma dropped (the `order:` joints put 6
    to 10 of the 1152 angles under the flip allowance, tests/test_euler_edges_cpu.py; the share allows one)."""
    aa, labels, d, want = oracle["gimbal"]
    got, st = _run_axis_angle(aa, gpu_device)
    assert st.tolist() == [0] * len(aa)
    _assert_branch("euler gimbal, axis-angle in", got, d, labels)
    _criterion("euler gimbal, axis-angle in", got, want, d["R"])
    near = np.abs(d["sy"] / ec.LOCK - 1) < 0.05
    _criterion("euler gimbal, axis-angle in, sy within 5 % of the threshold", got, want, d["R"], select=near)


def test_gimbal_matrices(gpu_device, oracle):
    """The same rotations through ops.pose_to_euler (polar factor, acos, then the stage above): the kernel's axis-angle is
    rodrigues_cv's in double to one float32 ulp of the vector's largest component, and its angles and its branch are the
    oracle's on the axis-angle IT produced.  Same mutants as test_gimbal_axis_angle, on the pipeline's path."""
    rot = ec.gimbal()[2]
    labels = oracle["gimbal"][1]
    aa_t, eul_t, st_t = ops.pose_to_euler(_t(rot, gpu_device))
    aa, got = aa_t.cpu().numpy(), eul_t.cpu().numpy().reshape(-1, 3)
    assert st_t.cpu().tolist() == [0] * len(rot)
    ref = np.stack([rodrigues_cv.rotmat_to_rotvec(m) for m in rot.reshape(-1, 3, 3).astype(np.float64)]).reshape(aa.shape)
    big = np.abs(ref).max(axis=-1, keepdims=True).astype(np.float32)
    off = np.abs(aa.astype(np.float64) - ref) / np.spacing(np.maximum(big, np.float32(1e-30))).astype(np.float64)
    measured("euler gimbal, matrices in: axis-angle vs rodrigues_cv in double (float32 ulps of the largest component)",
             off.max(), 1.0, "ulp")
    assert off.max() <= 1.0, off.max()
    d = ec.detail(aa)
    assert not d["raises"].any()
    measured("euler gimbal, matrices in: smallest |sy / 1e-6 - 1| on our axis-angle", np.abs(d["sy"] / ec.LOCK - 1).min())
    assert int(d["lock"].sum()) >= 150 and int((~d["lock"]).sum()) >= 150
    _assert_branch("euler gimbal, matrices in", got, d, labels)
    _criterion("euler gimbal, matrices in", got, ec.oracle_euler(aa).reshape(-1, 3), d["R"])


def test_tiny(gpu_device, oracle):
    """Mutants of rodrigues_vec2mat: the cut at FLT_EPSILON, or anywhere above the float32 neighbours of 2^-52 (a rotation of
    2.2e-16 .. 1e-12 rad is 1.3e-14 .. 5.7e-11 degrees: invisible at 1e-9 degrees, so the relative part of the criterion
    stands alone here); `theta <= DBL_EPSILON` (at_cut is above); the cut dropped (0 / 0 below it; pad_zero is theta = 0);
    an identity written with another sign of zero (the angles are (0, -0, 0) bit for bit)."""
    aa, labels, d, want = oracle["tiny"]
    got, st = _run_axis_angle(aa, gpu_device)
    assert st.tolist() == [0] * len(aa)
    below = ec.theta64(aa).reshape(-1) < ec.DBL_EPS
    assert below.sum() >= 40 and (~below).sum() >= 90
    exact = np.tile(np.array([POS_ZERO, NEG_ZERO, POS_ZERO], np.int64), (int(below.sum()), 1))
    assert np.array_equal(_bits(got[below]), exact), [(labels[i], got[i].tolist()) for i in np.nonzero(below)[0][:6]]
    assert np.array_equal(_bits(want[below]), exact)
    _criterion("euler tiny, above the cut", got, want, d["R"], absolute=0.0, select=~below)
    with np.errstate(divide="ignore", invalid="ignore"):
        rel = np.abs(got - want)[~below] / np.abs(want[~below])
    measured("euler tiny, above the cut: largest relative difference of an angle", np.nanmax(rel), 1e-12)


def test_large(gpu_device, oracle):
    """The same criterion at every magnitude, with no bound on |v| below float32's largest: cos and sin of 6.28 .. 5e38 in
    double (an argument reduction that loses bits shows here first; the device's agree with glibc's at every magnitude
    tried), 1 / theta and the squares of 3e38 (float32 arithmetic would overflow), the sum under theta in another order (at
    1e30 one ulp of theta is another rotation), status zero throughout."""
    aa, labels, d, want = oracle["large"]
    got, st = _run_axis_angle(aa, gpu_device)
    assert st.tolist() == [0] * len(aa)
    assert np.isfinite(got).all()
    dd, tight, flipped, bad = ec.compare(got, want, d["R"])
    for name in ["3e38_diagonal"] + [n for n, _ in ec.LARGE_THETAS]:
        sel = np.array([v == name or str(v).startswith(name + ",") for v in labels])
        measured(f"euler large, theta {name}: Euler vs the oracle's Euler stage", dd[sel].max(), unit="deg")
        measured(f"euler large, theta {name}: angles beyond max(1e-9 deg, 1e-12 rel)", int((~tight[sel]).sum()))
    _criterion("euler large", got, want, d["R"])


@pytest.fixture(scope="module")
def unplanted(gpu_device):
    """N -> the Euler angles of the finite base batch: status all zero, and the oracle's angles (generic rotations; too few
    for a share of them to mean anything, so no angle beyond the flip allowance is all that is asked)."""
    out = {}
    for N in ec.NONFINITE_N:
        base = ec.nonfinite_base(N)
        got, st = _run_axis_angle(base, gpu_device)
        assert st.tolist() == [0] * N
        bad = ec.compare(got, ec.oracle_euler(base).reshape(-1, 3), ec.detail(base)["R"])[3]
        assert not bad.any(), (N, np.argwhere(bad)[:6].tolist())
        out[N] = got.reshape(N, 24, 3)
    return out


@pytest.mark.parametrize("N", ec.NONFINITE_N)
def test_nonfinite_sets_bit_0_on_its_frame_only(gpu_device, unplanted, N):
    """A NaN (with or without payload) or an infinity in one component: the oracle raises "not a rotation matrix" for that
    frame, the kernel sets bit 0 of that frame's status and nothing else.  Mutants: `sqrtf(n2) >= 1e-6f` in place of
    `!(sqrtf(n2) < 1e-6f)` (a NaN norm compares false: status stays 0); `atomicOr` dropped (status stays 0); `flags[t % 8]`
    (frame 0 joint 23 lands on frame 7, or nowhere for N < 8); `flags[lf + 1]` or `status[f + 1]` (the plant of frame f shows on
    frame f + 1, the one of frame N-1 nowhere); the flag reset after the barrier or the status of the second workgroup read
    from the first (frame 7 joint 23 against frame 8 joint 0); root rows skipped (joint 0 planted); bit 1 set along (status
    is 1, not 3); a status slot of a frame >= N written (N = 1, 7, 9, 17 leave slots of the last workgroup unused; the
    guard-band test owns the write itself)."""
    for name, plants in ec.nonfinite_cases(N):
        a = ec.planted(N, plants)
        got, st = _run_axis_angle(a, gpu_device)
        want_st = np.zeros(N, np.int64)
        keep = np.ones((N, 24), bool)
        for f, j, _, _ in plants:
            want_st[f] = 1
            keep[f, j] = False
        assert st.tolist() == want_st.tolist(), (name, st.tolist())
        same = _bits(got.reshape(N, 24, 3)) == _bits(unplanted[N])
        assert same[keep].all(), (name, np.argwhere(~same & keep[:, :, None])[:6].tolist())


def test_status_pointer_may_be_null(gpu_device, unplanted):
    """pr_axis_angle_to_euler with status_dev = NULL on a planted batch: PR_OK, and the Euler bits of the call that has a
    status (the planted joints' NaNs included, as bits)."""
    N = 9
    name, plants = ec.nonfinite_cases(N)[0]
    a = _t(ec.planted(N, plants), gpu_device)
    want, st = ops.axis_angle_to_euler(a)
    assert st.cpu().tolist() == [1 if f in {p[0] for p in plants} else 0 for f in range(N)]
    eul = torch.full((N, 24, 3), 7.0, dtype=torch.float64, device=gpu_device)
    stream = torch.cuda.current_stream(gpu_device).cuda_stream
    rc = _lib.load().pr_axis_angle_to_euler(a.data_ptr(), N, eul.data_ptr(), None, stream)
    assert rc == 0
    torch.cuda.synchronize(gpu_device)
    assert np.array_equal(_bits(eul.cpu().numpy()), _bits(want.cpu().numpy()))
    keep = np.ones((N, 24), bool)
    for f, j, _, _ in plants:
        keep[f, j] = False
    assert (_bits(eul.cpu().numpy()) == _bits(unplanted[N]))[keep].all()


@pytest.mark.parametrize("value", [np.nan, 100.0, -100.0], ids=["nan", "plus_100", "minus_100"])
def test_matrix_entry_outside_check_range(gpu_device, value):
    """Through the pipeline's entry a matrix entry that OpenCV's checkRange(-100, 100) refuses (NaN, or +-100, its edge)
    makes Rodrigues return the zero vector: status stays 0 on every frame, that joint's axis-angle is exactly zero and its
    angles are exactly (0, -0, 0); every other joint keeps the bits of the clean run.  Mutants: `fabs(R[e]) <= 100.0`; the NaN
    let through to the polar factor; bit 0 set from the input matrix instead of from the rebuilt one."""
    rot = ec.gimbal()[2][:9].copy()
    clean = ops.pose_to_euler(_t(rot, gpu_device))
    f, j = 8, 5
    rot[f, j, 1, 2] = value
    assert rodrigues_cv.rotmat_to_rotvec(rot[f, j]).tolist() == [0.0, 0.0, 0.0]
    aa, eul, st = ops.pose_to_euler(_t(rot, gpu_device))
    assert st.cpu().tolist() == [0] * 9
    aa, eul = aa.cpu().numpy(), eul.cpu().numpy()
    assert np.array_equal(_bits(aa[f, j]), np.zeros(3, np.int32))
    assert np.array_equal(_bits(eul[f, j]), np.array([POS_ZERO, NEG_ZERO, POS_ZERO], np.int64))
    keep = np.ones((9, 24), bool)
    keep[f, j] = False
    assert (_bits(aa) == _bits(clean[0].cpu().numpy()))[keep].all()
    assert (_bits(eul) == _bits(clean[1].cpu().numpy()))[keep].all()
