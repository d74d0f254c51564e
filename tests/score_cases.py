"""The REBA / RULA probe set: poses and info dicts that drive the two scoring kernels onto every rule edge and every table
cell.  Numpy only and deterministic: tests/golden/make_golden.py runs the reference's own classes over the pairs and stores
the results (score_probes.npz); the tests rebuild the inputs from here and compare.

  build() -> (pose f64[N,24,3], blocks {name: (start, stop)}, infos [dict], pairs [(block name, info index)])

Blocks of rows:
  grid      per rule group (the angles of one joint that the rules read together), the full product of the angle classes: with
            sorted thresholds t1 < ... < tk an angle has the k classes "exactly ti" and the k+1 open intervals between them,
            an interval being represented by the double next to its lower end (the leftmost by the double below t1).  Groups
            on different joints share rows, the shorter products cycling.  The thresholds are the union of what reba.py and
            rula.py compare an angle with, because one pose feeds both kernels.
  cross     the product of the four shoulder angles through which the reference's right-arm rules read the LEFT arm and its
            right-arm rotation bumps the LEFT score; the other joints go on cycling.
  specials  NaN, +-inf, +-0, +-180 in each angle a rule reads, the rest at the baseline; NaN and +-inf in each position of the
            pairs read together, against every class of the partner.
  cells_ab  every (trunk, neck) sub-score pair of REBA's table A and every (neck, trunk) pair of RULA's table B; the leg index
            of both tables comes from the info.
  cells_reba_arm, cells_rula_arm
            every per-arm index tuple of REBA's table B and of RULA's table A, on the left arm with the right at its minimum,
            on the right with the left at its minimum, and on both arms at once (the two arms enter through max()).
  corner    the baseline pose, which every info of the (score A, score B) shift grid carries across the whole of table C.

Infos: the rule infos (Sitting, the arm supports, the legs fields) run over grid, cross and specials; the shift infos (one
field non-zero, and sums that move a group score along table C's rows and columns and past its clamps) run over the cells.
The reference clips before every table lookup (np.clip), so any small integer is a legal field value; |value| <= 20.
"""
import itertools

import numpy as np

JOINTS = ('Pelvis', 'L_Hip', 'R_Hip', 'Torso', 'L_Knee', 'R_Knee', 'Spine', 'L_Ankle', 'R_Ankle', 'Chest',
          'L_Toe', 'R_Toe', 'Neck', 'L_Thorax', 'R_Thorax', 'Head', 'L_Shoulder', 'R_Shoulder', 'L_Elbow',
          'R_Elbow', 'L_Wrist', 'R_Wrist', 'L_Hand', 'R_Hand')
J = {n: i for i, n in enumerate(JOINTS)}

REBA_KEYS = ("Legs_bilateral_weight_bearing/walking", "Sitting", "Load/Force Score", "Arm_supported_leaning_L",
             "Arm_supported_leaning_R", "Coupling", "Activity_Score")
RULA_KEYS = ("Arm_supported_leaning_L", "Arm_supported_leaning_R", "A_Muscle_use_L", "A_Muscle_use_R", "A_Load/Force_L",
             "A_Load/Force_R", "Legs_bilateral_weight_bearing", "B_Muscle_use", "B_Load/Force")

# rule group -> [(joint, axis, thresholds)]: every constant reba.py:140-392 or rula.py:158-422 compares that angle with
GROUPS = {
    "torso": [("Torso", 0, (-20, -5, 5, 20, 60)), ("Torso", 1, (-10, 10)), ("Torso", 2, (-10, 10))],
    "neck": [("Neck", 0, (-5, 10, 20)), ("Neck", 1, (-10, 10)), ("Neck", 2, (-10, 10))],
    "knees": [("L_Knee", 0, (30, 60)), ("R_Knee", 0, (30, 60))],
    "l_upper_arm": [("L_Shoulder", 2, (-110, -70, -20, 45, 110)), ("L_Shoulder", 1, (-90, -70, -45, -20, 20, 70)),
                    ("L_Shoulder", 0, (-10, 10))],
    "r_upper_arm": [("R_Shoulder", 2, (-70, 20, 45, 110)), ("R_Shoulder", 1, (-90, -70, -45, -20, 20, 45, 70, 90)),
                    ("R_Shoulder", 0, (-10, 10))],
    "l_thorax": [("L_Thorax", 0, (-45, -10, 10)), ("L_Thorax", 2, (-10, 10))],
    "r_thorax": [("R_Thorax", 0, (-10, 10, 45)), ("R_Thorax", 2, (-10, 10))],
    "l_elbow": [("L_Elbow", 1, (-100, -60, 0)), ("L_Elbow", 2, (-100, -60, 0))],
    "r_elbow": [("R_Elbow", 1, (0, 60, 100)), ("R_Elbow", 2, (0, 60, 100))],
    "l_wrist": [("L_Wrist", 0, (-45, -10, 10, 45)), ("L_Wrist", 1, (-10, 10)), ("L_Wrist", 2, (-15, -1, 1, 15))],
    "r_wrist": [("R_Wrist", 0, (-45, -10, 10, 45)), ("R_Wrist", 1, (-10, 10)), ("R_Wrist", 2, (-15, -1, 1, 15))],
}
# Q13 / Q14: the right arm's rules read these left-arm angles, and the right arm's rotation bumps the left score
CROSS = [("R_Shoulder", 2, (20, 110)), ("R_Shoulder", 0, (-10, 10)), ("L_Shoulder", 2, (-110, -20)),
         ("L_Shoulder", 1, (-70, -20, 20, 70))]
# angles read together by one condition: (joint, axis a, axis b)
PAIRS_READ_TOGETHER = [("L_Elbow", 1, 2), ("R_Elbow", 1, 2), ("Neck", 2, 1), ("L_Wrist", 1, 0), ("R_Wrist", 1, 0)]
SPECIAL_VALUES = (np.nan, np.inf, -np.inf, 0.0, -0.0, 180.0, -180.0)

FILLER = 7.5          # joints no rule reads
# the finite baseline: every sub-score of both scorers at its minimum, each arm inside its own first branch
BASELINE = {("L_Shoulder", 2): -60.0, ("R_Shoulder", 2): 60.0, ("L_Elbow", 1): -80.0, ("L_Elbow", 2): -80.0,
            ("R_Elbow", 1): 80.0, ("R_Elbow", 2): 80.0}


def read_angles():
    """Every (joint, axis) a rule reads, with its thresholds, in GROUPS order."""
    return [a for g in GROUPS.values() for a in g]


def thresholds_of(joint, axis):
    for j, k, th in read_angles():
        if (j, k) == (joint, axis):
            return th
    raise KeyError((joint, axis))


def class_values(th):
    """One double per class of an angle, in class order: below t1, t1, just above t1, t2, just above t2, ..."""
    th = np.asarray(th, np.float64)
    vals = [np.nextafter(th[0], -np.inf)]
    for t in th:
        vals += [t, np.nextafter(t, np.inf)]
    return np.array(vals, np.float64)


def baseline_pose(n=1):
    p = np.full((n, 24, 3), FILLER, np.float64)
    for j, k, _ in read_angles():
        p[:, J[j], k] = 0.0
    for (j, k), v in BASELINE.items():
        p[:, J[j], k] = v
    return p


def _product_rows(angles):
    """The full product of the angles' class values: f64[rows, len(angles)]."""
    return np.array(list(itertools.product(*[class_values(th) for _, _, th in angles])), np.float64)


def _fill_groups(pose, skip=()):
    """Every group's product into the rows of `pose`, cycling."""
    n = len(pose)
    for name, angles in GROUPS.items():
        rows = _product_rows(angles)
        idx = np.arange(n) % len(rows)
        for c, (j, k, _) in enumerate(angles):
            if (j, k) not in skip:
                pose[:, J[j], k] = rows[idx, c]


def grid_block():
    n = max(len(_product_rows(a)) for a in GROUPS.values())
    pose = baseline_pose(n)
    _fill_groups(pose)
    return pose


def cross_block():
    rows = _product_rows(CROSS)
    pose = baseline_pose(len(rows))
    shoulders = {(j, k) for g in ("l_upper_arm", "r_upper_arm") for j, k, _ in GROUPS[g]}
    _fill_groups(pose, skip=shoulders)
    for c, (j, k, _) in enumerate(CROSS):
        pose[:, J[j], k] = rows[:, c]
    return pose


def specials_block():
    rows = []
    for j, k, _ in read_angles():
        for v in SPECIAL_VALUES:
            p = baseline_pose()[0]
            p[J[j], k] = v
            rows.append(p)
    for j, a, b in PAIRS_READ_TOGETHER:
        for here, partner in ((a, b), (b, a)):
            for v in (np.nan, np.inf, -np.inf):
                for w in class_values(thresholds_of(j, partner)):
                    p = baseline_pose()[0]
                    p[J[j], here] = v
                    p[J[j], partner] = w
                    rows.append(p)
    return np.stack(rows)


# ---- cells ------------------------------------------------------------------------------------------------------------
# Torso[0]: (REBA bend, RULA bend) = (1,1) (2,2) (3,3) (4,4) (2,1) (3,1); [1] twists both; [2] bends RULA's side only.
# Neck[0]: (REBA, RULA) = (1,1) (1,2) (1,3) (2,4); Neck[1] twists both.
_TORSO0, _NECK0 = (0.0, 10.0, 30.0, 70.0, -10.0, -30.0), (0.0, 15.0, 25.0, -10.0)


def cells_ab_block():
    rows = []
    for t0, t1, t2, n0, n1 in itertools.product(_TORSO0, (0.0, 15.0), (0.0, 15.0), _NECK0, (0.0, 15.0)):
        p = baseline_pose()[0]
        p[J["Torso"]] = (t0, t1, t2)
        p[J["Neck"], 0], p[J["Neck"], 1] = n0, n1
        rows.append(p)
    return np.stack(rows)


# upper-arm sub-score 1..6 -> (Shoulder[2], Shoulder[1], Shoulder[0], Thorax[2]); derived from reba.py:203-335 and
# rula.py:158-288 by hand (bending + shoulder rise + abduction, no arm support)
_REBA_UA = {"L": [(-60, 0, 0, 0), (-60, 0, 0, 15), (-60, 30, 0, 15), (-60, -60, 0, 15), (-60, -100, 0, 15), (-60, -100, 15, 15)],
            "R": [(60, 0, 0, 0), (60, 0, 0, 15), (60, 30, 0, 15), (60, 60, 0, 15), (60, 100, 0, 15), (60, 100, 15, 15)]}
_RULA_UA = {"L": [(-60, 0, 0, 0), (-60, 0, 0, 15), (-60, 30, 0, 15), (-60, -60, 0, 15), (-60, -100, 0, 15), (120, -50, 0, 15)],
            "R": [(60, 0, 0, 0), (60, 30, 0, 0), (60, 30, 0, 15), (60, 60, 0, 15), (60, 100, 0, 15), (30, 100, 0, 15)]}
# lower arm: (Elbow[1] = Elbow[2], Thorax[0]); REBA 1..2 ignores the thorax, RULA 1..3 adds it
_LA = {"L": [(-80, 0), (-30, 0), (-30, 20)], "R": [(80, 0), (30, 0), (30, -20)]}
# wrist (Wrist[2], Wrist[1]): REBA 1..3, RULA 1..4; twist Wrist[0]: RULA 1..2
_REBA_WR = [(0, 0), (20, 0), (20, 15)]
_RULA_WR = [(0, 0), (5, 0), (20, 0), (20, 15)]
_TWIST = [0, 60]


def _set_arm(p, side, ua, la, wr, twist=0):
    s2, s1, s0, th2 = ua
    e, th0 = la
    w2, w1 = wr
    p[J[f"{side}_Shoulder"]] = (s0, s1, s2)
    p[J[f"{side}_Thorax"], 0], p[J[f"{side}_Thorax"], 2] = th0, th2
    p[J[f"{side}_Elbow"], 1] = p[J[f"{side}_Elbow"], 2] = e
    p[J[f"{side}_Wrist"]] = (twist, w1, w2)


def _arm_cells(tuples, setter):
    rows = []
    for sides in (("L",), ("R",), ("L", "R")):
        for t in tuples:
            p = baseline_pose()[0]
            for s in sides:
                setter(p, s, t)
            rows.append(p)
    return np.stack(rows)


def cells_reba_arm_block():
    tuples = list(itertools.product(range(6), range(2), range(3)))
    return _arm_cells(tuples, lambda p, s, t: _set_arm(p, s, _REBA_UA[s][t[0]], _LA[s][t[1]], _REBA_WR[t[2]]))


def cells_rula_arm_block():
    tuples = list(itertools.product(range(6), range(3), range(4), range(2)))
    return _arm_cells(tuples, lambda p, s, t: _set_arm(p, s, _RULA_UA[s][t[0]], _LA[s][t[1]], _RULA_WR[t[2]], _TWIST[t[3]]))


# ---- infos ------------------------------------------------------------------------------------------------------------
def make_info(reba=None, rula=None):
    r = dict.fromkeys(REBA_KEYS, 0)
    u = dict.fromkeys(RULA_KEYS, 0)
    r.update(reba or {})
    u.update(rula or {})
    assert set(r) == set(REBA_KEYS) and set(u) == set(RULA_KEYS)
    assert all(isinstance(v, int) and abs(v) <= 20 for v in list(r.values()) + list(u.values()))
    return {"REBA": r, "RULA": u}


def rule_infos():
    out = [make_info({"Sitting": s}) for s in (-1, 0, 1, 2)]
    for side in ("L", "R"):
        for v in (1, -1):
            out.append(make_info({f"Arm_supported_leaning_{side}": v}, {f"Arm_supported_leaning_{side}": v}))
    for v in (-1, 1, 2, 3, 4):          # legs 0 is the all-zero info, which Sitting = 0 already gave
        out.append(make_info({"Legs_bilateral_weight_bearing/walking": v}, {"Legs_bilateral_weight_bearing": v}))
    return out


def _rula_shift(a, b):
    """Both arms' group score by a (they meet in max()), the neck/trunk/leg group score by b."""
    return {"A_Load/Force_L": a, "A_Load/Force_R": a, "B_Load/Force": b}


def one_hot_infos():
    """Every field the rule infos leave alone, alone non-zero."""
    reba = [{"Load/Force Score": 1}, {"Coupling": 1}, {"Activity_Score": 1}, {"Load/Force Score": 2}, {"Coupling": 2},
            {"Activity_Score": 2}]
    rula = [{k: 1} for k in ("A_Muscle_use_L", "A_Muscle_use_R", "A_Load/Force_L", "A_Load/Force_R", "B_Muscle_use",
                             "B_Load/Force")]
    return [make_info(r, u) for r, u in zip(reba, rula)]


# (REBA Load/Force, REBA Coupling, RULA both arms, RULA group B) sums under which a one-off error in a table A / B entry
# moves the final score: table C's plateaus differ from table to table, so the shifts are plural (REBA C's columns 2 and 3
# are equal; RULA C's rows 6 and 7 differ in column 4 only, its columns 6 and 7 in row 3 only)
AB_SHIFTS = [(2, 0, 0, 0), (0, 0, 2, -2), (5, 1, 2, -3), (-2, 3, 3, 2), (1, 0, 1, 3), (3, 2, 5, 4)]
ARM_SHIFTS = [(0, 0, 0, 0), (2, 1, -3, 0), (5, 3, -3, 3), (8, -2, -2, 4), (1, 2, 2, 3), (0, -3, -4, 3), (3, 4, 0, 4),
              (1, 5, -5, 0)]


def _shift_info(s, legs=(0, 0)):
    ra, rb, ua, ub = s
    return make_info({"Load/Force Score": ra, "Coupling": rb, "Legs_bilateral_weight_bearing/walking": legs[0]},
                     dict(_rula_shift(ua, ub), Legs_bilateral_weight_bearing=legs[1]))


def ab_infos():
    """Table A / B cells: REBA's leg index 1..4 and RULA's 1..2 come from the legs fields."""
    return [_shift_info(s, (leg, 1 + leg % 2)) for leg in (1, 2, 3, 4) for s in AB_SHIFTS]


def arm_infos():
    return [_shift_info(s) for s in ARM_SHIFTS]


def corner_infos():
    """The baseline pose has group scores (1, 1) in both scorers: these carry it to every cell of both C tables, and one
    below and one above each clamp (REBA 0..13, RULA 0..8)."""
    out = []
    for i, (ra, rb) in enumerate(itertools.product(range(-1, 13), repeat=2)):
        out.append(make_info({"Load/Force Score": ra, "Coupling": rb, "Activity_Score": i % 3 - 1},
                             _rula_shift(i % 9 - 1, (i // 9) % 9 - 1)))
    return out


def build():
    blocks, poses, pos = {}, [], 0
    for name, fn in (("grid", grid_block), ("cross", cross_block), ("specials", specials_block),
                     ("cells_ab", cells_ab_block), ("cells_reba_arm", cells_reba_arm_block),
                     ("cells_rula_arm", cells_rula_arm_block), ("corner", baseline_pose)):
        p = fn()
        blocks[name] = (pos, pos + len(p))
        pos += len(p)
        poses.append(p)
    infos, pairs = [], []

    def run(block_names, new):
        for info in new:
            if info not in infos:
                infos.append(info)
            for b in block_names:
                if (b, infos.index(info)) not in pairs:
                    pairs.append((b, infos.index(info)))

    run(("grid", "cross", "specials"), rule_infos())
    cells = ("cells_ab", "cells_reba_arm", "cells_rula_arm")
    run(cells, one_hot_infos())
    run(("cells_ab",), ab_infos())
    run(("cells_reba_arm", "cells_rula_arm"), arm_infos())
    run(("corner",), corner_infos())
    return np.concatenate(poses), blocks, infos, pairs
