"""What the score-probe tests measure a set of (pose, info) rows by: which class every angle falls in, which table cells a
row reads, and which one-off table errors the rows would notice.  Written apart from tests/score_cases.py, which builds the
rows: the classifier looks an angle up (searchsorted / isin), it does not know how the builder made it."""
import numpy as np

from oracle import reba_ref, rula_ref, risk_tables
from oracle.risk_tables import J, REBA_INFO_KEYS, RULA_INFO_KEYS

TABLES = {"REBA A": risk_tables.REBA_A, "REBA B": risk_tables.REBA_B, "REBA C": risk_tables.REBA_C,
          "RULA A": risk_tables.RULA_A, "RULA B": risk_tables.RULA_B, "RULA C": risk_tables.RULA_C}
REBA_COLS = ("score", "trunk", "neck", "leg", "upper_arm L", "upper_arm R", "lower_arm L", "lower_arm R", "wrist L", "wrist R")
RULA_COLS = ("score", "upper_arm L", "upper_arm R", "lower_arm L", "lower_arm R", "wrist L", "wrist R", "wrist_twist L",
             "wrist_twist R", "neck", "trunk", "leg")


def classify(x, thresholds):
    """Class of every angle in x: 2i + 1 on the i-th threshold, 2i in the open interval below it, 2k above the last; -1 for
    NaN.  2k + 1 classes for k thresholds."""
    th = np.asarray(thresholds, np.float64)
    x = np.asarray(x, np.float64)
    c = 2 * np.searchsorted(th, x, side="left") + np.isin(x, th)
    return np.where(np.isnan(x), -1, c)


def class_tuples(pose, angles):
    """int[N, len(angles)]: the class of each (joint, axis, thresholds) angle in every row."""
    return np.stack([classify(pose[:, J[j], k], th) for j, k, th in angles], axis=1)


def n_classes(angles):
    return int(np.prod([2 * len(th) + 1 for _, _, th in angles]))


def reached(pose, angles):
    """How many of the angles' class combinations the rows reach."""
    t = class_tuples(pose, angles)
    return len(np.unique(t[(t >= 0).all(axis=1)], axis=0))


def flatten(pose, row_slices, infos):
    """One row per (pose, info): row_slices [(start, stop)] and infos [dict] of equal length ->
    (pose f64[M,24,3], reba info {key: int64[M]}, rula info {key: int64[M]}, first row of each pair int[P+1])."""
    idx = np.concatenate([np.arange(a, b) for a, b in row_slices])
    counts = [b - a for a, b in row_slices]
    rep = lambda scorer, keys: {k: np.repeat([int(i[scorer][k]) for i in infos], counts).astype(np.int64) for k in keys}
    return pose[idx], rep("REBA", REBA_INFO_KEYS), rep("RULA", RULA_INFO_KEYS), np.concatenate([[0], np.cumsum(counts)])


def take(info, rows):
    return {k: v[rows] for k, v in info.items()}


def cells_read(reba, rula, ri, ui):
    """{table: [index arrays, one per arm where the table is read twice]}: the cell(s) of each table that a row's lookups
    touch, restated from the packed sub-scores and the info fields."""
    r, u = np.asarray(reba, np.int64), np.asarray(rula, np.int64)
    A, B = TABLES["REBA A"], TABLES["REBA B"]
    a = (r[:, 1] - 1, r[:, 2] - 1, r[:, 3] - 1)
    bl, br = (r[:, 4] - 1, r[:, 6] - 1, r[:, 8] - 1), (r[:, 5] - 1, r[:, 7] - 1, r[:, 9] - 1)
    sa = np.clip(A[a] + ri["Load/Force Score"], 1, 12)
    sb = np.clip(np.maximum(B[bl], B[br]) + ri["Coupling"], 1, 12)
    out = {"REBA A": [a], "REBA B": [bl, br], "REBA C": [(sa - 1, sb - 1)]}
    A, B = TABLES["RULA A"], TABLES["RULA B"]
    al, ar = (u[:, 1] - 1, u[:, 3] - 1, u[:, 5] - 1, u[:, 7] - 1), (u[:, 2] - 1, u[:, 4] - 1, u[:, 6] - 1, u[:, 8] - 1)
    b = (u[:, 9] - 1, u[:, 10] - 1, u[:, 11] - 1)
    sa = np.clip(np.maximum(A[al] + ui["A_Muscle_use_L"] + ui["A_Load/Force_L"],
                            A[ar] + ui["A_Muscle_use_R"] + ui["A_Load/Force_R"]), 1, 7)
    sb = np.clip(B[b] + ui["B_Muscle_use"] + ui["B_Load/Force"], 1, 7)
    out.update({"RULA A": [al, ar], "RULA B": [b], "RULA C": [(sa - 1, sb - 1)]})
    return out


def readers(reads, table):
    """int[M, reads per row]: the flat number of the cell(s) of `table` that each row reads (two for the per-arm tables)."""
    shape = TABLES[table].shape
    return np.stack([np.ravel_multi_index(ix, shape) for ix in reads[table]], axis=1)


def unread_cells(reads, table):
    flat = readers(reads, table)
    seen = np.zeros(TABLES[table].size, bool)
    seen[flat.ravel()] = True
    return [tuple(int(v) for v in np.unravel_index(c, TABLES[table].shape)) for c in np.flatnonzero(~seen)]


def surviving_mutants(pose, ri, ui, reba, rula):
    """Every table entry changed by +1 and by -1 in turn (in the oracle's own arrays, put back afterwards): the mutants that
    leave every stored row as it is.  Only the rows that read the entry are evaluated again.
    -> {table: [(cell index, delta)]}"""
    reads = cells_read(reba, rula, ri, ui)
    out = {}
    for name, T in TABLES.items():
        is_reba = name.startswith("REBA")
        packed, info, want = (reba_ref.reba_packed, ri, reba) if is_reba else (rula_ref.rula_packed, ui, rula)
        flat = readers(reads, name)
        order = {c: np.flatnonzero((flat == c).any(axis=1)) for c in range(T.size)}
        alive = []
        for c in range(T.size):
            cell = np.unravel_index(c, T.shape)
            rows = order[c]
            for d in (1, -1):
                if len(rows) == 0:
                    alive.append((tuple(int(v) for v in cell), d))
                    continue
                keep = T[cell]
                T[cell] = keep + d
                try:
                    got = packed(pose[rows], take(info, rows))
                finally:
                    T[cell] = keep
                if np.array_equal(got, want[rows]):
                    alive.append((tuple(int(v) for v in cell), d))
        out[name] = alive
    return out


def first_difference(got, want, cols):
    """(row, column name) of the first differing entry, or None."""
    bad = np.argwhere(np.asarray(got) != np.asarray(want))
    return (int(bad[0, 0]), cols[int(bad[0, 1])]) if len(bad) else None
