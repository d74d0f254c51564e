"""The contract of pr_activity_tracks (include/poserisk_hip.h, section t1) restated in float64 numpy: what the kernel's outputs
must EQUAL.  Every output is an integer and every comparison is made on a float64 number that is computed here by the same
operations in the same order, so there is no tolerance.  Nothing here is fast or clever: every dot of every window is taken,
nothing stops early."""
from concurrent.futures import ThreadPoolExecutor

import numpy as np

JOINT_NAMES = ("Torso", "Neck", "L_Knee", "R_Knee", "L_Thorax", "L_Shoulder", "L_Elbow", "L_Wrist", "R_Thorax", "R_Shoulder",
               "R_Elbow", "R_Wrist")
JOINT_INDEX = (3, 12, 4, 5, 13, 16, 18, 20, 14, 17, 19, 21)
MASK_B, MASK_L, MASK_R = 0x00f, 0x0f0, 0xf00
_BITS = (1 << np.arange(12)).astype(np.int64)


def dots(a, b):
    """sum over e = 0..8, ascending, of a[..., e] * b[..., e] in float64, each addition rounded on its own."""
    acc = a[..., 0] * b[..., 0]
    for e in range(1, 9):
        acc = acc + a[..., e] * b[..., e]
    return acc


def scored(rotmat):
    """f32[N,24,3,3] -> f64[N,12,9]: the scored joints in bit order (float32 -> float64 is exact)."""
    return np.asarray(rotmat, np.float32).reshape(-1, 24, 9)[:, list(JOINT_INDEX)].astype(np.float64)


def dot_pair(rotmat, k, i, b):
    """dot_b(k, i) as the contract computes it."""
    x = scored(rotmat)
    return float(dots(x[k, b], x[i, b]))


def window(f, i, first, L):
    """W_i(L): the rows k of the track starting at `first` with k <= i, i - k <= L and 0 <= f[i] - f[k] <= L, ascending."""
    ks = np.arange(max(i - L, first), i + 1)
    df = f[i] - f[ks]
    return ks[(df >= 0) & (df <= L)]


def events(x, f, first, end, G, dot_move, moved):
    """Stage A of one track, in place into moved i32[N]."""
    if end <= first:
        return
    anchor = x[first].copy()
    for k in range(first + 1, end):
        step = f[k] - f[k - 1]
        if step > G or step < 0:
            anchor = x[k].copy()
            continue
        with np.errstate(invalid="ignore"):
            ev = dots(anchor, x[k]) < dot_move
        moved[k] = int(_BITS[ev].sum())
        anchor[ev] = x[k][ev]


def row_masks(x, f, moved, i, first, H, R, G, E, dot_static, dot_rapid):
    """Stage B of row i -> (held, repeated, rapid) masks."""
    mem = window(f, i, first, H)
    fm = f[mem]
    steps = np.diff(fm)
    covered = bool(f[i] - fm[0] > H - G) and bool(np.all((steps >= 1) & (steps <= G)))
    d = dots(x[mem], x[i][None])                                  # [members, 12]
    with np.errstate(invalid="ignore"):
        still = np.all(d >= dot_static, axis=0)
        in_r = (i - mem <= R) & (f[i] - fm <= R)
        rapid = np.any(d[in_r] < dot_rapid, axis=0)
    count = ((moved[mem].astype(np.int64)[:, None] >> np.arange(12)) & 1).sum(axis=0)
    held = int(_BITS[still].sum()) if covered else 0
    repeated = int(_BITS[count > E].sum()) if covered else 0
    return held, repeated, int(_BITS[rapid].sum())


def activity(rotmat, frame_no, track_start, H, R, G, E, dot_static, dot_move, dot_rapid, threads=1):
    """-> dict(flags i32[N,4] = held, repeated, rapid, moved; adds i32[N,4] = reba_activity, a_muscle_l, a_muscle_r, b_muscle;
    stage_b i32[N,2] = held and repeated before stage C spreads them)."""
    x = scored(rotmat)
    f = np.asarray(frame_no).astype(np.int64)
    ts = np.asarray(track_start).astype(np.int64)
    N = len(f)
    assert x.shape[0] == N and ts[0] == 0 and ts[-1] == N and np.all(np.diff(ts) >= 0)
    moved = np.zeros(N, np.int32)
    first_of = np.zeros(N, np.int64)
    end_of = np.zeros(N, np.int64)
    for first, end in zip(ts[:-1], ts[1:]):
        events(x, f, int(first), int(end), G, dot_move, moved)
        first_of[first:end], end_of[first:end] = first, end
    stage_b = np.zeros((N, 3), np.int32)

    def some_rows(rows):
        for i in rows:
            stage_b[i] = row_masks(x, f, moved, i, int(first_of[i]), H, R, G, E, dot_static, dot_rapid)
    if threads > 1 and N:
        with ThreadPoolExecutor(threads) as pool:
            list(pool.map(some_rows, np.array_split(np.arange(N), threads * 8)))
    else:
        some_rows(range(N))
    flags = np.zeros((N, 4), np.int32)
    for i in range(N):                                            # stage C
        es = np.arange(i, min(i + H, int(end_of[i]) - 1) + 1)
        df = f[es] - f[i]
        sel = es[(df >= 0) & (df <= H)]
        flags[i, 0] = np.bitwise_or.reduce(stage_b[sel, 0])
        flags[i, 1] = np.bitwise_or.reduce(stage_b[sel, 1])
    flags[:, 2] = stage_b[:, 2]
    flags[:, 3] = moved
    return dict(flags=flags, adds=adds_of(flags), stage_b=stage_b[:, :2].copy())


def adds_of(flags):
    held, repeated, rapid = flags[:, 0], flags[:, 1], flags[:, 2]
    loaded = held | repeated
    return np.stack([(held != 0).astype(np.int32) + (repeated != 0) + (rapid != 0), (loaded & MASK_L) != 0, (loaded & MASK_R) != 0,
                     (loaded & MASK_B) != 0], axis=1).astype(np.int32)
