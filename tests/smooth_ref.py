"""The contract of pr_smooth_tracks (include/poserisk_hip.h, section s1) restated in float64 numpy: what the kernel's outputs
are compared with.  Vectorised over rows, looping over window offsets in ascending order, so every sum is accumulated in the
order the contract names.  Membership is a SELECTION, never a zero weight: what a row that is no member holds -- another
track's NaN, an inf beyond a gap -- is not multiplied by anything and enters no sum (0.0 * nan would be nan); adding the
selected 0.0 leaves a sum's bits alone.  A row whose stage-2 window holds nobody else comes back as stage 1 left it, bit for
bit.  Non-finite members behave as the header says: a NaN cost is never smaller than anything (a window whose every cost is
NaN yields its first member), a joint whose c is not a number falls back, cam and betas propagate.

    smooth(rotmat, frame_no, track_start, m, sigma, betas=None, cam=None) -> dict
        rotmat, betas, cam   with sigma > 0 float64 (the values before the one rounding to f32), else float32 (an input row's bits)
        status i32[N], replaced i32[N]
        stage1               dict(rotmat, betas, cam) float32: stage 1's outputs
        ties                 per tensor: (best cost, second-best cost, second-best row) of every stage-1 item, for the census
        c                    f64[N,24]: the fallback measure of every joint (sigma > 0)
"""
import math

import numpy as np

MAX_RADIUS = 15
FALLBACK_C = 0.05


def gaussian_radius(sigma):
    return int(min(math.ceil(3.0 * sigma), MAX_RADIUS)) if sigma > 0 else 0


def check_arguments(N, track_start, m, sigma):
    ts = np.asarray(track_start)
    assert 0 <= int(m) <= MAX_RADIUS and math.isfinite(sigma) and sigma >= 0
    assert ts.ndim == 1 and len(ts) >= 1 and ts[0] == 0 and ts[-1] == N and np.all(np.diff(ts) >= 0)


def track_bounds(track_start, N):
    """-> (lo i64[N], hi i64[N]): the rows of row i's track are lo[i] .. hi[i] - 1."""
    ts = np.asarray(track_start, np.int64)
    t = np.searchsorted(ts, np.arange(N), side="right") - 1
    return ts[t], ts[t + 1]


def members(frame_no, lo, hi, r):
    """-> (rows k = i + o as i64[N, 2r+1], clipped into the tensor; member bool[N, 2r+1]; |frame difference| i64[N, 2r+1])."""
    N = len(frame_no)
    f = np.asarray(frame_no, np.int64)
    k = np.arange(N)[:, None] + np.arange(-r, r + 1)[None, :]
    inside = (k >= lo[:, None]) & (k < hi[:, None])
    kc = np.clip(k, 0, max(N - 1, 0))
    df = np.abs(f[kc] - f[:, None])
    return kc, inside & (df <= r), df


def medoid(x, frame_no, lo, hi, r):
    """x f32[N,G,D] -> (chosen row i64[N,G], best cost, second-best cost, second-best row)."""
    N, G, D = x.shape
    X = x.astype(np.float64)
    kc, mem, df = members(frame_no, lo, hi, r)
    W = 2 * r + 1

    def dist(ka, kb):                                   # ||x_ka - x_kb|| per group, the squares summed in element order
        ss = np.zeros((N, G))
        with np.errstate(invalid="ignore"):             # (inf - inf where a row holds an inf)
            for e in range(D):
                d = X[ka, :, e] - X[kb, :, e]
                ss = ss + d * d
        return np.sqrt(ss)
    best = np.full((N, G), -1, np.int64)
    best_cost = np.full((N, G), np.inf)
    best_df = np.zeros((N, G), np.int64)
    second_cost = np.full((N, G), np.inf)
    second = np.full((N, G), -1, np.int64)
    for ok in range(W):
        cost = np.zeros((N, G))
        for ol in range(W):
            cost = cost + np.where(mem[:, ol, None], dist(kc[:, ok], kc[:, ol]), 0.0)
        is_mem = mem[:, ok, None]
        dfk = df[:, ok, None]
        better = is_mem & ((best < 0) | (cost < best_cost) | ((cost == best_cost) & (dfk < best_df)))
        # the runner-up: the old best where it is beaten, else this candidate where it beats the old runner-up
        demoted = better & (best >= 0)
        runner = is_mem & ~better & (cost < second_cost)
        second_cost = np.where(demoted, best_cost, np.where(runner, cost, second_cost))
        second = np.where(demoted, best, np.where(runner, kc[:, ok, None], second))
        best = np.where(better, kc[:, ok, None], best)
        best_cost = np.where(better, cost, best_cost)
        best_df = np.where(better, dfk, best_df)
    return best, best_cost, second_cost, second


def polar_svd(A):
    """The rotation nearest each A[..., 3, 3] in Frobenius norm: U diag(1, 1, det(U V^T)) V^T."""
    U, _, Vt = np.linalg.svd(A)
    d = np.linalg.det(U @ Vt)
    S = np.zeros(A.shape)
    S[..., 0, 0] = S[..., 1, 1] = 1.0
    S[..., 2, 2] = d
    return U @ S @ Vt


def fallback_measure(A):
    s = np.sqrt((A * A).sum((-1, -2))) / math.sqrt(3.0)
    with np.errstate(all="ignore"):
        return np.linalg.det(A) / (s * s * s)


def weights(frame_no, lo, hi, g, sigma):
    kc, mem, df = members(frame_no, lo, hi, g)
    with np.errstate(all="ignore"):
        w = np.where(df == 0, 1.0, np.exp(-(df * df).astype(np.float64) / (2.0 * sigma * sigma)))
    return kc, mem, w


def smooth(rotmat, frame_no, track_start, m, sigma, betas=None, cam=None):
    rotmat = np.ascontiguousarray(rotmat, np.float32)
    N = rotmat.shape[0]
    check_arguments(N, track_start, m, sigma)
    lo, hi = track_bounds(track_start, N)
    tensors = {"rotmat": rotmat.reshape(N, 24, 9)}
    if cam is not None:
        tensors["cam"] = np.ascontiguousarray(cam, np.float32).reshape(N, 1, 3)
    if betas is not None:
        tensors["betas"] = np.ascontiguousarray(betas, np.float32).reshape(N, 1, 10)
    bit0 = {"rotmat": 0, "cam": 24, "betas": 25}
    out = {"rotmat": None, "betas": None, "cam": None, "status": np.zeros(N, np.int32), "replaced": np.zeros(N, np.int32),
           "stage1": {}, "ties": {}, "c": None}
    rows = np.arange(N)
    for name, x in tensors.items():                                          # stage 1
        if m > 0 and N:
            pick, c1, c2, k2 = medoid(x, frame_no, lo, hi, m)
            y = np.take_along_axis(x, pick[:, :, None], axis=0)
            out["ties"][name] = (c1, c2, k2, pick)
            for j in range(x.shape[1]):
                out["replaced"] |= ((pick[:, j] != rows).astype(np.int32) << (bit0[name] + j))
        else:
            y = x.copy()
        out["stage1"][name] = y
    g = gaussian_radius(sigma)
    for name, y in out["stage1"].items():                                    # stage 2
        if sigma > 0 and N:
            kc, mem, w = weights(frame_no, lo, hi, g, sigma)
            Y = y.astype(np.float64)
            acc, wsum = np.zeros(Y.shape), np.zeros(N)
            for o in range(2 * g + 1):
                is_mem = mem[:, o]
                with np.errstate(invalid="ignore"):                          # (0 * inf where a member holds an inf)
                    acc = acc + np.where(is_mem[:, None, None], w[:, o, None, None] * Y[kc[:, o]], 0.0)
                wsum = wsum + np.where(is_mem, w[:, o], 0.0)
            if name == "rotmat":
                A = acc.reshape(N, 24, 3, 3)
                c = fallback_measure(A)
                fell = ~(c >= FALLBACK_C)
                R = polar_svd(np.where(fell[..., None, None], np.eye(3), A))
                res = np.where(fell[..., None, None], Y.reshape(N, 24, 3, 3), R).reshape(N, 24, 9)
                for j in range(24):
                    out["status"] |= fell[:, j].astype(np.int32) << j
                out["c"] = c
            else:
                with np.errstate(invalid="ignore"):
                    res = acc / wsum[:, None, None]
            alone = mem.sum(1) == 1                                          # an isolated row comes back as it is
            res = np.where(alone[:, None, None], Y, res)
        else:
            res = y
        out[name] = res.reshape((N, 24, 3, 3) if name == "rotmat" else (N, res.shape[2]))
        out["stage1"][name] = y.reshape(out[name].shape)
    return out
