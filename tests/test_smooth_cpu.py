"""Temporal smoothing without a GPU: the numpy restatement of the contract (tests/smooth_ref.py) against brute-force
definitions, the near-tie census of the committed cases, the argument errors of smooth.smooth_tracks and of the C entry, the
binding, the knobs, and that with both knobs at 0 the scoring pass never reaches the smoothing code."""
import ctypes as C
import json
import math
import os
import re
import types

import numpy as np
import pytest
import torch

import smooth_cases as sc
import smooth_ref
from conftest import REPO
from poserisk_release_amd import _lib, dropin, smooth

dropin.install()
from core import base  # noqa: E402
from core.config import cfg  # noqa: E402


# ---- the reference against brute force ------------------------------------------------------------------------------------
def test_a_one_float_medoid_is_scipys_median_filter_on_full_windows():
    from scipy.ndimage import median_filter
    rng = np.random.default_rng(1)
    x = rng.standard_normal((97, 4)).astype(np.float32)
    frame_no, lo, hi = np.arange(97), np.zeros(97, np.int64), np.full(97, 97, np.int64)
    for m in (1, 2, 5, 15):
        pick, _, _, _ = smooth_ref.medoid(x[:, :, None], frame_no, lo, hi, m)
        got = np.take_along_axis(x, pick, axis=0)
        want = median_filter(x, size=(2 * m + 1, 1), mode="nearest")
        assert np.array_equal(got[m:-m], want[m:-m]), m          # odd full windows: the medoid of scalars is THE median
        assert (pick[m:-m] != np.arange(97)[m:-m, None]).any()


def _brute_force(c):
    """The contract, item by item, in plain loops: windows from their definition, costs and sums in the order it names, the polar
    factor from numpy's SVD."""
    N = len(c["frame_no"])
    f, ts = c["frame_no"].astype(np.int64), c["track_start"]
    m, sigma = c["m"], c["sigma"]
    g = smooth_ref.gaussian_radius(sigma)
    track = np.searchsorted(ts, np.arange(N), side="right") - 1

    def window(i, r):
        return [k for k in range(max(i - r, 0), min(i + r, N - 1) + 1) if track[k] == track[i] and abs(f[k] - f[i]) <= r]
    out, status = {}, np.zeros(N, np.int32)
    for key, G in (("rotmat", 24), ("cam", 1), ("betas", 1)):
        if c[key] is None:
            continue
        x = c[key].reshape(N, G, -1)
        D = x.shape[2]
        y = x.copy()
        if m > 0:
            for i in range(N):
                w = window(i, m)
                for j in range(G):
                    best = None
                    for k in w:
                        cost = 0.0
                        for l in w:
                            ss = 0.0
                            for e in range(D):
                                d = float(x[k, j, e]) - float(x[l, j, e])
                                ss = ss + d * d
                            cost = cost + math.sqrt(ss)
                        key_k = (cost, abs(int(f[k] - f[i])), k)
                        if best is None or key_k < best:
                            best = key_k
                    y[i, j] = x[best[2], j]
        res = y.astype(np.float64)
        if sigma > 0:
            for i in range(N):
                w = window(i, g)
                if len(w) == 1:
                    continue
                wt = [math.exp(-float((f[k] - f[i]) ** 2) / (2.0 * sigma * sigma)) for k in w]
                for j in range(G):
                    acc, wsum = np.zeros(D), 0.0
                    for k, wk in zip(w, wt):
                        acc = acc + wk * y[k, j].astype(np.float64)
                        wsum = wsum + wk
                    if key != "rotmat":
                        res[i, j] = acc / wsum
                        continue
                    A = acc.reshape(3, 3)
                    cval = np.linalg.det(A) / (np.linalg.norm(A) / math.sqrt(3.0)) ** 3
                    if not cval >= 0.05:
                        status[i] |= 1 << j
                        continue
                    U, _, Vt = np.linalg.svd(A)
                    res[i, j] = (U @ np.diag([1.0, 1.0, np.linalg.det(U @ Vt)]) @ Vt).reshape(9)
        out[key] = res.reshape(c[key].shape)
    return out, status


@pytest.mark.parametrize("name", ["short_m2_s1.5", "gaps_m2_s1.5", "gaps_m3_s0", "tile+1", "fallback_m0_s50", "outlier_m2_s1.5",
                                  "wild_m2_s1.5", "wild_m3_s0", "sigma_third_up2", "knife_c_below", "nonfinite_m2_s0", "nonfinite_m0_s1.5",
                                  "nonfinite_m2_s1.5"])
def test_the_vectorised_reference_is_the_contract_item_by_item(name):
    """(The loops below never multiply a row that is no member by anything, and their tuple comparison keeps the first member
    where a cost is NaN: the header's words on non-finite values, which the vectorised reference has to reproduce.)"""
    c, ref = sc.case(name), sc.reference(name)
    with np.errstate(invalid="ignore"):
        want, status = _brute_force(c)
    assert np.array_equal(ref["status"], status)
    for key, v in want.items():
        if c["sigma"] == 0:
            assert np.array_equal(sc.bits(ref[key]), sc.bits(v)), key
        else:
            # two float64 evaluations of the same sums (the batched SVD against one matrix at a time); NaNs compare as equal
            same = (np.isnan(ref[key]) & np.isnan(v)) | (ref[key] == v)
            with np.errstate(invalid="ignore"):
                off = np.where(same, 0.0, np.abs(ref[key] - v))
            assert (off <= 1e-13 * max(1.0, float(np.abs(v[np.isfinite(v)]).max()))).all(), key
    # what comes out of stage 2 is a rotation
    if c["sigma"] > 0 and c["rotations"]:
        R = ref["rotmat"]
        assert np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() < 1e-6 and np.linalg.det(R).min() > 0.999


def test_scaled_newton_agrees_with_the_svd_on_a_jittery_track():
    """The device's iteration, restated: from A / (||A||_F / sqrt 3), X <- (mu X + X^-T / mu) / 2, against the SVD's factor."""
    ref = sc.reference("mixed_m0_s1.5")
    c = sc.case("mixed_m0_s1.5")
    kc, mem, w = smooth_ref.weights(c["frame_no"], *smooth_ref.track_bounds(c["track_start"], len(c["frame_no"])), 5, 1.5)
    A = (np.where(mem, w, 0.0)[:, :, None, None, None] * c["rotmat"].astype(np.float64)[kc]).sum(1)
    assert ref["c"].min() > 0.9
    X = A / (np.sqrt((A * A).sum((-1, -2), keepdims=True)) / math.sqrt(3.0))
    for _ in range(12):
        inv_t = np.swapaxes(np.linalg.inv(X), -1, -2)
        mu = np.abs(np.linalg.det(X))[..., None, None] ** (-1.0 / 3.0)
        X = 0.5 * (mu * X + inv_t / mu)
    assert np.abs(X - smooth_ref.polar_svd(A)).max() < 1e-13


# ---- the committed cases ------------------------------------------------------------------------------------------------------
def test_the_committed_cases_hold_no_near_tie_and_what_they_claim():
    smallest = np.inf
    for name in sc.NAMES:
        ref = sc.reference(name)
        near, items = sc.near_ties(ref)
        assert sum(int(v.sum()) for v in near.values()) == 0, name
        smallest = min(smallest, sc.smallest_gap(ref))
        c = sc.case(name)
        assert len(c["frame_no"]) <= (2500 if name.startswith("many_") else 600)
        sc.check(name, {k: (None if ref[k] is None else ref[k].astype(np.float32) if k in ("rotmat", "betas", "cam") else ref[k])
                        for k in ("rotmat", "betas", "cam", "status", "replaced")})       # the reference passes its own check
    assert smallest > 1e-7, smallest                                      # far from the 1e-9 under which an item may be left out
    fb = sc.reference("fallback_m0_s50")
    # 2e-8, and for +-60 degrees 12 / (17 / 3)^1.5 = 0.89: neither near 0.05
    assert 1e-8 < fb["c"][1, 5] < 4e-8 and 0.88 < fb["c"][1, 7] < 0.90
    assert fb["status"][:3].tolist() == [1 << 5] * 3 and not fb["status"][3:].any()
    for name in sc.NAMES:                                                  # no other case sits near the threshold
        cc = sc.reference(name)["c"]
        if cc is not None and not name.startswith("knife_c_"):             # (those do, on purpose: see below)
            assert not ((cc > 0.005) & (cc < 0.5)).any(), name
    out = sc.case("outlier_m1_s0")
    row, j = out["outlier"]
    assert sc.reference("outlier_m1_s0")["replaced"][row] >> j & 1
    sizes = {len(sc.case(n)["frame_no"]) for n in sc.NAMES}
    assert {sc.TILE - 1, sc.TILE, sc.TILE + 1, 2 * sc.TILE + 1} <= sizes
    assert {(sc.CASES[n][1] > 0, sc.CASES[n][2] > 0) for n in sc.NAMES} == {(False, False), (True, False), (False, True), (True, True)}
    assert smooth_ref.gaussian_radius(5.0) == 15 == smooth.gaussian_radius(5.0) and smooth.gaussian_radius(1.5) == 5
    assert smooth.gaussian_radius(0.0) == 0 and smooth.gaussian_radius(1e9) == 15


def test_the_wild_many_and_sigma_cases_are_what_they_are_for():
    lo, hi = np.iinfo(np.int32).min, np.iinfo(np.int32).max
    for name in ("wild_m2_s1.5", "wild_m15_s5", "wild_m3_s0", "wild_m0_s2"):
        c = sc.case(name)
        assert len(c["track_start"]) - 1 == 3
        for a, b in zip(c["track_start"][:-1], c["track_start"][1:]):
            f = c["frame_no"][a:b].astype(np.int64)
            d = np.diff(f)
            assert f.min() == lo and f.max() == hi and len(np.unique(f)) < len(f)                   # the extremes, duplicates
            assert (d[8:17] <= 0).all() and (d[8:17] < 0).any() and (d[20:27] == 0).all()            # descending, constant
    for name in ("wild_m2_s1.5", "wild_m3_s0"):
        # the second tie rule: the last row and the one before it share a frame number and the window, their costs are one
        # number (a pair's distance, taken twice), and the smaller row wins every group
        c, ref = sc.case(name), sc.reference(name)
        i = sc.WILD_TIE_ROW
        assert c["frame_no"][i] == c["frame_no"][i - 1] and ref["replaced"][i] == (1 << 26) - 1
        for c1, c2, second, pick in ref["ties"].values():
            assert (pick[i] == i - 1).all() and (second[i] == i).all() and (c1[i] == c2[i]).all()
    for name in ("many_m2_s1.5", "many_m15_s5"):
        c = sc.case(name)
        ts = c["track_start"]
        lengths = np.diff(ts)
        assert len(lengths) >= 300 and lengths.min() == 0 and lengths.max() == 12 and len(np.unique(lengths)) == 13
        assert len(ts) - 1 > 256 and ts[256] % sc.TILE != 0 and ts[256] < ts[-1]           # the second launch starts inside a tile
        steps = np.concatenate([np.diff(c["frame_no"][a:b]) for a, b in zip(ts[:-1], ts[1:])])
        assert (steps > 1).any() and (steps > 15).any()
    radii = {"1e-200": 1, "1e300": 15, "1e-3": 1, "third": 1, "third_up": 1, "third_up2": 2, "1": 3, "1_up": 4, "4.999999999": 15, "5": 15}
    assert set(radii) == set(sc.SIGMAS)
    for label, want in radii.items():
        sigma = sc.SIGMAS[label]
        assert smooth_ref.gaussian_radius(sigma) == want == smooth.gaussian_radius(sigma), label
        c = sc.case(f"sigma_{label}")
        assert c["m"] == 0 and c["sigma"] == sigma and (np.diff(c["frame_no"][:60]) > 1).sum() >= 5          # a track with gaps
        assert sc.reference(f"sigma_{label}")["status"].sum() == 0
    third = sc.SIGMAS["third"]
    assert sc.SIGMAS["third_up"] == np.nextafter(third, 1.0) and sc.SIGMAS["third_up2"] == np.nextafter(sc.SIGMAS["third_up"], 1.0)
    assert 3.0 * sc.SIGMAS["third_up"] == 1.0 < 3.0 * sc.SIGMAS["third_up2"]                # radius 1 -> 2 across 1/3 ...
    assert sc.SIGMAS["1_up"] == np.nextafter(1.0, 2.0)                                      # ... 3 -> 4 across 1, 15 on both sides of 5
    assert (2.0 * 1e-200) * 1e-200 == 0.0 and (2.0 * 1e300) * 1e300 == np.inf               # sigma^2 underflows / overflows
    # the radius decides: behind the step of 2 frames cam is a thousand times larger, and a radius-2 window reaches across it
    r1, r2 = sc.reference("sigma_third_up")["cam"], sc.reference("sigma_third_up2")["cam"]
    row = sc.SIGMA_GAP_ROW - 1
    assert np.abs(r2[row] - r1[row]).max() > 100 * sc.ROT_TOL * np.abs(r1[row]).max()


def test_the_knife_edge_cases_sit_on_the_fallback_threshold():
    assert abs(sc.knife_theta() - 168.631) < 1e-3
    for name, side in (("knife_c_below", -1), ("knife_c_above", +1)):
        c, ref = sc.case(name), sc.reference(name)
        for row in (0, 1):
            rel = ref["c"][row, sc.KNIFE_JOINT] / smooth_ref.FALLBACK_C - 1.0
            assert 1e-9 <= side * rel <= 1e-3, (name, row, rel)          # on the named side, nearer than 1e-3, farther than 1e-9
            assert bool(ref["status"][row] >> sc.KNIFE_JOINT & 1) == (side < 0)
        assert (c["fallback"], c["no_fallback"]) == (([(0, sc.KNIFE_JOINT), (1, sc.KNIFE_JOINT)], []) if side < 0 else ([], [(0, sc.KNIFE_JOINT), (1, sc.KNIFE_JOINT)]))
        assert ref["status"][2:].sum() == 0
    c, ref = sc.case("knife_c_newton"), sc.reference("knife_c_newton")
    cc = ref["c"][:3, sc.KNIFE_JOINT]
    assert ((cc >= 0.05) & (cc <= 0.06)).all() and not ref["status"].any() and len(c["no_fallback"]) == 3
    R = ref["rotmat"][:3, sc.KNIFE_JOINT]                                  # the SVD's factor is a rotation at the ill-conditioned end too
    assert np.abs(R @ np.swapaxes(R, -1, -2) - np.eye(3)).max() < 1e-12 and np.linalg.det(R).min() > 0.999999


def test_non_finite_values_stay_inside_the_windows_that_hold_them():
    plant = sc.NONFINITE
    for name in ("nonfinite_m2_s0", "nonfinite_m0_s1.5", "nonfinite_m2_s1.5"):
        c, ref = sc.case(name), sc.reference(name)
        assert not c["rotations"] and c["track_start"].tolist() == [0, 40, 85, 115]
        f = c["frame_no"].astype(np.int64)
        assert f[20] - f[19] == 20 and f[65] - f[64] == 20                      # the gaps, wider than any radius
        for row in plant["rows"]:
            assert all(np.isnan(c[k][row]).all() for k in ("rotmat", "betas", "cam"))
        clean = sc.nonfinite_clean_rows(c)
        # the rows directly on the other side of each gap and boundary are clean, and a good part of every track is
        assert clean[[20, 40, 64, 84]].all() and not clean[list(plant["rows"])].any() and clean.sum() >= 40
        for key in ("rotmat", "betas", "cam"):
            assert np.isfinite(np.asarray(ref[key])[clean]).all(), (name, key)
            assert np.isfinite(ref["stage1"][key][clean]).all(), (name, key)
        assert not ref["status"][clean].any()
        if c["sigma"] > 0 and c["m"] == 0:
            row, j = plant["joint"]                                           # a NaN joint: its bit, on the rows whose window holds it
            want = np.zeros(len(f), bool)
            want[row - 5:row + 6] = True
            far = slice(91, len(f))                                           # (beyond the reach of the NaN row 85)
            assert np.array_equal((ref["status"][far] >> j & 1).astype(bool), want[far]) and (ref["status"][far] & ~(1 << j) == 0).all()
            row, e = plant["cam"]                                             # an inf in cam: propagated, no status bit for it
            assert np.isinf(ref["cam"][row, e]) and not np.isfinite(ref["cam"][row - 5:row + 6, e]).any()
            assert np.isfinite(ref["cam"][row + 6, e]) and np.isfinite(np.delete(ref["cam"][row], e)).all()
    # a window whose every cost is NaN yields its first member in row order: row 39 is NaN, so row 38's window 36 .. 39 gives 36
    ref = sc.reference("nonfinite_m2_s0")
    assert (ref["ties"]["rotmat"][3][38] == 36).all() and np.isnan(ref["ties"]["rotmat"][0][38]).all()


def test_the_sweep_draws_every_kind_of_problem_and_holds_no_near_tie():
    kinds, wild, absent = set(), 0, set()
    for name in sc.SWEEP_NAMES:
        c, ref = sc.case(name), sc.reference(name)
        near, _ = sc.near_ties(ref)
        assert sum(int(v.sum()) for v in near.values()) == 0, name
        assert 0 <= c["m"] <= 15 and 0 <= c["sigma"] <= 6 and 1 <= len(c["track_start"]) - 1 <= 4 and np.diff(c["track_start"]).max() <= 80
        kinds.add((c["m"] > 0, c["sigma"] > 0))
        absent.add((c["betas"] is None, c["cam"] is None))
        wild += int((c["frame_no"] == np.iinfo(np.int32).min).any())
        sc.check(name, {k: (None if ref[k] is None else ref[k].astype(np.float32) if k in ("rotmat", "betas", "cam") else ref[k])
                        for k in ("rotmat", "betas", "cam", "status", "replaced")})
    assert len(kinds) >= 3 and len(absent) == 4 and wild >= 5 and len(sc.SWEEP_NAMES) == 60


# ---- argument errors, before any device call -----------------------------------------------------------------------------------
def test_smooth_tracks_refuses_bad_arguments_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error must not reach the library"))
    rot, fno, ts = torch.zeros((5, 24, 3, 3)), np.arange(5), [0, 3, 5]
    ok = dict(rotmat=rot, frame_no=fno, track_start=ts, median_radius=2, sigma=1.5)
    for over, word in ((dict(median_radius=-1), "median_radius"), (dict(median_radius=16), "0..15"), (dict(median_radius=1.5), "integer"),
                       (dict(median_radius=True), "integer"), (dict(sigma=-0.1), "sigma"), (dict(sigma=float("nan")), "sigma"),
                       (dict(sigma=float("inf")), "sigma"), (dict(rotmat=torch.zeros((5, 24, 3))), r"float32\[N,24,3,3\]"),
                       (dict(rotmat=rot.double()), "float32"), (dict(betas=torch.zeros((5, 9))), "betas"), (dict(betas=torch.zeros((4, 10))), "4 rows"),
                       (dict(cam=torch.zeros((5, 4))), "cam"), (dict(track_start=[0, 3]), "s_T = N"), (dict(track_start=[1, 5]), "0 = s_0"),
                       (dict(track_start=[0, 4, 3, 5]), "<="), (dict(track_start=[[0, 5]]), "1-D"), (dict(track_start=[0.0, 5.0]), "integer"),
                       (dict(frame_no=np.arange(4)), "frame_no"), (dict(frame_no=np.arange(5.0)), "integer"),
                       (dict(frame_no=np.arange(5) + 2 ** 31), "int32")):
        with pytest.raises(ValueError, match=word):
            smooth.smooth_tracks(**{**ok, **over})
    with pytest.raises(TypeError, match="torch tensor"):
        smooth.smooth_tracks(**{**ok, "rotmat": rot.numpy()})
    with pytest.raises(_lib.PoseRiskHipError, match="on the GPU"):        # all else being right, a CPU tensor: there is no CPU path
        smooth.smooth_tracks(**ok)


def test_the_symbols_are_declared_and_bound_and_the_abi_is_16():
    header = open(os.path.join(REPO, "include", "poserisk_hip.h")).read()
    declared = set(re.findall(r"\b(pr_smooth_\w+)\s*\(", header))
    assert declared == {"pr_smooth_tile_rows", "pr_smooth_workspace_bytes", "pr_smooth_tracks"}
    assert declared <= set(_lib.SIGNATURES) and _lib.ABI_VERSION == 16
    assert "/* s1 " in header and "PR_SMOOTH_MAX_RADIUS 15" in header
    for struct, cls in (("pr_smooth_params", _lib.SmoothParams), ("pr_smooth_inputs", _lib.SmoothInputs), ("pr_smooth_outputs", _lib.SmoothOutputs)):
        fields = re.search(r"typedef struct %s \{(.*?)\}" % struct, header, re.S).group(1)
        names = re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", fields))
        assert names == [n for n, _ in cls._fields_], struct
    assert C.sizeof(_lib.SmoothParams) == 16
    lib = _lib.load()
    assert lib.pr_abi_version() == 16 and lib.pr_smooth_tile_rows() == sc.TILE
    assert lib.pr_smooth_workspace_bytes(-1, 1, 1) == 0 and lib.pr_smooth_workspace_bytes(100, 1, 1) >= 100 * 229 * 4
    assert lib.pr_smooth_workspace_bytes(100, 0, 0) >= 100 * 216 * 4 and lib.pr_smooth_workspace_bytes(100, 1, 1) % 256 == 0
    # the argument checks return before any device work (no GPU here)
    fake, starts = 256, (C.c_int * 3)(0, 3, 5)
    ins, outs = _lib.SmoothInputs(fake, None, None), _lib.SmoothOutputs(fake + 8192, None, None, None)

    def call(m=2, sigma=1.5, ins=ins, outs=outs, fno=fake + 4096, starts=starts, T=2, N=5, status=None, ws=fake + 65536):
        rc = lib.pr_smooth_tracks(C.byref(_lib.SmoothParams(m, 0, sigma)), C.byref(ins), fno, starts, T, N, C.byref(outs), status, ws, None)
        return rc, lib.pr_last_error().decode()
    for over, word in ((dict(m=16), "median_radius"), (dict(m=-1), "median_radius"), (dict(sigma=-1.0), "sigma"), (dict(sigma=float("nan")), "sigma"),
                       (dict(N=-1), "N = -1"), (dict(T=-1), "T = -1"), (dict(starts=(C.c_int * 3)(0, 4, 3)), "track_start"),
                       (dict(starts=(C.c_int * 3)(0, 3, 6)), "not N"), (dict(starts=None), "null track_start"), (dict(fno=None), "null"),
                       (dict(ws=None), "workspace"), (dict(outs=_lib.SmoothOutputs(fake, None, None, None)), "aliases"),
                       (dict(ins=_lib.SmoothInputs(fake, fake + 64, None)), "betas"), (dict(status=fake + 8192), "share")):
        rc, msg = call(**over)
        assert rc == -1 and word in msg and "pr_smooth_tracks" in msg, (over, rc, msg)
    assert lib.pr_smooth_tracks(None, None, None, None, 0, 0, None, None, None, None) == -1
    assert call(N=0, T=0, starts=(C.c_int * 1)(0))[0] == 0                # N = 0: PR_OK, nothing looked at


# ---- the knobs ----------------------------------------------------------------------------------------------------------------------
def _make(**knobs):
    return base.Predictor(types.SimpleNamespace(gpu="0", type="REBA", debug=False, debug_joints="", debug_frame=-1, **knobs),
                          spin_model=torch.nn.Identity(), smpl_model=object())


def test_knob_defaults_and_overrides(monkeypatch):
    assert cfg.DATASET.smooth_median_radius == 0 and cfg.DATASET.smooth_sigma == 0.0
    p = _make()
    assert (p.smooth_median_radius, p.smooth_sigma) == (0, 0.0)
    p = _make(smooth_median_radius=2, smooth_sigma=1.5)
    assert (p.smooth_median_radius, p.smooth_sigma) == (2, 1.5)
    monkeypatch.setitem(cfg.DATASET, "smooth_median_radius", 3)
    monkeypatch.setitem(cfg.DATASET, "smooth_sigma", 2.5)
    p = _make()
    assert (p.smooth_median_radius, p.smooth_sigma) == (3, 2.5)
    p = _make(smooth_median_radius=0, smooth_sigma=0.0)                    # args win, also with 0
    assert (p.smooth_median_radius, p.smooth_sigma) == (0, 0.0)
    p = _make(smooth_median_radius=None, smooth_sigma=None)                # None: not given
    assert (p.smooth_median_radius, p.smooth_sigma) == (3, 2.5)
    for knobs in (dict(smooth_median_radius=16), dict(smooth_median_radius=-1), dict(smooth_sigma=-1.0), dict(smooth_sigma=float("nan")),
                  dict(smooth_median_radius=1.5)):
        with pytest.raises(ValueError, match="frames"):
            _make(**knobs)


def _canned_pass(pred, monkeypatch, seen):
    n = 9
    rng = np.random.default_rng(3)
    canned = (rng.uniform(-90, 90, (n, 24, 3)), rng.standard_normal((n, 24, 3)).astype(np.float32), None,
              rng.standard_normal((n, 24, 3)).astype(np.float32))

    def pose(self, batches, keep_images=True, n_total=None, smpl_params=None):
        seen["smpl_params"] = smpl_params is not None
        if smpl_params is not None:
            smpl_params.update(rotmat=np.tile(np.eye(3, dtype=np.float32), (n, 24, 1, 1)), betas=np.zeros((n, 10), np.float32),
                               cam=np.ones((n, 3), np.float32))
        return canned
    monkeypatch.setattr(base.Predictor, "get_pose_estimation_results", pose)
    monkeypatch.setattr(base.Predictor, "_on_device", lambda self, frames: torch.as_tensor(frames))
    monkeypatch.setattr(base.Predictor, "_run_scorers", lambda self, out, info: {})
    people = [(7, np.ones((5, 4), np.float32), np.arange(5)), (8, np.ones((4, 4), np.float32), np.array([2, 3, 5, 6]))]
    return canned, people


def test_with_both_knobs_at_zero_the_scoring_pass_never_reaches_the_smoothing_code(monkeypatch):
    seen = {}
    pred = _make()
    canned, people = _canned_pass(pred, monkeypatch, seen)

    def spy(*a, **k):
        raise AssertionError("knobs 0: the smoothing code must not be reached")
    monkeypatch.setattr(smooth, "smooth_tracks", spy)
    monkeypatch.setattr(base.Predictor, "_smooth_rows", spy)
    outs, _ = pred._score_tracks(np.zeros((8, 4, 4, 3), np.uint8), people, {}, False, 1.2)
    assert seen["smpl_params"] is False and [list(o) for o in outs] == [["result", "joint_cam", "debug_result", "frames", "bboxes"]] * 2
    assert np.array_equal(np.concatenate([o["result"] for o in outs]), canned[0])
    # a predictor built without __init__ (no knob attributes at all) is off too
    bare = object.__new__(base.Predictor)
    bare.batch_size = 4
    outs, _ = bare._score_tracks(np.zeros((8, 4, 4, 3), np.uint8), people, {}, False, 1.2)
    assert "smooth" not in outs[0]


@pytest.mark.parametrize("knobs", [dict(smooth_median_radius=1), dict(smooth_sigma=0.5), dict(smooth_median_radius=2, smooth_sigma=1.5)])
def test_either_knob_sends_every_row_through_one_smoothing_call(monkeypatch, tmp_path, knobs):
    seen = {}
    pred = _make(**knobs)
    canned, people = _canned_pass(pred, monkeypatch, seen)
    calls = []

    def rows(self, smpl, people_, fidx, m, sigma):
        calls.append((sorted(smpl), np.asarray(fidx).tolist(), m, sigma))
        n = len(fidx)
        flags = dict(status=np.arange(n, dtype=np.int32) % 2, replaced=np.full(n, 0b101, np.int32))
        return canned[0] + 1.0, canned[1] + 1.0, canned[3] + 1.0, flags
    monkeypatch.setattr(base.Predictor, "_smooth_rows", rows)
    outs, _ = pred._score_tracks(np.zeros((8, 4, 4, 3), np.uint8), people, {}, False, 1.2)
    assert seen["smpl_params"] is True                                   # asked for internally
    assert calls == [(["betas", "cam", "rotmat"], [0, 1, 2, 3, 4, 2, 3, 5, 6], pred.smooth_median_radius, pred.smooth_sigma)]
    assert "rotmat" not in outs[0] and np.array_equal(outs[1]["result"], canned[0][5:] + 1.0)
    assert outs[1]["smooth"]["status"].tolist() == [1, 0, 1, 0] and outs[0]["smooth"]["median_radius"] == pred.smooth_median_radius
    # smooth.json: the parameters and per person the replaced items and the fallbacks
    report = pred.write_smooth_report(outs[0], {"ids": [7, 8], "people": outs}, str(tmp_path))
    assert json.loads((tmp_path / "smooth.json").read_text()) == report
    assert report["unit"] == "frames" and report["sigma"] == pred.smooth_sigma and report["gaussian_radius"] == smooth.gaussian_radius(pred.smooth_sigma)
    assert report["people"] == [dict(id=7, n_frames=5, replaced=10, fallbacks=2), dict(id=8, n_frames=4, replaced=8, fallbacks=2)]
    assert pred.write_smooth_report(outs[0], None, str(tmp_path))["people"] == [dict(id=None, n_frames=5, replaced=10, fallbacks=2)]
