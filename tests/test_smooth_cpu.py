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


@pytest.mark.parametrize("name", ["short_m2_s1.5", "gaps_m2_s1.5", "gaps_m3_s0", "tile+1", "fallback_m0_s50", "outlier_m2_s1.5"])
def test_the_vectorised_reference_is_the_contract_item_by_item(name):
    c, ref = sc.case(name), sc.reference(name)
    want, status = _brute_force(c)
    assert np.array_equal(ref["status"], status)
    for key, v in want.items():
        if c["sigma"] == 0:
            assert np.array_equal(sc.bits(ref[key]), sc.bits(v)), key
        else:
            # two float64 evaluations of the same sums (the batched SVD against one matrix at a time)
            assert np.abs(ref[key] - v).max() <= 1e-13 * max(1.0, float(np.abs(v).max())), key
    # what comes out of stage 2 is a rotation
    if c["sigma"] > 0:
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
        assert len(c["frame_no"]) <= 600
        sc.check(name, {k: (None if ref[k] is None else ref[k].astype(np.float32) if k in ("rotmat", "betas", "cam") else ref[k])
                        for k in ("rotmat", "betas", "cam", "status", "replaced")})       # the reference passes its own check
    assert smallest > 1e-7, smallest                                      # far from the 1e-9 under which an item may be left out
    fb = sc.reference("fallback_m0_s50")
    # 2e-8, and for +-60 degrees 12 / (17 / 3)^1.5 = 0.89: neither near 0.05
    assert 1e-8 < fb["c"][1, 5] < 4e-8 and 0.88 < fb["c"][1, 7] < 0.90
    assert fb["status"][:3].tolist() == [1 << 5] * 3 and not fb["status"][3:].any()
    for name in sc.NAMES:                                                  # no other case sits near the threshold
        cc = sc.reference(name)["c"]
        if cc is not None:
            assert not ((cc > 0.005) & (cc < 0.5)).any(), name
    out = sc.case("outlier_m1_s0")
    row, j = out["outlier"]
    assert sc.reference("outlier_m1_s0")["replaced"][row] >> j & 1
    sizes = {len(sc.case(n)["frame_no"]) for n in sc.NAMES}
    assert {sc.TILE - 1, sc.TILE, sc.TILE + 1, 2 * sc.TILE + 1} <= sizes
    assert {(sc.CASES[n][1] > 0, sc.CASES[n][2] > 0) for n in sc.NAMES} == {(False, False), (True, False), (False, True), (True, True)}
    assert smooth_ref.gaussian_radius(5.0) == 15 == smooth.gaussian_radius(5.0) and smooth.gaussian_radius(1.5) == 5
    assert smooth.gaussian_radius(0.0) == 0 and smooth.gaussian_radius(1e9) == 15


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
