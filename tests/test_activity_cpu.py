"""No GPU: what tests/activity_ref.py (the float64 restatement of pr_activity_tracks' contract, include/poserisk_hip.h section
t1) says on planted scenes -- held, repeated and rapid each fire where planted and nowhere else, the knife edges decide a bit --,
activity.frames / thresholds / counts, the argument refusals of the Python entry and of the C entry, the declared symbols, and the
Predictor's knob: its parsing, its refusals, that off never reaches the new code and that on sends every row through one call."""
import ctypes as C
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import activity_cases as ac
import activity_ref
from conftest import REPO
from poserisk_release_amd import _lib, activity, dropin

dropin.install()
from core import base  # noqa: E402
from core.config import cfg  # noqa: E402

ALL = 0xfff
H, R, G, E = ac.H0, ac.R0, ac.G0, ac.E0


# ---- the reference on planted scenes -------------------------------------------------------------------------------------------
def test_the_case_list_covers_what_the_kernel_can_get_wrong():
    sizes = {n: len(ac.case(n)["frame_no"]) for n in ac.NAMES}
    assert max(sizes.values()) <= 3000 and sizes["empty"] == 0 and len(ac.case("empty")["track_start"]) == 1
    assert all(ac.case(n)["H"] <= (110 if n in ac.LATTICE_NAMES else 40) for n in ac.NAMES if n != "big")
    assert ac.case("big")["H"] == 700 and sizes["big"] == 1500
    assert ac.case("big")["H"] > 10 * ac.CHUNK and sizes["big"] > 10 * ac.TILE                  # many chunks, many tiles
    lengths = np.diff(ac.case("lengths")["track_start"]).tolist()
    assert {0, 1, H, H + 1, H + G} <= set(lengths)
    starts = set(ac.case("edges")["track_start"].tolist())
    assert {ac.TILE, ac.TILE + ac.CHUNK, 2 * ac.TILE - 1} <= starts and any(s % ac.TILE == 0 and s for s in starts)
    assert len(ac.case("many_tracks")["track_start"]) - 1 > 256                                  # more tracks than one launch carries
    f = ac.case("wild_frames")["frame_no"]
    assert f.min() == -2 ** 31 and f.max() == 2 ** 31 - 1 and (np.diff(f) < 0).any() and (np.diff(f) == 0).any()
    assert np.isnan(ac.case("nan")["rotmat"]).any()
    for n in ac.NAMES:                                   # every case has a reference, over every row, and something to find
        ref = ac.reference(n)
        assert ref["flags"].shape == (sizes[n], 4) and ref["adds"].shape == (sizes[n], 4)
        assert np.array_equal(ref["adds"], activity_ref.adds_of(ref["flags"]))
    fired = np.sum([np.count_nonzero(ac.reference(n)["flags"], axis=0) for n in ac.NAMES if sizes[n]], axis=0)
    assert (fired > 0).all()


def test_a_still_stretch_of_exactly_h_plus_1_rows_is_held_and_nothing_else_is():
    c, ref = ac.case("still_segment"), ac.reference("still_segment")
    q, last = c["planted"]["first_still"], c["planted"]["last_still"]
    assert last - q == H
    want = np.zeros(len(c["frame_no"]), np.int32)
    want[last] = ALL
    assert np.array_equal(ref["stage_b"][:, 0], want)                       # only the window that ends the stretch is all still
    want[q:last + 1] = ALL
    assert np.array_equal(ref["flags"][:, 0], want)                         # ... and stage C marks the whole stretch
    assert not ref["flags"][:, 1].any() and not ref["flags"][:, 2].any()    # E = 1000; 12 degrees a row is not rapid over R rows
    assert np.array_equal(ref["adds"][:, 0], (want != 0).astype(np.int32)) and np.array_equal(ref["adds"][:, 3], ref["adds"][:, 0])


def test_more_than_e_events_inside_h_are_repeated_and_e_are_not():
    c, ref = ac.case("oscillation"), ac.reference("oscillation")
    n = 3 * H
    first = c["planted"]["first_event"]
    assert first == H
    for t, n_events in enumerate((E, E + 1)):
        moved = ref["flags"][t * n:(t + 1) * n, 3]
        assert np.array_equal(np.nonzero(moved)[0], first + 2 * np.arange(n_events)) and set(moved[moved != 0]) == {activity_ref.MASK_L}
    rep = ref["flags"][:, 1]
    want = np.zeros(2 * n, np.int32)
    want[n + 2 * E:n + 2 * H + 1] = activity_ref.MASK_L     # windows ending at rows H + 2 E .. 2 H hold all E + 1 events; spread back by H
    assert np.array_equal(rep, want)
    assert not ref["flags"][:, 2].any()                      # 20 degrees is not rapid
    assert np.array_equal(ref["adds"][:, 1], (want != 0).astype(np.int32) | (ref["flags"][:, 0] & activity_ref.MASK_L != 0))


def test_a_jump_is_rapid_for_r_rows_and_no_longer():
    c, ref = ac.case("jump"), ac.reference("jump")
    r = c["planted"]["jump_row"]
    want = np.zeros(len(c["frame_no"]), np.int32)
    want[r:r + R] = 1 << 1                                   # the neck; row r + R - 1 still sees row r - 1, row r + R does not
    assert np.array_equal(ref["flags"][:, 2], want)
    assert np.array_equal(np.nonzero(ref["flags"][:, 3])[0], [r]) and ref["flags"][r, 3] == 1 << 1
    assert not ref["flags"][:, 1].any()


def test_a_gap_of_g_keeps_a_window_whole_and_g_plus_1_breaks_it():
    c, ref = ac.case("gaps"), ac.reference("gaps")
    n, row = 3 * H, c["planted"]["gap_row"]
    f = c["frame_no"].astype(np.int64)
    assert f[row] - f[row - 1] == G and f[n + row] - f[n + row - 1] == G + 1
    one, two = ref["stage_b"][:n, 0], ref["stage_b"][n:, 0]
    covered = f[:n] - f[0] > H - G
    assert np.array_equal(one, np.where(covered, ALL, 0))                  # steps of G: every window long enough is whole
    broken = (np.arange(n) >= row) & (f[n:] - f[n + row] <= H - G)         # windows that hold the step, or start too close behind it
    assert broken.sum() >= H - G and not two[broken].any() and (two[~broken & (f[n:] - f[n] > H - G)] == ALL).all()


def test_a_second_track_does_not_see_the_first():
    c, ref = ac.case("adjacent"), ac.reference("adjacent")
    for a, b in c["planted"]["planted_tracks"]:
        alone = activity_ref.activity(c["rotmat"][a:b], c["frame_no"][a:b], [0, b - a], *(c[k] for k in ac.PARAMS))
        assert np.array_equal(alone["flags"], ref["flags"][a:b])
    assert not ref["stage_b"][140:140 + H - G, 0].any()                    # the third track's first windows are too short


def test_each_knife_edge_decides_an_output_bit():
    c, ref = ac.case("knife"), ac.reference("knife")
    k, i, b = ac.KNIFE["k"], ac.KNIFE["i"], ac.KNIFE["b"]
    d = c["dot_static"]
    assert d == activity_ref.dot_pair(c["rotmat"], k, i, b) and 2.9 < d < 3.0
    assert (ref["flags"][:, 0] >> b & 1).all() and not (ref["flags"][:, 2] >> b & 1).any() and not (ref["flags"][:, 3] >> b & 1).any()
    run = lambda **over: activity_ref.activity(c["rotmat"], c["frame_no"], c["track_start"], *({**{p: c[p] for p in ac.PARAMS}, **over}[p]
                                                                                          for p in ac.PARAMS))
    up = np.nextafter(d, 4.0)
    assert not (run(dot_static=up)["stage_b"][i, 0] >> b & 1)              # >= at equality, not >
    assert run(dot_move=up)["flags"][k, 3] >> b & 1                        # < at equality records nothing, one ulp up it does
    assert run(dot_rapid=up)["flags"][i, 2] >> b & 1


def test_rows_holding_nan_fail_every_comparison():
    ref = ac.reference("nan")
    torso = 1 << 0
    # the row whose torso is NaN is not held itself, records no event, is not rapid -- and breaks every window that holds it
    assert not (ref["stage_b"][30:30 + H + 1, 0] & torso).any() and ref["stage_b"][29, 0] & torso
    assert not ref["stage_b"][50:50 + H + 1, 0].any() and (ref["stage_b"][50 + H + 1:80, 0] == ALL).all()      # the all-NaN row 50
    assert not ref["flags"][30, 3] & torso and not ref["flags"][30, 2] & torso
    assert ref["stage_b"][50, 0] == 0 and ref["flags"][50, 2] == 0 and ref["flags"][50, 3] == 0


# ---- the cases that pin the chunk loop, the span, the spread and the bounds ---------------------------------------------------
def _first_row(c, i):
    ts = c["track_start"]
    return int(ts[np.searchsorted(ts, i, side="right") - 1])


def _has_hole(c, i):
    """Two rows that follow each other in W_i(H) are not 1..G frames apart."""
    f = c["frame_no"].astype(np.int64)
    steps = np.diff(f[activity_ref.window(f, i, _first_row(c, i), c["H"])])
    return bool(((steps < 1) | (steps > c["G"])).any())


def _nearest_witness(c, x, i, b):
    """The largest k in W_i(R) with dot_b(k, i) < dot_rapid, or None."""
    f = c["frame_no"].astype(np.int64)
    mem = activity_ref.window(f, i, _first_row(c, i), c["R"])
    with np.errstate(invalid="ignore"):
        hit = mem[activity_ref.dots(x[mem, b], x[i, b][None]) < c["dot_rapid"]]
    return int(hit.max()) if hit.size else None


def test_the_lattice_reaches_an_older_chunk_for_rapid_alone():
    assert [(ac.case(n)["H"], ac.case(n)["R"]) for n in ac.LATTICE_NAMES] == [(31, 31), (32, 1), (33, 33), (63, 40), (64, 64), (65, 33), (96, 96), (100, 50)]
    fired = np.zeros(4, np.int64)
    far = {}
    for name in ac.LATTICE_NAMES:
        c, ref = ac.case(name), ac.reference(name)
        ts, f = c["track_start"], c["frame_no"].astype(np.int64)
        assert np.diff(ts).tolist() == [200, 130, 70] and f.min() == -2 ** 31 and f.max() == 2 ** 31 - 1
        steps = np.diff(f[:330])
        assert (steps == c["G"]).any() and (steps == c["G"] + 1).any() and (steps == 0).any()      # gaps <= G, > G, a repeated frame
        assert f[128] == f[127] and f[256] == f[255] and 128 % ac.TILE == 0 == 256 % ac.TILE       # the holes, on tile edges
        fired += np.count_nonzero(ref["flags"], axis=0)
        x = activity_ref.scored(c["rotmat"])
        far[name] = 0
        for i in np.nonzero(ref["flags"][:, 2])[0]:
            if not _has_hole(c, i):
                continue
            for b in range(12):
                if ref["flags"][i, 2] >> b & 1:
                    far[name] += int(i - _nearest_witness(c, x, i, b) >= ac.CHUNK)
    assert (fired > 0).all(), fired                              # held, repeated, rapid and moved each fire somewhere
    # rows that are rapid only through a row CHUNK or more back, in a window with a hole: wherever R allows it
    assert all((far[n] > 0) == (ac.case(n)["R"] > ac.CHUNK) for n in ac.LATTICE_NAMES), far


def test_a_span_of_exactly_h_minus_g_is_not_whole_and_one_more_is():
    c, ref = ac.case("span_edge"), ac.reference("span_edge")
    f, ts, p = c["frame_no"].astype(np.int64), c["track_start"], c["planted"]
    assert len(p["not_whole"]) == len(p["whole"]) == 4
    for rows, whole in ((p["not_whole"], False), (p["whole"], True)):
        for i in rows:
            first = _first_row(c, i)
            mem = activity_ref.window(f, i, first, H)
            assert i + 1 in ts and not _has_hole(c, i)                          # the track's last row, its window without a hole
            assert (f[i] - f[mem[0]] == H - G) if not whole else (f[i] - f[mem[0]] in (H - G + 1, H - G + 2))
            assert ref["stage_b"][i, 0] == (ALL if whole else 0)                 # the reference's stage-B mask ...
            assert (ref["flags"][mem, 0] == (ALL if whole else 0)).all()         # ... and what the spread makes of it
            assert not ref["stage_b"][first:i, 0].any()                          # no earlier window of the track is whole
    assert [int(f[i] - f[activity_ref.window(f, i, _first_row(c, i), H)[0]]) for i in p["whole"]] == [H - G + 1] * 3 + [H - G + 2]
    assert not ref["flags"][p["untouched"], 0].any()                             # the rows before the long step are out of reach
    assert np.count_nonzero(ref["stage_b"][:, 0]) == 4


def test_a_gap_bound_above_the_hold_makes_every_covered_window_whole():
    for name in ("G_huge", "G_gt_H"):
        c, ref = ac.case(name), ac.reference(name)
        assert c["G"] > c["H"] and (c["G"] == 2 ** 31 - 1) == (name == "G_huge")
        lengths = np.diff(c["track_start"])
        one = int(c["track_start"][np.nonzero(lengths == 1)[0][0]])
        assert ref["stage_b"][one, 0] == ALL == ref["flags"][one, 0]           # a one-row window is whole, and still
        for i in range(len(c["frame_no"])):
            if not _has_hole(c, i):
                assert ref["stage_b"][i, 0] != 0 or np.count_nonzero(ref["flags"][i, 2:]) or c["rotmat"][i].std() > 0, i
        still_rows = np.arange(c["track_start"][0], c["track_start"][1]) if name == "G_huge" else np.arange(3, 43)
        holes = np.array([_has_hole(c, int(i)) for i in still_rows])
        assert np.array_equal(ref["stage_b"][still_rows, 0] == ALL, ~holes)       # in a still track: held exactly where there is no hole
    f = ac.case("G_huge")["frame_no"].astype(np.int64)
    assert (np.diff(f[:72]) > 2 ** 29).any() and not np.array([_has_hole(ac.case("G_huge"), i) for i in range(72)]).any()
    assert np.array([_has_hole(ac.case("G_huge"), i) for i in range(123, 130)]).any()      # a repeated and a backward frame still are holes
    # (with G > H a step above G never lies inside a window: the row behind it is more than H frames away)
    assert not np.array([_has_hole(ac.case("G_gt_H"), i) for i in range(3, 43)]).any()


def test_more_tracks_than_a_launch_with_the_second_launch_inside_a_tile():
    c = ac.case("many_unaligned")
    ts = c["track_start"]
    lengths = np.diff(ts)
    assert len(lengths) >= 300 and lengths.min() == 0 and lengths.max() == 10 and (c["H"], c["R"]) == (5, 2)
    assert len(ts) - 1 > 256 and ts[256] % ac.TILE != 0 and ts[256] < ts[-1]
    assert (np.count_nonzero(ac.reference("many_unaligned")["flags"][:, [0, 1, 3]], axis=0) > 0).all()


def test_a_held_bit_does_not_spread_to_a_row_that_lies_later_in_frames():
    c, ref = ac.case("spread_back"), ac.reference("spread_back")
    f = c["frame_no"].astype(np.int64)
    i, e = c["planted"]["i"], c["planted"]["e"]
    assert 0 < e - i <= H and f[e] < f[i] and ref["stage_b"][e, 0] == ALL and not ref["stage_b"][:e, 0].any()
    assert ref["flags"][i, 0] == 0 and not ref["flags"][:i + 1, 0].any() and (ref["flags"][i + 1:, 0] == ALL).all()
    # stage C without its `0 <=` on the frame difference would change this case's flags
    n = len(f)
    dropped = np.zeros(n, np.int32)
    for r in range(n):
        es = np.arange(r, min(r + H, n - 1) + 1)
        dropped[r] = np.bitwise_or.reduce(ref["stage_b"][es[f[es] - f[r] <= H], 0])
    assert dropped[i] == ALL and not np.array_equal(dropped, ref["flags"][:, 0])


def test_thresholds_at_the_ends_of_their_range():
    c, ref = ac.case("thresholds_at_bounds"), ac.reference("thresholds_at_bounds")
    assert (c["dot_static"], c["dot_move"], c["dot_rapid"]) == (3.0, 3.0, -1.0)
    b, u, fb, fl = ac.BOUNDS["ulp_bit"], ac.BOUNDS["ulp_row"], ac.BOUNDS["flip_bit"], ac.BOUNDS["flip_row"]
    assert activity_ref.dot_pair(c["rotmat"], 0, 1, b) == 3.0                           # bit-equal rows: exactly 3
    assert 3.0 - 2.0 ** -23 < activity_ref.dot_pair(c["rotmat"], u, u + 1, b) < 3.0      # one ulp of one element
    assert activity_ref.dot_pair(c["rotmat"], u, u, b) < 3.0                             # ... and the row against itself
    assert activity_ref.dot_pair(c["rotmat"], fl, fl + 1, fb) == -1.0                    # a half turn: exactly -1, not below
    assert not ref["flags"][:, 2].any()                                                  # rapid never
    want = np.zeros(80, np.int32)
    want[[u, u + 1]] = 1 << b
    want[[fl, fl + 1]] |= 1 << fb
    assert np.array_equal(ref["flags"][:, 3], want)                                      # an event there and on the way back
    held = np.full(80, ALL, np.int32)
    held[u:u + H + 1] &= ~(1 << b)
    held[fl:fl + H + 1] &= ~(1 << fb)
    held[:H - G + 1] = 0                                                                 # (the first windows span H - G frames or fewer)
    assert np.array_equal(ref["stage_b"][:, 0], held)                                    # held only where every member is bit-equal


def test_the_sweep_draws_every_kind_of_problem():
    fired, wild, holds = np.zeros(4, np.int64), 0, set()
    for name in ac.SWEEP_NAMES:
        c, ref = ac.case(name), ac.reference(name)
        assert 1 <= c["R"] <= c["H"] <= 110 and 1 <= c["G"] <= 5 and 0 <= c["E"] <= 4 and 1 <= len(c["track_start"]) - 1 <= 3
        assert np.diff(c["track_start"]).max() <= 160 and len(c["frame_no"]) >= 1
        fired += np.count_nonzero(ref["flags"], axis=0)
        wild += int((c["frame_no"] == -2 ** 31).any())
        holds.add(c["H"] // ac.CHUNK)
    assert (fired > 0).all() and wild >= 5 and holds == {0, 1, 2, 3} and len(ac.SWEEP_NAMES) == 60


# ---- the Python helpers ------------------------------------------------------------------------------------------------------
def test_frames_thresholds_and_counts():
    assert activity.frames(60, 30) == 1800 and activity.frames(0.2, 30) == 6 and activity.frames(1, 29.97) == 30
    assert activity.frames(0.001, 30) == 1 and activity.frames(1.0, 25.0) == 25 and activity.frames(0.2, 24) == 5
    ds, dm, dr = activity.thresholds(10, 15, 45)
    assert abs(ds - (1 + 2 * np.cos(np.deg2rad(10.0)))) < 1e-15 and ds > dm > dr and abs(dr - (1 + np.sqrt(2.0))) < 1e-15
    assert activity.thresholds(0, 90, 180) == (3.0, pytest.approx(1.0, abs=1e-15), -1.0)
    assert ac.thresholds(10, 15, 45) == (ds, dm, dr)
    assert activity.JOINT_NAMES == activity_ref.JOINT_NAMES and len(activity.JOINT_NAMES) == 12
    par = activity.check_parameters(30.0)
    assert (par["hold_frames"], par["rapid_frames"], par["gap_frames"], par["rep_events"]) == (1800, 30, 6, 8)
    assert (par["dot_static"], par["dot_move"], par["dot_rapid"]) == (ds, dm, dr) and par["hold_seconds"] == 60.0
    flags = np.array([[0b11, 0, 0, 0], [0b01, 1 << 11, 0, 0], [0, 0, 1 << 4, 1 << 4]], np.int32)
    got = activity.counts(flags)
    assert list(got) == ["held", "repeated", "rapid", "moved"] and got["held"]["rows"] == 2 and got["held"]["joints"]["Torso"] == 2
    assert got["held"]["joints"]["Neck"] == 1 and got["repeated"]["joints"]["R_Wrist"] == 1 and got["rapid"]["joints"]["L_Thorax"] == 1
    assert sum(got["moved"]["joints"].values()) == 1 and activity.counts(np.zeros((0, 4), np.int32))["held"]["rows"] == 0
    ref = ac.reference("jump")
    assert activity.counts(ref["flags"])["rapid"] == dict(rows=R, joints={n: (R if n == "Neck" else 0) for n in activity.JOINT_NAMES})


def test_activity_tracks_refuses_bad_arguments_before_any_device_call(monkeypatch):
    monkeypatch.setattr(_lib, "load", lambda: pytest.fail("an argument error must not reach the library"))
    rot, fno, ts = torch.zeros((5, 24, 3, 3)), np.arange(5), [0, 3, 5]
    ok = dict(rotmat=rot, frame_no=fno, track_start=ts, fps=30.0)
    for over, word in ((dict(fps=None), "fps"), (dict(fps=0), "fps"), (dict(fps=float("nan")), "fps"), (dict(hold_seconds=0), "hold_seconds"),
                       (dict(hold_seconds=600), "16384"), (dict(rapid_seconds=61), "longer than hold_seconds"), (dict(gap_seconds=-1), "gap_seconds"),
                       (dict(rep_events=-1), "rep_events"), (dict(rep_events=1.5), "rep_events"), (dict(rep_events=True), "rep_events"),
                       (dict(static_deg=181), "static_deg"), (dict(move_deg=-1), "move_deg"), (dict(rapid_deg=float("inf")), "rapid_deg"),
                       (dict(rapid_deg="45"), "rapid_deg"), (dict(hold_frames=3), "unknown"),
                       (dict(rotmat=torch.zeros((5, 24, 3))), r"float32\[N,24,3,3\]"), (dict(rotmat=rot.double()), "float32"),
                       (dict(track_start=[0, 3]), "s_T = N"), (dict(track_start=[1, 5]), "0 = s_0"), (dict(track_start=[0, 4, 3, 5]), "<="),
                       (dict(track_start=[[0, 5]]), "1-D"), (dict(track_start=[0.0, 5.0]), "integer"), (dict(frame_no=np.arange(4)), "frame_no"),
                       (dict(frame_no=np.arange(5.0)), "integer"), (dict(frame_no=np.arange(5) + 2 ** 31), "int32")):
        with pytest.raises(ValueError, match=word):
            activity.activity_tracks(**{**ok, **over})
    with pytest.raises(TypeError, match="torch tensor"):
        activity.activity_tracks(**{**ok, "rotmat": rot.numpy()})
    with pytest.raises(_lib.PoseRiskHipError, match="on the GPU"):        # all else being right, a CPU tensor: there is no CPU path
        activity.activity_tracks(**ok)


def test_the_symbols_are_declared_and_bound_and_the_abi_is_16():
    header = open(os.path.join(REPO, "include", "poserisk_hip.h")).read()
    declared = set(re.findall(r"\b(pr_activity_\w+|pr_reba_rows|pr_rula_rows)\s*\(", header))
    assert declared == {"pr_activity_tile_rows", "pr_activity_chunk_rows", "pr_activity_workspace_bytes", "pr_activity_tracks", "pr_reba_rows",
                        "pr_rula_rows"}
    assert declared <= set(_lib.SIGNATURES) and _lib.ABI_VERSION == 16
    assert "/* t1 " in header and "PR_ACTIVITY_MAX_HOLD 16384" in header and activity.MAX_HOLD_FRAMES == 16384
    fields = re.search(r"typedef struct pr_activity_params \{(.*?)\}", header, re.S).group(1)
    assert re.findall(r"(\w+)\s*;", re.sub(r"/\*.*?\*/", "", fields)) == [n for n, _ in _lib.ActivityParams._fields_]
    assert C.sizeof(_lib.ActivityParams) == 40
    lib = _lib.load()
    assert lib.pr_abi_version() == 16 and lib.pr_activity_tile_rows() == ac.TILE and lib.pr_activity_chunk_rows() == ac.CHUNK
    assert lib.pr_activity_workspace_bytes(-1) == 0 and lib.pr_activity_workspace_bytes(100) >= 1200 and lib.pr_activity_workspace_bytes(100) % 256 == 0
    # the argument checks return before any device work (no GPU here)
    fake, starts = 256, (C.c_int * 3)(0, 3, 5)

    def call(par=(24, 3, 2, 3, 2.9, 2.8, 2.4), rot=fake, fno=fake + 4096, starts=starts, T=2, N=5, flags=fake + 8192, adds=fake + 12288, ws=fake + 65536):
        rc = lib.pr_activity_tracks(C.byref(_lib.ActivityParams(*par)), rot, fno, starts, T, N, flags, adds, ws, None)
        return rc, lib.pr_last_error().decode()
    nan = float("nan")
    for over, word in ((dict(par=(0, 3, 2, 3, 2.9, 2.8, 2.4)), "hold_frames"), (dict(par=(16385, 3, 2, 3, 2.9, 2.8, 2.4)), "hold_frames"),
                       (dict(par=(24, 25, 2, 3, 2.9, 2.8, 2.4)), "rapid_frames"), (dict(par=(24, 0, 2, 3, 2.9, 2.8, 2.4)), "rapid_frames"),
                       (dict(par=(24, 3, 0, 3, 2.9, 2.8, 2.4)), "gap_frames"), (dict(par=(24, 3, 2, -1, 2.9, 2.8, 2.4)), "rep_events"),
                       (dict(par=(24, 3, 2, 3, nan, 2.8, 2.4)), "dot_static"), (dict(par=(24, 3, 2, 3, 2.9, 3.1, 2.4)), "dot_move"),
                       (dict(par=(24, 3, 2, 3, 2.9, 2.8, -1.1)), "dot_rapid"), (dict(N=-1), "N = -1"), (dict(T=-1), "T = -1"),
                       (dict(starts=(C.c_int * 3)(0, 4, 3)), "track_start"), (dict(starts=(C.c_int * 3)(0, 3, 6)), "not N"),
                       (dict(starts=None), "null track_start"), (dict(fno=None), "null"), (dict(rot=None), "null"), (dict(flags=None), "null flags"),
                       (dict(ws=None), "workspace"), (dict(ws=fake + 2), "aligned"), (dict(adds=fake + 8192), "share"), (dict(ws=fake), "share")):
        rc, msg = call(**over)
        assert rc == -1 and word in msg and "pr_activity_tracks" in msg, (over, rc, msg)
    assert lib.pr_activity_tracks(None, None, None, None, 0, 0, None, None, None, None) == -1
    assert call(N=0, T=0, starts=(C.c_int * 1)(0))[0] == 0                # N = 0: PR_OK, nothing looked at
    info = _lib.RebaInfo(1, 0, 0, 0, 0, 0, 0)
    assert lib.pr_reba_rows(None, 4, C.byref(info), None, None, None) == -1 and "pr_reba_rows" in lib.pr_last_error().decode()
    assert lib.pr_rula_rows(fake, 4, None, None, fake + 64, None) == -1 and "pr_rula_rows" in lib.pr_last_error().decode()
    assert lib.pr_reba_rows(fake, 4, C.byref(info), fake + 64, fake + 64, None) == -1 and "output" in lib.pr_last_error().decode()


# ---- the knob ----------------------------------------------------------------------------------------------------------------------
def _make(**knobs):
    return base.Predictor(types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1, **knobs),
                          spin_model=torch.nn.Identity(), smpl_model=object())


def test_knob_defaults_overrides_and_refusals(monkeypatch):
    assert dict(cfg.ACTIVITY) == dict(derive=False, hold_seconds=60.0, static_deg=10.0, move_deg=15.0, rep_events=8, rapid_seconds=1.0,
                                      rapid_deg=45.0, gap_seconds=0.2) == activity.DEFAULTS
    assert _make().activity is None and _make(derive_activity=False).activity is None and _make(derive_activity=None).activity is None
    on = _make(derive_activity=True).activity
    assert on == {k: v for k, v in activity.DEFAULTS.items() if k != "derive"}
    monkeypatch.setitem(cfg.ACTIVITY, "derive", True)
    monkeypatch.setitem(cfg.ACTIVITY, "hold_seconds", 2.0)
    assert _make().activity["hold_seconds"] == 2.0 and _make(derive_activity=None).activity is not None
    assert _make(derive_activity=False).activity is None                  # args win, also with False
    for key, value, word in (("hold_seconds", -1, "hold_seconds"), ("rep_events", 1.5, "rep_events"), ("static_deg", 200, "static_deg"),
                             ("rapid_seconds", 5.0, "longer than hold_seconds"), ("gap_seconds", "x", "gap_seconds"), ("hold_seconds", 1e6, "16384")):
        with monkeypatch.context() as m:
            m.setitem(cfg.ACTIVITY, key, value)
            with pytest.raises(ValueError, match=word):
                _make()
    with monkeypatch.context() as m:
        m.setitem(cfg.ACTIVITY, "hold_frames", 5)
        with pytest.raises(ValueError, match="unknown"):
            _make()
        m.setitem(cfg.ACTIVITY, "derive", False)
        assert _make().activity is None                                     # off: nothing of the section is looked at


def _canned_pass(monkeypatch, seen):
    n = 9
    rng = np.random.default_rng(3)
    canned = (rng.uniform(-90, 90, (n, 24, 3)), rng.standard_normal((n, 24, 3)).astype(np.float32), None,
              rng.standard_normal((n, 24, 3)).astype(np.float32))
    rotmat = rng.standard_normal((n, 24, 3, 3)).astype(np.float32)

    def pose(self, batches, keep_images=True, n_total=None, smpl_params=None):
        seen["smpl_params"] = smpl_params is not None
        if smpl_params is not None:
            smpl_params.update(rotmat=rotmat, betas=np.zeros((n, 10), np.float32), cam=np.ones((n, 3), np.float32))
        return canned
    monkeypatch.setattr(base.Predictor, "get_pose_estimation_results", pose)
    monkeypatch.setattr(base.Predictor, "_on_device", lambda self, frames: torch.as_tensor(frames))
    people = [(7, np.ones((5, 4), np.float32), np.arange(5)), (8, np.ones((4, 4), np.float32), np.array([2, 3, 5, 6]))]
    return canned, rotmat, people


def test_with_the_knob_off_the_scoring_pass_never_reaches_the_activity_code(monkeypatch):
    seen = {}
    pred = _make()
    canned, _, people = _canned_pass(monkeypatch, seen)

    def spy(*a, **k):
        raise AssertionError("knob off: the activity code must not be reached")
    monkeypatch.setattr(activity, "activity_tracks", spy)
    monkeypatch.setattr(base.Predictor, "_activity_rows", spy)
    monkeypatch.setattr(base.Predictor, "_run_scorers", lambda self, out, info: {})       # the two-argument call of before
    outs, _ = pred._score_tracks(np.zeros((8, 4, 4, 3), np.uint8), people, {}, False, 1.2)
    assert seen["smpl_params"] is False and [list(o) for o in outs] == [["result", "joint_cam", "debug_result", "frames", "bboxes"]] * 2
    outs, _ = pred._score_tracks(np.zeros((8, 4, 4, 3), np.uint8), people, {}, False, 1.2, fps=30.0)      # fps alone changes nothing
    assert "activity" not in outs[0]


def test_the_knob_sends_every_row_through_one_call_and_the_addends_to_the_scorers(monkeypatch, tmp_path):
    seen = {}
    pred = _make(derive_activity=True)
    canned, rotmat, people = _canned_pass(monkeypatch, seen)
    with pytest.raises(ValueError, match="fps"):
        pred._score_tracks(np.zeros((8, 4, 4, 3), np.uint8), people, {}, False, 1.2)
    with pytest.raises(ValueError, match="fps"):
        pred.score_frames(np.zeros((8, 4, 4, 3), np.uint8), {7: dict(bbox=people[0][1], frames=people[0][2])}, {})
    calls, scored = [], []
    flags = np.arange(36, dtype=np.int32).reshape(9, 4) % 5
    adds = np.arange(36, dtype=np.int32).reshape(9, 4) % 3

    def rows(self, rot, people_, fidx, fps, parameters):
        calls.append((rot is rotmat, np.asarray(fidx).tolist(), fps, parameters))
        return flags, adds, activity.check_parameters(fps, **parameters)

    class Scorer:
        def __init__(self, kind):
            self.kind, self.log = kind, []

        def __call__(self, poses, joint_cams, add_info, *, rows=None):
            scored.append((self.kind, np.array(rows)))
            return [dict(score=np.int64(1), log_score=[0]) for _ in poses]

        def action_level(self, score):
            return 1, "x"
    monkeypatch.setattr(base.Predictor, "_activity_rows", rows)
    pred.reba, pred.rula = Scorer("reba"), Scorer("rula")
    outs, _ = pred._score_tracks(np.zeros((8, 4, 4, 3), np.uint8), people, {}, False, 1.2, fps=25.0)
    assert seen["smpl_params"] is True and calls == [(True, [0, 1, 2, 3, 4, 2, 3, 5, 6], 25.0, pred.activity)]
    assert "rotmat" not in outs[0] and list(outs[0])[:4] == ["result", "joint_cam", "debug_result", "activity"]
    assert np.array_equal(outs[1]["activity"]["flags"], flags[5:]) and np.array_equal(outs[0]["activity"]["adds"], adds[:5])
    assert outs[0]["activity"]["parameters"]["hold_frames"] == 1500
    assert [k for k, _ in scored] == ["reba", "rula", "reba", "rula"]
    assert np.array_equal(scored[0][1], adds[:5, 0]) and np.array_equal(scored[1][1], adds[:5, 1:4]) and np.array_equal(scored[3][1], adds[5:, 1:4])
    # activity.json: the parameters and per person the rows per kind and joint
    report = pred.write_activity_report(outs[0], {"ids": [7, 8], "people": outs}, str(tmp_path))
    assert json.loads((tmp_path / "activity.json").read_text()) == report
    assert report["parameters"]["hold_seconds"] == 60.0 and report["parameters"]["hold_frames"] == 1500 and report["joints"] == list(activity.JOINT_NAMES)
    assert [p["id"] for p in report["people"]] == [7, 8] and report["people"][1]["n_frames"] == 4
    assert report["people"][0]["held"] == activity.counts(flags[:5])["held"] and report["people"][1]["adds"]["b_muscle"] == int(adds[5:, 3].sum())
    assert pred.write_activity_report(outs[0], None, str(tmp_path))["people"][0]["id"] is None
