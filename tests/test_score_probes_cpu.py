"""Is the score probe set (tests/score_cases.py, results in tests/golden/score_probes.npz from the reference's own classes)
sufficient?  It must reach every class combination of every rule group, hold every special value, read every reachable
table cell, and notice every one-off error in a table entry and every dropped or exchanged info field.  No GPU and no
reference here: the oracle stands in for the kernels, and these tests pin it on all the new ground first."""
import itertools
import json

import numpy as np
import pytest

import score_cases
import score_probe_checks as ck
from conftest import golden
from oracle import reba_ref, rula_ref
from oracle.risk_tables import J, REBA_INFO_KEYS, RULA_INFO_KEYS
from poserisk_release_amd import synth

RULE_BLOCKS = ("grid", "cross", "specials")
# RULA's table B has a neck = 6 row that the neck rules (bending at most 4, twist at most 1) cannot reach
UNREACHABLE = {"RULA B": [(5, t, leg) for t in range(6) for leg in range(2)]}
# fields that enter only as a sum: exchanging them changes nothing, by construction
SUM_PAIRS = {("A_Muscle_use_L", "A_Load/Force_L"), ("A_Muscle_use_R", "A_Load/Force_R"), ("B_Muscle_use", "B_Load/Force")}


@pytest.fixture(scope="module")
def probes():
    g = golden("score_probes.npz")
    infos = json.loads(str(g["infos_json"]))
    pairs = [(int(a), int(b), int(i)) for a, b, i in g["pairs"]]
    pose, ri, ui, starts = ck.flatten(g["pose"], [(a, b) for a, b, _ in pairs], [infos[i] for _, _, i in pairs])
    for a in (pose, g["reba"], g["rula"], *ri.values(), *ui.values()):
        a.setflags(write=False)
    return dict(g=g, infos=infos, pairs=pairs, blocks=json.loads(str(g["blocks_json"])),
                pair_blocks=json.loads(str(g["pair_blocks_json"])), pose=pose, ri=ri, ui=ui, starts=starts,
                reba=g["reba"].astype(np.int32), rula=g["rula"].astype(np.int32))


def _rows_of(p, block_names, info=None):
    """Flat rows of the pairs on these blocks (under this info index)."""
    rows = [np.arange(p["starts"][n], p["starts"][n + 1]) for n, (b, (_, _, i)) in enumerate(zip(p["pair_blocks"], p["pairs"]))
            if b in block_names and (info is None or i == info)]
    return np.concatenate(rows) if rows else np.zeros(0, np.int64)


def test_fixture_is_what_score_cases_builds(probes):
    pose, blocks, infos, pairs = score_cases.build()
    g = probes["g"]
    assert g["pose"].dtype == np.float64 and g["pose"].shape == pose.shape
    np.testing.assert_array_equal(g["pose"].view(np.int64), pose.view(np.int64))      # bits: NaN, -0.0, denormals
    assert probes["infos"] == infos
    assert probes["blocks"] == {k: list(v) for k, v in blocks.items()}
    assert probes["pair_blocks"] == [b for b, _ in pairs]
    assert probes["pairs"] == [(*blocks[b], i) for b, i in pairs]
    assert len(set(pairs)) == len(pairs)
    assert g["reba"].dtype == np.int8 and g["rula"].dtype == np.int8
    assert g["reba"].shape == (probes["starts"][-1], 10) and g["rula"].shape == (probes["starts"][-1], 12)
    assert max(abs(v) for i in infos for s in i.values() for v in s.values()) <= 20


def test_oracle_matches_reference_on_every_pair(probes):
    g, st = probes["g"], probes["starts"]
    for n, (a, b, i) in enumerate(probes["pairs"]):
        info = probes["infos"][i]
        for name, packed, cols in (("reba", reba_ref.reba_packed, ck.REBA_COLS), ("rula", rula_ref.rula_packed, ck.RULA_COLS)):
            got, want = packed(g["pose"][a:b], info[name.upper()]), probes[name][st[n]:st[n + 1]]
            d = ck.first_difference(got, want, cols)
            assert d is None, (name, "pair", n, probes["pair_blocks"][n], info[name.upper()], "row", a + d[0], d[1],
                               got[d[0]].tolist(), want[d[0]].tolist())


def test_every_class_product_is_reached_under_every_rule_info(probes):
    rule = [probes["infos"].index(i) for i in score_cases.rule_infos()]
    assert len(rule) == len(set(rule)) == 13
    groups = dict(score_cases.GROUPS, cross=score_cases.CROSS)
    for i in rule:
        for b in RULE_BLOCKS:
            assert len(_rows_of(probes, (b,), i)), (b, probes["infos"][i])
        pose = probes["pose"][_rows_of(probes, ("grid", "cross"), i)]
        for name, angles in groups.items():
            assert ck.reached(pose, angles) == ck.n_classes(angles), (name, probes["infos"][i])
    assert ck.n_classes(score_cases.CROSS) == 1125
    assert {n: ck.n_classes(a) for n, a in groups.items() if n in ("l_upper_arm", "r_upper_arm", "neck", "torso", "l_wrist")} \
        == dict(l_upper_arm=715, r_upper_arm=765, neck=175, torso=275, l_wrist=405)
    # the classifier sees what it should: thresholds exactly, and the doubles next to them
    assert ck.classify([9.999999999999998, 10.0, 10.000000000000002, -11.0, 5e-324, np.nan], (-10, 0, 10)).tolist() == \
        [4, 5, 6, 0, 4, -1]


def test_every_special_value_is_present(probes):
    a, b = probes["blocks"]["specials"]
    pose = probes["g"]["pose"][a:b]
    angles = score_cases.read_angles()
    vals = np.stack([pose[:, J[j], k] for j, k, _ in angles], axis=1)
    assert len(angles) == 28
    for c, (j, k, _) in enumerate(angles):
        others_finite = np.isfinite(np.delete(vals, c, axis=1)).all(axis=1)
        for v in score_cases.SPECIAL_VALUES:
            want = np.array(v, np.float64).view(np.int64)             # bitwise: +0.0 is not -0.0, NaN is NaN
            assert (others_finite & (vals[:, c].view(np.int64) == want)).any(), (j, k, v)
    for j, x, y in score_cases.PAIRS_READ_TOGETHER:
        for here, partner in ((x, y), (y, x)):
            th = score_cases.thresholds_of(j, partner)
            cls = ck.classify(pose[:, J[j], partner], th)
            for name, hit in (("nan", np.isnan(pose[:, J[j], here])), ("+inf", pose[:, J[j], here] == np.inf),
                              ("-inf", pose[:, J[j], here] == -np.inf)):
                assert set(cls[hit].tolist()) >= set(range(2 * len(th) + 1)), (j, here, partner, name)


def test_every_reachable_table_cell_is_read(probes):
    reads = ck.cells_read(probes["reba"], probes["rula"], probes["ri"], probes["ui"])
    for name in ck.TABLES:
        assert ck.unread_cells(reads, name) == UNREACHABLE.get(name, []), name
    # ... and RULA B's neck = 6 row cannot be read: over the whole product of the Neck classes (and every special value)
    # the neck sub-score stays at or below 5, and it is the same under every info, so no info field feeds it
    pose = probes["pose"][_rows_of(probes, ("grid",))]
    assert ck.reached(pose, score_cases.GROUPS["neck"]) == 175
    assert probes["rula"][:, 9].max() == 5
    first = {}
    for n, b in enumerate(probes["pair_blocks"]):
        neck = probes["rula"][probes["starts"][n]:probes["starts"][n + 1], 9]
        np.testing.assert_array_equal(neck, first.setdefault(b, neck))
    fields = {k for i in probes["infos"] for k, v in i["RULA"].items() if v != 0}
    assert fields == set(RULA_INFO_KEYS)           # every field was non-zero somewhere while the neck column stood still


def test_every_table_mutant_is_noticed(probes):
    alive = ck.surviving_mutants(probes["pose"], probes["ri"], probes["ui"], probes["reba"], probes["rula"])
    want = {name: [(c, d) for c in UNREACHABLE.get(name, []) for d in (1, -1)] for name in ck.TABLES}
    assert sum(t.size for t in ck.TABLES.values()) == 505
    assert alive == want, {k: v for k, v in alive.items() if v != want[k]}
    assert sum(len(v) for v in alive.values()) == 24


def _changed(probes, scorer, edit):
    """Does any stored row change when every info's fields go through edit(dict) -> dict?"""
    packed, info, want = (reba_ref.reba_packed, probes["ri"], probes["reba"]) if scorer == "REBA" else \
        (rula_ref.rula_packed, probes["ui"], probes["rula"])
    return not np.array_equal(packed(probes["pose"], edit(dict(info))), want)


@pytest.mark.parametrize("scorer,keys", [("REBA", REBA_INFO_KEYS), ("RULA", RULA_INFO_KEYS)])
def test_every_info_field_mutant_is_noticed(probes, scorer, keys):
    assert not _changed(probes, scorer, lambda d: d)
    for k in keys:
        assert _changed(probes, scorer, lambda d: {**d, k: np.zeros_like(d[k])}), ("zeroed", k)
    for a, b in itertools.combinations(keys, 2):
        swapped = _changed(probes, scorer, lambda d: {**d, a: d[b], b: d[a]})
        assert swapped == ((a, b) not in SUM_PAIRS), ("exchanged", a, b)


def test_record_what_the_older_fixtures_notice(probes):
    """The same two criteria applied to the score inputs the suite had before: scores.npz (6 000 poses under three infos,
    the reference's results) and the 20 000 uniform poses of test_scores_large_batch_against_oracle (EXAMPLE_INFO, the
    oracle's results).  A record, printed; the assertions only say that the probe set is not behind on either."""
    g = golden("scores.npz")
    infos = json.loads(str(g["infos_json"]))
    uniform = np.random.default_rng(11).uniform(-180, 180, (20000, 24, 3))
    n = len(g["pose"])
    all_pose = np.concatenate([g["pose"], uniform])
    names = list(infos) + ["uniform"]
    pose, ri, ui, _ = ck.flatten(all_pose, [(0, n)] * len(infos) + [(n, n + 20000)], list(infos.values()) + [synth.EXAMPLE_INFO])
    reba = np.concatenate([g[f"reba_{k}"] for k in infos] + [reba_ref.reba_packed(uniform, synth.EXAMPLE_INFO["REBA"])])
    rula = np.concatenate([g[f"rula_{k}"] for k in infos] + [rula_ref.rula_packed(uniform, synth.EXAMPLE_INFO["RULA"])])
    print(f"\n[score probes] older fixtures: {len(all_pose)} poses, {len(names)} infos, {len(pose)} rows")
    alive = ck.surviving_mutants(pose, ri, ui, reba, rula)
    reads = ck.cells_read(reba, rula, ri, ui)
    for name, T in ck.TABLES.items():
        print(f"[score probes] {name}: {2 * T.size} mutants, {len(alive[name])} unnoticed by the older fixtures, "
              f"{len(ck.unread_cells(reads, name))} of {T.size} cells never read")
        assert len(alive[name]) >= 2 * len(UNREACHABLE.get(name, []))
    new = probes["pose"][_rows_of(probes, ("grid", "cross"))]
    for name, angles in dict(score_cases.GROUPS, cross=score_cases.CROSS).items():
        old = ck.reached(all_pose, angles)
        print(f"[score probes] {name}: {ck.n_classes(angles)} classes, {old} reached by the older fixtures")
        assert old <= ck.reached(new, angles) == ck.n_classes(angles)
