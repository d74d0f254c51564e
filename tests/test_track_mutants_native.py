"""The cases of tests/smooth_cases.py and tests/activity_cases.py held to the mutants they exist for (tests/track_mutants.py).

For each mutant the shipped kernel file's text is changed in memory, written into the test's temporary directory, built there
into the same stand-alone host program as tests/test_smooth_native.py / tests/test_activity_native.py build (g++, ASan + UBSan,
tests/host_build.py), and run over the cases named for it: at least one must fail `check` or be reported by a sanitizer.  That
the unmutated source passes the same cases is what the two native files assert, case by case.  Nothing here touches the tree,
the library or a GPU."""
import os

import pytest

import activity_cases as ac
import host_build
import smooth_cases as sc
import track_mutants as tm

DRIVER = {tm.SMOOTH: ("smooth_host", "smooth_host.cc", sc, (sc.TILE,)), tm.ACTIVITY: ("activity_host", "activity_host.cc", ac, (ac.TILE, ac.CHUNK))}


def test_the_list_names_real_cases_and_every_new_family():
    for ident, file, old, new, killers in tm.MUTANTS:
        assert killers and set(killers) <= set(DRIVER[file][2].CASES), ident
        assert old != new
    assert len(set(tm.IDS)) == len(tm.IDS)
    named = {k for m in tm.MUTANTS for k in m[4]}
    for family in ("knife_c_", "sigma_", "many_", "wild_", "nonfinite_", "lattice_", "span_edge", "spread_back"):
        assert any(k.startswith(family) for k in named), family


@pytest.mark.parametrize("ident", tm.IDS)
def test_a_named_case_kills_the_mutant(tmp_path, ident):
    _, file, old, new, killers = tm.MUTANTS[tm.IDS.index(ident)]
    name, main, cases, sizes = DRIVER[file]
    with open(os.path.join(host_build.CSRC, file)) as f:
        shipped = f.read()
    mutated = tm.mutate(shipped, old, new)
    exe = host_build.build(tmp_path, name, main, stage=(file,), shim=True, threads=True, staged_text={file: mutated})
    assert open(tmp_path / file).read() == mutated and open(os.path.join(host_build.CSRC, file)).read() == shipped
    verdicts = {}
    for case in killers:
        r = exe.run(cases.write_case(tmp_path / "case.bin", case), tmp_path / "out.bin", *sizes, check=False)
        if not host_build.clean(r.returncode, r.stderr):
            verdicts[case] = "reported by the program or a sanitizer"
            continue
        try:
            cases.check(case, cases.read_outputs(tmp_path / "out.bin", case))
        except AssertionError as e:
            verdicts[case] = str(e)[:200]
    assert verdicts, f"{ident}: {killers} all pass on the mutated {file}"
