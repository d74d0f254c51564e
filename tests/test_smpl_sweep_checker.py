"""CPU: the comparison of tests/test_smpl_sweep_gpu.py (smpl_cases.check: within twice the float32 oracle's own error of the
float64 restatement) can fail.  It is fed the float32 oracle's output with a defect a kernel could plausibly have; every
defect must be rejected on every case where it can show, while the same route without a defect passes everywhere."""
import numpy as np
import pytest

import smpl_cases as sc

# the smaller cases of every kernel family, all trees, centres, translations and pose kinds among them
NAMES = [c.name for c in sc.CASES if c.B * c.V <= 3000]


def _rejected(name, out):
    _, _, r64, o32 = sc.references(name)
    return [k for k in ("verts", "joints") if not sc.check(out[k], r64[k], o32[k])[0]]


def test_enough_cases():
    cs = [sc.BY_NAME[n] for n in NAMES]
    assert len(cs) >= 40 and {c.tree for c in cs} == set(sc.TREES) and {c.pose for c in cs} == set(sc.POSES)
    assert {(c.center_idx, c.trans) for c in cs} == {(a, b) for a in sc.CENTERS for b in sc.TRANS}


@pytest.mark.parametrize("name", NAMES)
def test_route_without_a_defect_is_the_oracle_and_passes(name):
    _, _, _, o32 = sc.references(name)
    out = sc.mutant(name, None)
    assert np.array_equal(out["verts"], o32["verts"]) and np.array_equal(out["joints"], o32["joints"])
    assert not _rejected(name, out)


@pytest.mark.parametrize("kind", sc.MUTANTS)
def test_defect_is_rejected_wherever_it_applies(kind):
    applied, survived = 0, []
    for name in NAMES:
        out = sc.mutant(name, kind)
        if out is None:
            continue
        applied += 1
        if not _rejected(name, out):
            survived.append(name)
    assert applied >= 5, f"{kind} applies to {applied} cases only"
    assert not survived, f"{kind} passes the comparison on {survived}"
