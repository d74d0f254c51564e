"""CPU: the comparison of tests/test_conv_rect_gpu.py (conv_rect_cases.check: the project's own fp32 / bf16 criteria against the
fp64 reference) can fail.  It is fed the index-explicit restatement of the convolution (conv_rect_cases.conv_indexed) with one
index formula changed the way a kernel could plausibly have it, rounded to the family's storage type; every defect must be
rejected on every case whose indices it changes, while the same route without a defect passes everywhere -- and on the square
twins of the suite's older shapes the defects that only exchange the two extents change nothing at all, which is the gap the
rectangular cases close."""
from math import gcd

import numpy as np
import pytest
import torch

import conv_rect_cases as rc
import kernel_refs as kr

# (case, with residual, pixel enumeration): every way the GPU test runs a case
RUNS = [(c, r, t) for c in rc.CASES for r in rc.FAMILIES[c.family].residual for t in rc.tiles(c)]
_id = lambda run: f"{run[0].name}{'-res' if run[1] else ''}{f'-tile{run[2]}' if run[2] else ''}"


def test_enough_cases():
    """The conditions the case table was chosen by, asserted about the table itself."""
    assert all(c.H != c.W for c in rc.CASES)
    assert 2 * sum(gcd(c.H * c.W, 64) == 1 for c in rc.CASES) >= len(rc.CASES)
    assert {c.family for c in rc.CASES} == set(rc.FAMILIES)
    for family in rc.FAMILIES:
        cs = rc.of_family(family)
        assert any(c.H > c.W for c in cs) and any(c.H < c.W for c in cs), family
        if any(c.k == 3 for c in cs):
            assert any(c.k == 3 and c.W <= 2 and c.H >= 5 for c in cs), f"{family}: no map narrower than the kernel"
            assert any(c.k == 3 and c.H == 1 for c in cs), f"{family}: no single-row map"
        assert any(c.B >= 2 for c in cs), f"{family}: the image pitch H * W is never exercised"
    for c in rc.CASES:
        Ho, Wo = rc.out_extent(c)
        if c.stride == 2:
            assert (Ho + Wo) % 2 == 1, f"{c.name}: {Ho} x {Wo}"
        if c.c2:
            assert (c.H2 - 1) // 2 + 1 == c.H and (c.W2 - 1) // 2 + 1 == c.W, c.name
        if c.family == "wino":      # th != tw under F(2x2) and F(4x4)
            assert all(-(-c.H // t) != -(-c.W // t) for t in (2, 4)), c.name
    assert sum(c.H % 4 != 0 and c.W % 4 != 0 for c in rc.of_family("wino")) >= 2
    for family in ("dual_f32", "dual_bf16"):
        mixes = {(c.H2 == 2 * c.H - 1, c.W2 == 2 * c.W - 1) for c in rc.of_family(family)}
        assert {(True, False), (False, True)} <= mixes, family
    # the 64x64 kernel's whole tiles and quarter tail (more than one round of 256), cfg 11's whole 256-row tile
    assert any(-(-c.B * c.H * c.W // 64) * (c.cout // 64) > 256 for c in rc.of_family("tile_f32") if c.k == 1 and c.stride == 1)
    assert any(c.B * c.H * c.W >= 256 for c in rc.of_family("tile_bf16") if c.stride == 1)
    assert any(c.cin_real < c.cin and c.k == 7 for c in rc.of_family("tile_f32"))
    assert set(rc.EXTENT_DEFECTS) < set(rc.DEFECTS)


@pytest.mark.parametrize("run", RUNS, ids=_id)
def test_route_without_a_defect_is_the_fp64_reference_and_passes(run):
    c, with_res, tile = run
    y = rc.indexed(c, with_res, None, tile)
    if c.family == "fused_bf16":      # (the route rounds the map between the convolutions; the fp64 reference does not)
        d = rc.data(c)
        t2 = rc.conv_indexed(d["x"], d["w"], d["bias"], None, 1, 1, True)
        exact = rc.conv_indexed(t2, d["w3"].reshape(c.n3, 64, 1, 1), d["bias3"], d["res3"] if with_res else None, 1, 0, True)
    else:
        exact = y
    ref = rc.reference(c, with_res).numpy()
    assert exact.shape == ref.shape and np.abs(exact - ref).max() <= 1e-12
    rc.check(c, with_res, rc.stored(c, y), run)


@pytest.mark.parametrize("defect", rc.DEFECTS)
def test_defect_is_rejected_wherever_it_applies(defect):
    applied, survived = set(), []
    for c, with_res, tile in RUNS:
        if not rc.applies(c, with_res, defect, tile):
            continue
        applied.add(c.name)
        if rc.passes(c, with_res, rc.stored(c, rc.indexed(c, with_res, defect, tile))):
            survived.append(_id((c, with_res, tile)))
    assert len(applied) >= 5, f"{defect} applies to {len(applied)} cases only"
    assert not survived, f"{defect} passes the comparison on {survived}"


# the square twins of three shapes the suite had before: test_guard_band_gpu.py's 3x3 (1, 9, 9), stride-2 (2, 5, 5), dual (1, 5, 5)
SQUARE_TWINS = [rc._case("tile_f32", 1, 9, 9, 64, 64, 3), rc._case("wino", 1, 9, 9, 64, 192, 3), rc._case("tile_f32", 2, 5, 5, 64, 128, 3, 2),
                rc._case("dual_f32", 1, 5, 5, 64, 64, H2=9, W2=9, c2=128)]


@pytest.mark.parametrize("c", SQUARE_TWINS, ids=lambda c: c.name)
def test_on_square_maps_the_extent_defects_pass_unnoticed(c):
    """The gap: with H == W these defects gather through the very same indices, so the output is the clean one bit for bit and no
    test on a square map can see them.  (On the rectangular cases each of them changes the indices and is rejected: above.)"""
    for tile in rc.tiles(c):
        clean = rc.indexed(c, True, None, tile)
        for defect in rc.EXTENT_DEFECTS:
            assert not rc.applies(c, True, defect, tile), (defect, tile)
            assert np.array_equal(rc.indexed(c, True, defect, tile), clean), (defect, tile)
        assert rc.passes(c, True, rc.stored(c, clean))


def test_an_address_outside_the_tensor_reads_zero_not_a_neighbour():
    """The restatement's own edge: a defect that runs past the tensor (H as the pitch of a tall map) gathers 0 there, it does not
    wrap around or fail."""
    x = torch.ones(1, 5, 2, 4)
    w = np.ones((4, 4, 1, 1))
    clean = rc.conv_indexed(x, w, None, None, 1, 0, False)
    bad = rc.conv_indexed(x, w, None, None, 1, 0, False, defect="pitch_H")
    assert clean.shape == (1, 5, 2, 4) and (clean == 4).all()
    assert (bad[0, :2] == 4).all() and (bad[0, 2:] == 0).all()       # rows 2 .. 4 start at pixel 10, 15, 20 of 10
    assert float(kr.conv_ref64(x, w).sub(torch.from_numpy(clean)).abs().max()) == 0
