"""The crop contract on its knife edges, without a GPU: the emulation of tests/crop_cases.py is the oracle's arithmetic, the
selected boxes do tell the contract's order of roundings from the fused one (in integers and in pixels), and
`crop_ref.box_status` says which boxes have a crop at all."""
import collections

import numpy as np
import pytest

import crop_cases as cc
from conftest import measured
from oracle import crop_ref


@pytest.fixture(scope="module")
def chosen():
    return cc.selected()


@pytest.fixture(scope="module")
def noise():
    return np.random.default_rng(11).integers(0, 256, (cc.FRAME_H, cc.FRAME_W, 3), dtype=np.uint8)


def _assert_integers_equal(box, scale):
    X0, Y0, adelta, bdelta = crop_ref.warp_integers(crop_ref.affine_from_bbox(box, scale))
    e = cc.emulate(box, scale, fused=False)
    assert (X0 == e[0]).all() and np.array_equal(Y0, e[1]) and np.array_equal(adelta, e[2]) and \
        np.array_equal(bdelta, e[3]), (box, scale)


def test_emulation_is_the_oracle_on_the_suites_boxes():
    boxes = cc.suite_boxes()
    assert len(boxes) == 126
    for box in boxes:
        _assert_integers_equal(box, 1.2)


def test_emulation_is_the_oracle_on_the_selected_boxes(chosen):
    for _, scale, boxes in chosen:
        for box in boxes:
            _assert_integers_equal(box, scale)


def test_fused_order_differs_somewhere_on_the_suites_boxes_but_crosses_nothing():
    """Why the seeded boxes of test_hip_parity.py never saw the contraction: the fused order changes an integer on a few of
    them, and none of those changes crosses a multiple of 32."""
    differ = 0
    for box in cc.suite_boxes():
        p, f = cc.emulate(box, 1.2, False), cc.emulate(box, 1.2, True)
        differ += int(p[0] != f[0] or not np.array_equal(p[1], f[1]))
        rows, x_moves = cc.crossing(p, f, (241, 317))
        assert len(rows) == 0 and not x_moves, box
    measured("crop_edges.suite_boxes_with_a_fused_integer_changed", differ)


def test_enough_discriminating_boxes_per_family(chosen):
    """The condition of the search: 32 boxes per family at scale 1.2 (8 at 1.0 and at 2.0) from at most 2000 candidates, every
    placement and both size regimes among the 32."""
    for fam, scale, boxes in chosen:
        want = cc.PER_FAMILY if scale == cc.SCALES[0] else cc.PER_EXTRA_SCALE
        _, looked, made = cc.select(fam, scale, want)
        measured(f"crop_edges.{fam}.scale{scale:g}.selected", len(boxes))
        measured(f"crop_edges.{fam}.scale{scale:g}.candidates", looked)
        measured(f"crop_edges.{fam}.scale{scale:g}.knife_edge_candidates", made)
        assert len(boxes) == want and looked <= cc.MAX_CANDIDATES, (fam, scale, len(boxes), looked)
        assert len({tuple(b) for b in boxes}) == want                          # no box twice
        assert boxes.dtype == np.float32
        if scale == cc.SCALES[0]:
            classes = collections.Counter((cc.placement(b, scale), cc.magnifying(b, scale)) for b in boxes)
            assert {c[0] for c in classes} == set(cc.PLACEMENTS), (fam, classes)
            assert {c[1] for c in classes} == {True, False}, (fam, classes)


def test_families_sit_on_their_edges(chosen):
    """Each family is what it says: the stated value is 32 m + 15.5 exactly (y_centre, x_shift), or within 4 ulps of it on a
    row other than the centre row (y_rows)."""
    from fractions import Fraction
    for fam, scale, boxes in chosen:
        for box in boxes:
            sx0, sy0, sx2, sy1 = crop_ref.control_points(box, scale)
            if fam == "y_centre":
                assert (Fraction(sy0) * 1024 - Fraction(31, 2)) % 32 == 0, box
            elif fam == "x_shift":
                assert ((2 * Fraction(sx0) - Fraction(sx2)) * 1024 - Fraction(31, 2)) % 32 == 0, box
            else:
                M = cc._matrix(box, scale, False)
                v = (M[4] * np.arange(cc.S, dtype=np.float64) + M[5]) * 1024.0
                off = np.abs((v - 15.5) / 32 - np.rint((v - 15.5) / 32)) * 32
                near = off <= 4 * np.spacing(np.abs(v))
                near[112] = False
                assert near.any(), box


def test_every_selected_box_is_discriminating(chosen):
    for _, scale, boxes in chosen:
        for box in boxes:
            assert cc.discriminating(box, scale), (box, scale)
            assert not cc.scale_width_matters(box, scale), (box, scale)
            assert crop_ref.box_status(box, scale) == 0


def test_fused_integers_change_pixels_on_every_selected_box(chosen, noise):
    """What makes the GPU test able to fail: the oracle's own pixel arithmetic, fed the fused order's integers, gives another
    crop of a noise frame than the oracle -- for every selected box."""
    changed = []
    for fam, scale, boxes in chosen:
        for box in boxes:
            want = crop_ref.warp_affine_u8(noise, crop_ref.affine_from_bbox(box, scale))
            fused = crop_ref.warp_from_integers(noise, *cc.integers_as_arrays(cc.emulate(box, scale, True)))
            n = int((fused != want).any(2).sum())
            assert n > 0, (fam, scale, box)
            changed.append(n)
    measured("crop_edges.min_pixels_changed_by_fusion", min(changed))


def test_scale_width_boxes_change_pixels(noise):
    """The C entry carries the scale as a float32; the contract multiplies by the double.  These ordinary boxes get another
    crop of a noise frame when the oracle is handed the float32's value, so the GPU test on them can fail."""
    boxes, looked = cc.scale_width_boxes()
    measured("crop_edges.scale_width.selected", len(boxes))
    measured("crop_edges.scale_width.candidates", looked)
    assert len(boxes) == 16 and looked <= cc.MAX_CANDIDATES
    narrow = cc.f32(1.2)
    assert narrow != 1.2
    for box in boxes:
        _assert_integers_equal(box, 1.2)
        _assert_integers_equal(box, narrow)
        a = crop_ref.warp_affine_u8(noise, crop_ref.affine_from_bbox(box, 1.2))
        b = crop_ref.warp_affine_u8(noise, crop_ref.affine_from_bbox(box, narrow))
        assert (a != b).any(), box


def test_oracle_pixels_unchanged_by_the_split():
    """warp_affine_u8 is warp_from_integers of warp_integers, and crop_to_tensor its ToTensor: a fixed digest of one crop."""
    img = np.random.default_rng(3).integers(0, 256, (37, 53, 3), dtype=np.uint8)
    got = crop_ref.crop_to_tensor(img, np.array([20.3, 18.7, 30.1, 25.9], np.float32), 1.2)
    assert got.shape == (3, 224, 224) and got.dtype == np.float32
    patch = crop_ref.warp_affine_u8(img, crop_ref.affine_from_bbox(np.array([20.3, 18.7, 30.1, 25.9], np.float32), 1.2))
    assert np.array_equal(got, crop_ref.to_tensor(patch))
    # exact float bilinear sampling agrees within the fixed-point step (1/32 pixel of gradient + rounding)
    M = crop_ref.invert_affine(crop_ref.affine_from_bbox(np.array([20.3, 18.7, 30.1, 25.9], np.float32), 1.2))
    ys, xs = np.mgrid[0:224, 0:224].astype(np.float64)
    sx, sy = M[0, 0] * xs + M[0, 2], M[1, 1] * ys + M[1, 2]
    inside = (sx >= 0) & (sx <= 52) & (sy >= 0) & (sy <= 36)
    x0, y0 = np.clip(np.floor(sx).astype(int), 0, 51), np.clip(np.floor(sy).astype(int), 0, 35)
    fx, fy = (sx - x0)[..., None], (sy - y0)[..., None]
    f = img.astype(np.float64)
    ref = (f[y0, x0] * (1 - fx) * (1 - fy) + f[y0, x0 + 1] * fx * (1 - fy) + f[y0 + 1, x0] * (1 - fx) * fy +
           f[y0 + 1, x0 + 1] * fx * fy)
    assert np.abs(patch.astype(np.float64) - ref)[inside].max() <= 255 / 32 * 2 + 1


# ---------------------------------------------------------------------------------------------------------------------
# boxes without a defined crop
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("scale", [1.2, 1.0])
def test_box_status_on_its_edges(scale):
    table = cc.status_table(scale)
    names = [name for name, _, _ in table]
    assert len(set(names)) == len(names)
    for name, box, want in table:
        assert box.dtype == np.float32
        assert crop_ref.box_status(box, scale) == want, (name, box)
        crop = crop_ref.crop_to_tensor(np.full((4, 4, 3), 200, np.uint8), box, scale)
        assert crop.shape == (3, 224, 224) and crop.dtype == np.float32
        if want:
            assert not crop.any(), name


def test_status_table_entries_are_where_they_claim():
    """The table's edges are derived, not guessed: the absorbed side is the last float32 that vanishes in the centre's
    rounding, the limit entries put a control value on 2^18 and on the float32 after it."""
    lim = crop_ref.BOX_LIMIT
    above = float(np.nextafter(np.float32(lim), np.float32(np.inf)))
    t = {name: (box, want) for name, box, want in cc.status_table(1.2)}
    for c in (0.5, 300.0, 5000.0):
        last, first = t[f"w_absorbed_at_{c:g}"][0], t[f"w_not_absorbed_at_{c:g}"][0]
        assert first[2] == np.nextafter(last[2], np.float32(np.inf))
        sx0, _, sx2, _ = crop_ref.control_points(last, 1.2)
        assert sx2 == sx0 == c
        sx0, _, sx2, _ = crop_ref.control_points(first, 1.2)
        assert sx2 == float(np.nextafter(np.float32(c), np.float32(np.inf)))
        # half an ulp of cx: the half-extent at which absorption ends
        assert cc.f32(float(last[2]) * 1.2 * 0.5) == float(np.spacing(np.float32(c))) / 2
    assert crop_ref.control_points(t["cx_far_at_limit"][0], 1.2)[2] == lim
    assert crop_ref.control_points(t["cx_far_above_limit"][0], 1.2)[2] == above
    assert crop_ref.control_points(t["cy_far_at_limit"][0], 1.2)[3] == lim
    assert crop_ref.control_points(t["cy_far_above_limit"][0], 1.2)[3] == above
    assert crop_ref.control_points(t["cx_at_minus_limit"][0], 1.2)[0] == -lim
    # w * scale is beyond float32 there; the contract halves it in double first, so the control value is finite and huge
    assert float(t["w_times_scale_overflows"][0][2]) * 1.2 > float(np.finfo(np.float32).max)
    assert lim < crop_ref.control_points(t["w_times_scale_overflows"][0], 1.2)[2] < np.inf
    # in-domain integers fit int32: the extreme in-domain box of the table
    X0, Y0, adelta, bdelta = crop_ref.warp_integers(crop_ref.affine_from_bbox(t["cx_far_at_limit"][0], 1.2))
    assert max(np.abs(X0).max() + np.abs(adelta).max(), np.abs(Y0).max() + np.abs(bdelta).max()) < 2 ** 31


def test_degenerate_box_raised_before_and_is_refused_now():
    box = np.array([100.0, 80.0, 0.0, 50.0], np.float32)
    with pytest.raises(ZeroDivisionError):
        crop_ref.affine_from_bbox(box, 1.2)
    assert crop_ref.box_status(box, 1.2) == 2
