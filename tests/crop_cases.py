"""Knife-edge boxes for the crop kernel, and the table of boxes that have no defined crop.

The crop contract (oracle/crop_ref.py, include/poserisk_hip.h f-1) rounds every double operation on its own.  A compiler that
contracts `a * b + c` into one fused multiply-add changes some doubles by an ulp, and that shows only where
rint(v * 1024) + 16 sits next to a multiple of 32 -- which three float32 box families reach by algebra, not by chance:

  y_centre  row 112 of the crop samples the source at M4 * 112 + M5 = cy up to rounding noise: cy = (32 m + 15.5) / 1024.
  x_shift   every row has X0 = rint(M2 * 1024) + 16 and M2 = 2 sx0 - sx2 up to rounding noise: (2 sx0 - sx2) * 1024 = 32 m + 15.5.
  y_rows    with sy1 - sy0 = 112 j / 2^s the row step M4 is j / 2^s up to rounding noise, and cy is searched (at that fixed h)
            so that another row y lands on 32 m + 15.5.

`emulate` restates the contract's integers in Python floats, in the contract's order or with exactly the multiply-adds fused
that a contracting compiler fuses.  A candidate is kept when the two orders differ in an integer whose change crosses a
multiple of 32 on a tap that reads the frame.  Everything is generated from fixed seeds.
"""
import math
from fractions import Fraction

import numpy as np

from oracle import crop_ref

S = 224
FRAME_H, FRAME_W = 240, 320
PER_FAMILY = 32                 # discriminating boxes per family at the project's scale
PER_EXTRA_SCALE = 8             # and at each scale whose half-extent is exact
MAX_CANDIDATES = 2000
FAMILIES = ("y_centre", "x_shift", "y_rows")
SCALES = (1.2, 1.0, 2.0)

if hasattr(math, "fma"):
    fma = math.fma
else:
    def fma(a, b, c):
        """a * b + c rounded once (finite arguments)."""
        return float(Fraction(a) * Fraction(b) + Fraction(c))


def f32(v):
    return float(np.float32(v))


def _matrix(bbox, scale, fused):
    """The inverse matrix (M0, M1, M2, M3, M4, M5) as the contract forms it; fused: with `112 - a sx0`, `112 - d sy0`, the
    determinant and b1 / b2 as fused multiply-adds."""
    sx0, sy0, sx2, sy1 = crop_ref.control_points(bbox, scale)
    a, d = 112.0 / (sx2 - sx0), 112.0 / (sy1 - sy0)
    if fused:
        m2, m5 = fma(-a, sx0, 112.0), fma(-d, sy0, 112.0)
        D = fma(a, d, -(0.0 * 0.0))
    else:
        m2, m5 = 112.0 - a * sx0, 112.0 - d * sy0
        D = a * d - 0.0 * 0.0
    D = 1.0 / D if D != 0 else 0.0
    M0, M4 = d * D, a * D
    M1, M3 = 0.0 * -D, 0.0 * -D
    if fused:       # one product of each pair is an exact zero: the same doubles either way
        b1, b2 = fma(-M0, m2, -(M1 * m5)), fma(-M3, m2, -(M4 * m5))
    else:
        b1, b2 = -M0 * m2 - M1 * m5, -M3 * m2 - M4 * m5
    return M0, M1, b1, M3, M4, b2


def emulate(bbox, scale, fused):
    """(X0, Y0[224], adelta[224], bdelta[224]): the fixed-point integers of the crop contract for one float32 box, computed
    in Python floats.  fused = False: every operation rounded on its own, as OpenCV and oracle/crop_ref.py do.  fused = True:
    `112 - a sx0`, `112 - d sy0`, `M1 y + M2`, `M4 y + M5`, b1 and b2 each rounded once."""
    M0, M1, M2, M3, M4, M5 = _matrix(bbox, scale, fused)
    mad = fma if fused else (lambda p, q, r: p * q + r)
    X0 = [round(mad(M1, float(y), M2) * 1024.0) + 16 for y in range(S)]
    assert min(X0) == max(X0)                                  # M1 is a signed zero
    Y0 = np.array([round(mad(M4, float(y), M5) * 1024.0) + 16 for y in range(S)], np.int64)
    adelta = np.array([round(M0 * float(x) * 1024.0) for x in range(S)], np.int64)
    bdelta = np.array([round(M3 * float(x) * 1024.0) for x in range(S)], np.int64)
    return X0[0], Y0, adelta, bdelta


def integers_as_arrays(e):
    """`emulate`'s result in the form crop_ref.warp_from_integers takes."""
    X0, Y0, adelta, bdelta = e
    return np.full(S, X0, np.int64), Y0, adelta, bdelta


def crossing(plain, fused, frame_hw=(FRAME_H, FRAME_W)):
    """Does the fused order move a tap that reads the frame?  -> (rows whose Y >> 5 changes, does X >> 5 change anywhere),
    counting only positions whose 2x2 taps touch the frame under either order."""
    H, W = frame_hw
    Xp, Xf = (plain[0] + plain[2]) >> 5, (fused[0] + fused[2]) >> 5          # [224] columns
    Yp, Yf = (plain[1][:, None] + plain[3][None, :]) >> 5, (fused[1][:, None] + fused[3][None, :]) >> 5

    def inside(v, n):
        return ((v >> 5) >= -1) & ((v >> 5) < n)
    col_ok = inside(Xp, W) | inside(Xf, W)
    row_ok = inside(Yp, H) | inside(Yf, H)                                   # [224,224]
    seen = row_ok & col_ok[None, :]
    rows = np.nonzero(((Yp != Yf) & seen).any(1))[0]
    x_moves = bool(((Xp != Xf)[None, :] & seen).any())
    return rows, x_moves


def discriminating(bbox, scale, frame_hw=(FRAME_H, FRAME_W)):
    rows, x_moves = crossing(emulate(bbox, scale, False), emulate(bbox, scale, True), frame_hw)
    return len(rows) > 0 or x_moves


def scale_width_matters(bbox, scale):
    """The C entry carries `scale` as a float32.  Where the control points differ between the double and the float32 scale
    the crop depends on that width, which is a separate question from the order of roundings: such boxes are not selected."""
    return crop_ref.control_points(bbox, scale) != crop_ref.control_points(bbox, f32(scale))


# ---------------------------------------------------------------------------------------------------------------------
# candidates
# ---------------------------------------------------------------------------------------------------------------------
PLACEMENTS = ("inside", "straddling", "outside")


def placement(bbox, scale, frame_hw=(FRAME_H, FRAME_W)):
    """inside: the scaled box lies within the frame; straddling: its centre does, the box crosses an edge; outside: its centre
    lies off the frame."""
    H, W = frame_hw
    cx, cy, w, h = [float(v) for v in bbox]
    if not (0 <= cx <= W - 1 and 0 <= cy <= H - 1):
        return "outside"
    hx, hy = abs(w) * scale / 2, abs(h) * scale / 2
    return "inside" if cx - hx >= 0 and cx + hx <= W - 1 and cy - hy >= 0 and cy + hy <= H - 1 else "straddling"


def magnifying(bbox, scale):
    """Is a source pixel larger than a crop pixel along y (the axis every family pins)?"""
    return abs(float(bbox[3])) * scale < S


def _centre(rng, place, n, half):
    """A centre coordinate along an axis of n pixels for a box of half-extent `half`."""
    if place == "outside":      # off the frame, the box still reaching a good way in
        off = rng.uniform(1.0, max(2.0, 0.7 * half))
        return -off if rng.integers(2) else n - 1 + off
    if place == "inside" and 2 * half < n - 1:
        return rng.uniform(half, n - 1 - half)
    return rng.uniform(0.0, n - 1.0)


def _size(rng, magnify, scale, place, n):
    """A box side: magnifying (scaled side under 224) or minifying; an `inside` box has to fit the frame."""
    if magnify:
        hi = min(S / scale, (n - 2) / scale if place == "inside" else 1e9)
        return math.exp(rng.uniform(math.log(12.0), math.log(hi * 0.98)))
    return math.exp(rng.uniform(math.log(S / scale * 1.05), math.log(3.0 * n)))


def _snap_half(target_half, scale):
    """A float32 side whose float32 half-extent f32(side * scale / 2) is `target_half` exactly, or None."""
    w = np.float32(2.0 * target_half / scale)
    for cand in (w, np.nextafter(w, np.float32(np.inf)), np.nextafter(w, np.float32(-np.inf))):
        if f32((float(cand) * scale) * 0.5) == target_half:
            return float(cand)
    return None


def _is_f32(fr):
    return Fraction(f32(float(fr))) == fr


def _shape(k):
    """Candidate k's (placement, magnifying): the classes in turn.  An `inside` box that minifies does not exist in a 240-row
    frame (224 / scale rows and more do not fit); such a candidate ends up straddling."""
    return PLACEMENTS[k % 3], bool((k // 3) % 2)


def _candidate_y_centre(rng, k, scale):
    place, magnify = _shape(k)
    h = f32(_size(rng, magnify, scale, place if place != "outside" else "straddling", FRAME_H))
    w = f32(_size(rng, place == "inside" or bool(rng.integers(2)), scale, place, FRAME_W))
    # the tie row is the centre row: cy stays on the frame; an `outside` box is off it along x
    cy0 = _centre(rng, "inside" if place == "inside" else "straddling", FRAME_H, h * scale / 2)
    cx = f32(_centre(rng, place, FRAME_W, w * scale / 2))
    m = int(cy0 * 1024 // 32)
    return np.array([cx, (32 * m + 15.5) / 1024.0, w, h], np.float32)


def _candidate_x_shift(rng, k, scale):
    place, magnify = _shape(k)
    h = f32(_size(rng, magnify, scale, place, FRAME_H))
    half = _size(rng, place == "inside" or bool(rng.integers(2)), scale, place, FRAME_W) * scale / 2
    cx = round(_centre(rng, place, FRAME_W, half) * 2048) / 2048.0           # on the 1/2048 grid: a float32 below 8192
    cy = f32(_centre(rng, "straddling" if place == "outside" and rng.integers(2) else place, FRAME_H, h * scale / 2))
    m = int((cx - half) * 1024 // 32)
    sx2 = 2 * cx - (32 * m + 15.5) / 1024.0                                  # 2 sx0 - sx2 on the knife edge
    w = _snap_half(sx2 - cx, scale)
    if w is None:
        return None
    box = np.array([cx, cy, w, h], np.float32)
    sx0, _, sx2, _ = crop_ref.control_points(box, scale)
    t = (2 * Fraction(sx0) - Fraction(sx2)) * 1024                           # random boxes, kept when the edge is hit exactly
    return box if (t - Fraction(31, 2)) % 32 == 0 else None


def _candidate_y_rows(rng, k, scale, state):
    """Search over cy at fixed h: a fresh h (so a fresh dyadic row step j / 2^s) every 8 candidates, and for it centres that
    put some row other than 112 on 32 m + 15.5."""
    place, magnify = _shape(k // 8)
    if k % 8 == 0 or "h" not in state:
        state.pop("h", None)
        s = int(rng.integers(7, 11))
        half = _size(rng, magnify, scale, place if place != "outside" else "straddling", FRAME_H) * scale / 2
        j = max(1, int(round(half / 112.0 * (1 << s)))) | 1                  # odd: the step's denominator is 2^s
        r = Fraction(112 * j, 1 << s)                                        # sy1 - sy0
        h = _snap_half(float(r), scale)
        if h is None:
            return None
        state.update(h=h, s=s, j=j, r=r)
    h, s, j, r = state["h"], state["s"], state["j"], state["r"]
    w = f32(_size(rng, place == "inside" or bool(rng.integers(2)), scale, place, FRAME_W))
    cx = f32(_centre(rng, place, FRAME_W, w * scale / 2))
    y = int(rng.integers(0, S))
    if y == 112:
        y = 113
    # row y samples cy + (y - 112) j / 2^s: it has to read the frame, and to sit on 32 m + 15.5
    row_src = rng.uniform(0.0, FRAME_H - 1.0)
    m = int(row_src * 1024 // 32)
    cy = Fraction(2 * (32 * m) + 31, 2048) - Fraction((y - 112) * j, 1 << s)
    if not (_is_f32(cy) and _is_f32(cy + r)):
        return None
    box = np.array([cx, float(cy), w, h], np.float32)
    if crop_ref.control_points(box, scale)[3] - float(cy) != float(r):
        return None
    M = _matrix(box, scale, False)
    v = (M[4] * float(y) + M[5]) * 1024.0                                    # within 4 ulps of the edge, or no candidate
    return box if abs(v - (32 * m + 15.5)) <= 4 * np.spacing(v) else None


def _y0_can_differ(box, scale):
    """Cheap necessary condition for the two orders to differ in Y0 or X0 at all (a bound on the fused order's distance from
    the plain one), so that the exact emulation runs on few candidates."""
    Mp, Mf = _matrix(box, scale, False), _matrix(box, scale, True)
    if Mp != Mf:
        return True
    ys = np.arange(S, dtype=np.float64)
    prod = Mp[4] * ys
    v = prod + Mp[5]
    t = v * 1024.0
    gap = np.abs(np.abs(t - np.floor(t)) - 0.5)                              # distance from a rounding tie
    return bool((gap <= 1024.0 * (np.spacing(np.abs(prod)) + np.spacing(np.abs(v))) + np.spacing(np.abs(t))).any())


_SELECTED = {}


def select(family, scale, want):
    """The first `want` discriminating boxes of a family at a scale, from at most MAX_CANDIDATES candidates: (boxes f32[n,4],
    candidates looked at, candidates that were knife-edge boxes at all)."""
    key = (family, scale, want)
    if key in _SELECTED:
        return _SELECTED[key]
    rng = np.random.default_rng([FAMILIES.index(family), int(scale * 10), 20261])
    state, boxes, looked, made = {}, [], 0, 0
    per_class = {}
    while len(boxes) < want and looked < MAX_CANDIDATES:
        k = looked
        looked += 1
        if family == "y_centre":
            box = _candidate_y_centre(rng, k, scale)
        elif family == "x_shift":
            box = _candidate_x_shift(rng, k, scale)
        else:
            box = _candidate_y_rows(rng, k, scale, state)
        if box is None or crop_ref.box_status(box, scale) or scale_width_matters(box, scale):
            continue
        made += 1
        if not _y0_can_differ(box, scale) or not discriminating(box, scale):
            continue
        # no more than a fair share from one class, so that every placement and both size regimes are among the kept boxes
        cls = (placement(box, scale), magnifying(box, scale))
        if per_class.get(cls, 0) >= max(2, want // 4):
            continue
        per_class[cls] = per_class.get(cls, 0) + 1
        boxes.append(box)
    _SELECTED[key] = (np.array(boxes, np.float32).reshape(-1, 4), looked, made)
    return _SELECTED[key]


def selected():
    """[(family, scale, boxes f32[n,4])]: PER_FAMILY boxes per family at scale 1.2, PER_EXTRA_SCALE at 1.0 and at 2.0."""
    return [(fam, sc, select(fam, sc, PER_FAMILY if sc == SCALES[0] else PER_EXTRA_SCALE)[0])
            for fam in FAMILIES for sc in SCALES]


def scale_width_boxes(want=16, scale=1.2):
    """Seeded ordinary boxes (no knife edge aimed at) whose crop depends on the WIDTH of the scale: with the float32 nearest
    to `scale` a control point lands one float32 away and an integer of the warp crosses a multiple of 32 on the frame.  The
    contract multiplies by the double.  -> (boxes f32[want,4], candidates looked at)."""
    rng = np.random.default_rng(20262)
    boxes, looked = [], 0
    while len(boxes) < want and looked < MAX_CANDIDATES:
        looked += 1
        box = np.array([rng.uniform(0, FRAME_W), rng.uniform(0, FRAME_H), math.exp(rng.uniform(math.log(20.0), math.log(600.0))),
                        math.exp(rng.uniform(math.log(20.0), math.log(600.0)))], np.float32)
        if not scale_width_matters(box, scale):
            continue
        rows, x_moves = crossing(emulate(box, scale, False), emulate(box, f32(scale), False))
        if len(rows) > 0 or x_moves:
            boxes.append(box)
    return np.array(boxes, np.float32).reshape(-1, 4), looked


def suite_boxes():
    """The 126 boxes of tests/test_hip_parity.py's two bit-exact crop tests (6 hand-picked + 120 seeded), same seeds."""
    first = np.array([[400.3, 220.7, 150.2, 310.9], [5.0, 5.0, 100.0, 100.0], [790.0, 440.0, 60.5, 200.25],
                      [300.0, 200.0, 224 / 1.2, 224 / 1.2], [400.0, 225.0, 1200.0, 900.0], [123.456, 78.9, 33.3, 44.4]],
                     np.float32)
    rng = np.random.default_rng(77)
    F, H, W, n = 4, 241, 317, 120
    rng.integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    cx = rng.uniform(-0.4 * W, 1.4 * W, n); cy = rng.uniform(-0.4 * H, 1.4 * H, n)
    bw = np.exp(rng.uniform(np.log(2.0), np.log(3.0 * W), n)); bh = np.exp(rng.uniform(np.log(2.0), np.log(3.0 * H), n))
    return np.concatenate([first, np.stack([cx, cy, bw, bh], 1).astype(np.float32)])


# ---------------------------------------------------------------------------------------------------------------------
# boxes without a defined crop (status bit 1) and their nearest neighbours that have one
# ---------------------------------------------------------------------------------------------------------------------
def _absorbed_side(c, scale):
    """The largest float32 side whose half-extent vanishes in f32(c + half), and the next float32 above it."""
    c = np.float32(c)
    up = np.float32(np.inf)
    side = np.float32(np.spacing(c) / scale)                  # half-extent about half an ulp of c: near the threshold
    absorbed = lambda s: f32(float(c) + f32((float(s) * scale) * 0.5)) == float(c)
    while not absorbed(side):
        side = np.nextafter(side, np.float32(0))
    while absorbed(np.nextafter(side, up)):
        side = np.nextafter(side, up)
    return float(side), float(np.nextafter(side, up))


def _side_reaching(c, far, scale):
    """A float32 side that puts the far control value f32(c + f32(side * scale / 2)) on `far` exactly."""
    side = np.float32((far - c) * 2.0 / scale)
    for _ in range(8):
        got = f32(c + f32((float(side) * scale) * 0.5))
        if got == far:
            return float(side)
        side = np.nextafter(side, np.float32(np.inf if got < far else -np.inf))
    raise AssertionError((c, far, scale))


def status_table(scale=1.2):
    """[(name, box f32[4], want status)] on the edges of the rule `crop_ref.box_status` states."""
    t = []
    good = [100.25, 80.5, 60.0, 90.0]
    tiny = float(np.float32(1e-45))                           # the smallest float32 denormal
    for fi, field in ((2, "w"), (3, "h")):
        for name, v in (("zero", 0.0), ("minus_zero", -0.0), ("denormal", tiny), ("minus_denormal", -tiny)):
            b = list(good); b[fi] = v
            t.append((f"{field}_{name}", b, 2))
        for c in (0.5, 300.0, 5000.0):
            last, first = _absorbed_side(c, scale)
            # the same side mirrored: half an ulp below c is a tie that rounds back to c (an even mantissa) -- except under a
            # power of two, where float32 is twice as fine and c - half is a number of its own
            mirrored = 0 if math.frexp(c)[0] == 0.5 else 2
            for name, v, want in (("absorbed", last, 2), ("not_absorbed", first, 0), ("mirrored_absorbed", -last, mirrored)):
                b = list(good); b[fi - 2] = c; b[fi] = v
                t.append((f"{field}_{name}_at_{c:g}", b, want))
        b = list(good); b[fi] = 3e38                         # side * scale overflows float32
        t.append((f"{field}_times_scale_overflows", b, 2))
        b = list(good); b[fi] = -70.0                        # mirrored: finite, defined
        t.append((f"{field}_negative", b, 0))
    for fi, field in enumerate(("cx", "cy", "w", "h")):
        for name, v in (("nan", float("nan")), ("inf", float("inf")), ("minus_inf", float("-inf"))):
            b = list(good); b[fi] = v
            t.append((f"{field}_{name}", b, 2))
    lim = crop_ref.BOX_LIMIT
    above = float(np.nextafter(np.float32(lim), np.float32(np.inf)))
    for fi, field in ((0, "cx"), (1, "cy")):
        for name, v, want in (("at_limit", lim, 0), ("above_limit", above, 2), ("at_minus_limit", -lim, 0),
                              ("below_minus_limit", -above, 2)):
            b = list(good); b[fi] = v; b[fi + 2] = -math.copysign(100.0, v)    # the other control value stays inside the limit
            t.append((f"{field}_{name}", b, want))
        # the far control value (sx2 / sy1) on the limit and just above it, the centre well inside
        for name, far, want in (("far_at_limit", lim, 0), ("far_above_limit", above, 2)):
            b = list(good); b[fi] = 1024.0; b[fi + 2] = _side_reaching(1024.0, far, scale)
            t.append((f"{field}_{name}", b, want))
    t.append(("good", list(good), 0))
    return [(name, np.array(b, np.float32), want) for name, b, want in t]
