"""Rectangular maps (H != W) for every stand-alone convolution entry: the case table, seeded inputs with their fp64 references,
the comparison, and an index-explicit float64 restatement of the convolution in which an index defect is ONE changed formula.
(A helper module, not a conftest.)  tests/test_conv_rect_gpu.py runs the kernels on these cases,
tests/test_conv_rect_checker.py proves on the CPU that its comparison rejects every defect below.

Why: pr_conv2d_nhwc, pr_conv1x1_dual_nhwc and pr_conv3x3_conv1x1_nhwc document [B,H,W,C] and decode a pixel from HoWo, Wo, H, W,
H2, W2, th and tw, yet every other test of them builds square maps, on which H as the row pitch, rem / Ho in the decode, wi
tested against H, ho * stride2 paired with W2, th and tw exchanged ... all compute the right answer.

conv_indexed() builds the convolution by gather from the integer formulas the kernels use:
    m -> (img, rem) = (m / HoWo, m % HoWo),  (ho, wo) = (rem / Wo, rem % Wo)
    (hi, wi) = (ho * stride - pad + kh, wo * stride - pad + kw), taken if (unsigned)hi < H and (unsigned)wi < W
    x at ((img * H + hi) * W + wi) * Cin + ci,  x2 at ((img * H2 + ho * stride2) * W2 + wo * stride2) * Cin2 + ci
    the residual and the output at flat row m = (img * Ho + ho) * Wo + wo
With tile = t > 0 the pixels are enumerated as the Winograd forms do, by tiles of t x t (th x tw of them per frame, those that
overhang the map computed and dropped).  An address outside its tensor reads 0, as a buffer descriptor's range check gives.

DEFECTS (each changes one formula; it APPLIES to a case when the index arrays it gathers differ from the clean ones):
    pitch_H             x's row pitch is H
    decode_Ho           (ho, wo) = (rem / Ho, rem % Ho): Ho where the decode divides by Wo (not (rem % Ho, rem / Ho), which
                        transposes a square map too and so is no defect a square test misses)
    bound_w_vs_H        wi tested against H
    bound_h_vs_W        hi tested against W
    pad_rows_only       pad applied to hi but not to wi
    stride_cols_only    stride applied to wo but not to ho
    out_extent_swapped  Ho computed from W, Wo from H
    x2_pitch_Wo         x2's row pitch is Wo * stride2 (differs from W2 where W2 = 2 Wo - 1)
    x2_pitch_H2         x2's row pitch is H2
    wino_tiles_swapped  the output side decodes tile number t as (t / th, t % th): the tile computed at (i, j) lands where the
                        tile-major count with th as the inner extent puts it (tile = t > 0 only)
    res_pitch           the residual is read with row pitch Ho
All but pad_rows_only, stride_cols_only and x2_pitch_Wo only exchange the roles of the two extents: on a square map they are the
clean convolution, bit for bit (test_conv_rect_checker.py::test_on_square_maps_the_extent_defects_pass_unnoticed).

THE CASES (B, H, W; "s2": stride 2).  H != W everywhere; H * W odd in at least half; H > W and H < W in every family; under
stride 2 one of Ho, Wo odd and the other even (so the issue's 5 x 9 / 12 x 7 became 5 x 7 / 13 x 7 there, and the stem's
30 x 22 became 31 x 21); every family with a 3x3 kernel has a map narrower than the kernel (7 x 1) and a single-row map.
  tile_f32   cfg -1, 7, 8       3x3 64->64: 2x5x9, 1x12x7, 2x7x1, 2x1x9;  3x3 s2 64->128: 2x5x7, 1x13x7;  1x1 96->64: 2x5x9,
                                1x12x7;  1x1 s2 64->128: 2x5x7, 1x13x7;  7x7 s2 pad 3, 3 of 4 channels -> 64: 2x31x21;
                                1x1 64->512: 4x20x26 (33 x 8 = 264 tiles of 64x64: whole tiles and a quarter tail)
  splitk     cfg 202, 203, 204  3x3 64->128: 2x9x5, 2x7x1, 2x1x7;  1x1 96->64: 1x5x7
  panel      cfg 100            1x1 128->256: 1x5x3, 2x3x7
  regw       cfg 400            1x1 128->256: 1x5x3;  256->192: 3x7x4, 2x3x5
  wino       cfg -2, -4, -5     3x3 64->192: 2x5x11, 1x9x3, 2x2x7, 1x7x1, 2x1x7;  512->512: 1x9x5 (7 x 5 has th = tw under
                                F(4x4)).  th != tw in every case and form
  tile_bf16  every cfg offered  3x3 64->64 and 128->128: 2x5x9, 1x12x7;  3x3 s2 64->64 and 128->128: 2x5x7, 1x13x7;
                                3x3 128->128: 2x12x11 (264 pixels: one whole 256x64 tile and a tail); 64->64: 2x7x1, 2x1x9
  expand     cfg 300, residual  1x1 128->512 and 256->1024: 1x9x5, 3x5x2, 1x1x3
  bal        cfg 301, 302       1x1 64->128: 1x9x5, 2x5x9;  3x3 192->256: 7x5x3, 2x3x7, 2x7x1, 3x1x5;  3x3 s2 256->256: 2x5x7,
                                1x13x7
  dual_f32   cfg -1, 8, 100     64 + 128 -> 64, stride2 2, (Ho, Wo) / (H2, W2): 1x5x3 / 9x6, 2x3x5 / 6x9, 2x4x7 / 8x13,
                                1x7x2 / 13x3, 1x2x6 / 4x11
  dual_bf16  cfg 13, 300, 301   128 + 256 -> 512, the same maps
  fused_f32  pr_conv3x3_conv1x1 32->64->64 and 64->64->256: 1x5x9, 2x9x4;  32->64->64: 1x7x1, 2x1x5
  fused_bf16                    64->64->256: 1x5x9, 2x9x4, 1x7x1, 2x1x5
Out of scope: pr_stem_pool_nhwc and pr_stem_pool_f32_nhwc are square by signature; pr_conv3x3_wino64_nhwc and the three
pr_bottleneck*_nhwc entries already run rectangular maps (13 x 6, 8 x 12 ...); pr_hmr_* takes fixed 224 x 224 crops."""
import zlib
from collections import namedtuple

import numpy as np
import torch

import kernel_refs as kr

DEFECTS = ("pitch_H", "decode_Ho", "bound_w_vs_H", "bound_h_vs_W", "pad_rows_only", "stride_cols_only", "out_extent_swapped",
           "x2_pitch_Wo", "x2_pitch_H2", "wino_tiles_swapped", "res_pitch")
# those that only exchange the roles of H and W (Ho and Wo, H2 and W2, th and tw)
EXTENT_DEFECTS = ("pitch_H", "decode_Ho", "bound_w_vs_H", "bound_h_vs_W", "out_extent_swapped", "x2_pitch_H2", "wino_tiles_swapped",
                  "res_pitch")


# ------------------------------------------------------------------------------------------------
# the index-explicit restatement
# ------------------------------------------------------------------------------------------------
def _np64(a):
    return None if a is None else (a.detach().cpu().double().numpy() if isinstance(a, torch.Tensor) else np.asarray(a, np.float64))


def _u(a):
    """The kernels' unsigned compare: a negative coordinate becomes a huge one."""
    return np.asarray(a, np.int64).astype(np.uint32)


def conv_indices(B, H, W, k, stride, pad, H2=0, W2=0, stride2=1, defect=None, tile=0):
    """The integer side of conv_indexed: for every computed pixel, in the order the kernel enumerates them,
    pix [P, k, k] flat pixel of x per tap (-1: a tap the bounds tests drop, or an address past the tensor), pix2 [P] flat pixel of
    x2, rrow [P] the residual's row (-1 likewise), dest [P] the output row it is stored to (-1: a pixel of an overhanging tile,
    dropped) -> dict, with Ho, Wo."""
    assert defect is None or defect in DEFECTS, defect
    extent = lambda n: (n + 2 * pad - k) // stride + 1
    Ho, Wo = (extent(W), extent(H)) if defect == "out_extent_swapped" else (extent(H), extent(W))
    HoWo = Ho * Wo
    if tile:
        th, tw = -(-Ho // tile), -(-Wo // tile)
        e = np.arange(B * th * tw * tile * tile, dtype=np.int64)
        p, a, b = e // (tile * tile), e % (tile * tile) // tile, e % tile
        img, t = p // (th * tw), p % (th * tw)
        ho, wo = t // tw * tile + a, t % tw * tile + b
        i2, j2 = (t // th, t % th) if defect == "wino_tiles_swapped" else (t // tw, t % tw)
        oh, ow = i2 * tile + a, j2 * tile + b
        dest = np.where((oh < Ho) & (ow < Wo), (img * Ho + oh) * Wo + ow, -1)
    else:
        m = np.arange(B * HoWo, dtype=np.int64)
        img, rem = m // HoWo, m % HoWo
        ho, wo = (rem // Ho, rem % Ho) if defect == "decode_Ho" else (rem // Wo, rem % Wo)
        dest = m
    kh, kw = np.arange(k)[None, :, None], np.arange(k)[None, None, :]
    hi = (ho * (1 if defect == "stride_cols_only" else stride))[:, None, None] - pad + kh + 0 * kw
    wi = (wo * stride)[:, None, None] - (0 if defect == "pad_rows_only" else pad) + kw + 0 * kh
    ok = (_u(hi) < np.uint32(W if defect == "bound_h_vs_W" else H)) & (_u(wi) < np.uint32(H if defect == "bound_w_vs_H" else W))
    pix = np.where(ok, (img[:, None, None] * H + hi) * (H if defect == "pitch_H" else W) + wi, -1)
    pitch2 = {"x2_pitch_Wo": Wo * stride2, "x2_pitch_H2": H2}.get(defect, W2)
    pix2 = (img * H2 + ho * stride2) * pitch2 + wo * stride2
    rrow = (img * Ho + ho) * (Ho if defect == "res_pitch" else Wo) + wo
    # an address past its tensor reads 0 like a dropped tap: the same index, -1 (so that a defect whose only effect is to
    # turn dropped taps into reads past the last frame does not count as applying)
    inside = lambda idx, n: np.where((idx >= 0) & (idx < n), idx, -1)
    return {"pix": inside(pix, B * H * W), "pix2": inside(pix2, B * H2 * W2), "rrow": inside(rrow, B * HoWo), "dest": dest,
            "Ho": Ho, "Wo": Wo}


def _rows(flat, idx):
    """flat[idx] with 0 where idx is outside flat (a dropped tap, or an address past the tensor: the descriptor's range check)."""
    inside = (idx >= 0) & (idx < flat.shape[0])
    return np.where(inside[..., None], flat[np.where(inside, idx, 0)], 0.0)


def conv_indexed(x, w, bias, res, stride, pad, relu, x2=None, w2=None, stride2=1, defect=None, tile=0):
    """float64 conv2d + bias + second source + residual, ReLU of the NHWC x [B,H,W,Cin] (w [Cout,Cin_real,k,k], the channels behind
    Cin_real unused; x2 [B,H2,W2,Cin2] with w2 [Cout,Cin2]) by gather through conv_indices -> numpy float64 [B,Ho,Wo,Cout]."""
    x, w, bias, res, x2, w2 = (_np64(a) for a in (x, w, bias, res, x2, w2))
    B, H, W, Cin = x.shape
    Cout, Cr, k, _ = w.shape
    H2, W2 = x2.shape[1:3] if x2 is not None else (0, 0)
    ix = conv_indices(B, H, W, k, stride, pad, H2, W2, stride2, defect, tile)
    taps = _rows(x.reshape(B * H * W, Cin), ix["pix"])[..., :Cr]                      # [P, k, k, Cr]
    val = np.einsum("pabc,ocab->po", taps, w)
    if bias is not None:
        val = val + bias
    if x2 is not None:
        val = val + _rows(x2.reshape(B * H2 * W2, -1), ix["pix2"]) @ w2.T
    if res is not None:
        val = val + _rows(res.reshape(-1, Cout), ix["rrow"])
    if relu:
        val = np.maximum(val, 0.0)
    M = B * ix["Ho"] * ix["Wo"]
    y = np.zeros((M, Cout))
    stored = ix["dest"] >= 0
    y[ix["dest"][stored]] = val[stored]
    return y.reshape(B, ix["Ho"], ix["Wo"], Cout)


# ------------------------------------------------------------------------------------------------
# the cases
# ------------------------------------------------------------------------------------------------
# family: its precision, the tile_cfgs its GPU test runs (None: every index pr_conv_num_tile_cfgs() offers), with / without residual
Family = namedtuple("Family", "bf16 cfgs residual")
FAMILIES = {
    "tile_f32": Family(False, (-1, 7, 8), (False, True)),
    "splitk": Family(False, (202, 203, 204), (False, True)),
    "panel": Family(False, (100,), (False, True)),
    "regw": Family(False, (400,), (False, True)),
    "wino": Family(False, (-2, -4, -5), (False,)),
    "tile_bf16": Family(True, None, (True,)),
    "expand": Family(True, (300,), (True,)),
    "bal": Family(True, (301, 302), (False,)),
    "dual_f32": Family(False, (-1, 8, 100), (False,)),
    "dual_bf16": Family(True, (13, 300, 301), (False,)),
    "fused_f32": Family(False, (), (False, True)),
    "fused_bf16": Family(True, (), (False, True)),
}
# the Winograd forms' output tiles: F(2x2,3x3), F(4x4,3x3) on either point set
WINO_TILE = {-2: 2, -4: 4, -5: 4}

# B, H, W: x's map (the dual entries: x1's, which is the output's); cin_real of cin channels; cout: the (first) convolution's output
# channels; k / stride / pad; H2, W2, c2: the second source (dual); n3: conv3's output channels (fused)
Case = namedtuple("Case", "name family B H W cin_real cin cout k stride pad H2 W2 c2 n3")


def _case(family, B, H, W, cin, cout, k=1, stride=1, pad=None, cin_real=None, H2=0, W2=0, c2=0, n3=0):
    pad = k // 2 if pad is None else pad
    name = f"{family}-{B}x{H}x{W}-{cin}to{cout}-k{k}s{stride}" + (f"-x2_{H2}x{W2}" if c2 else "") + (f"-n{n3}" if n3 else "")
    return Case(name, family, B, H, W, cin if cin_real is None else cin_real, cin, cout, k, stride, pad, H2, W2, c2, n3)


def _dual(family, c1, c2, n):
    # (B, Ho, Wo, H2, W2): H2 = 2 Ho - 1 with W2 = 2 Wo, the reverse, and three more mixes
    maps = [(1, 5, 3, 9, 6), (2, 3, 5, 6, 9), (2, 4, 7, 8, 13), (1, 7, 2, 13, 3), (1, 2, 6, 4, 11)]
    return [_case(family, B, Ho, Wo, c1, n, H2=H2, W2=W2, c2=c2) for B, Ho, Wo, H2, W2 in maps]


CASES = (
    [_case("tile_f32", B, H, W, 64, 64, 3) for B, H, W in ((2, 5, 9), (1, 12, 7), (2, 7, 1), (2, 1, 9))] +
    [_case("tile_f32", B, H, W, 64, 128, 3, 2) for B, H, W in ((2, 5, 7), (1, 13, 7))] +
    [_case("tile_f32", B, H, W, 96, 64) for B, H, W in ((2, 5, 9), (1, 12, 7))] +
    [_case("tile_f32", B, H, W, 64, 128, 1, 2) for B, H, W in ((2, 5, 7), (1, 13, 7))] +
    [_case("tile_f32", 2, 31, 21, 4, 64, 7, 2, 3, cin_real=3), _case("tile_f32", 4, 20, 26, 64, 512)] +
    [_case("splitk", B, H, W, 64, 128, 3) for B, H, W in ((2, 9, 5), (2, 7, 1), (2, 1, 7))] + [_case("splitk", 1, 5, 7, 96, 64)] +
    [_case("panel", B, H, W, 128, 256) for B, H, W in ((1, 5, 3), (2, 3, 7))] +
    [_case("regw", 1, 5, 3, 128, 256), _case("regw", 3, 7, 4, 256, 192), _case("regw", 2, 3, 5, 256, 192)] +
    [_case("wino", B, H, W, 64, 192, 3) for B, H, W in ((2, 5, 11), (1, 9, 3), (2, 2, 7), (1, 7, 1), (2, 1, 7))] +
    [_case("wino", 1, 9, 5, 512, 512, 3)] +
    [_case("tile_bf16", B, H, W, c, c, 3) for c in (64, 128) for B, H, W in ((2, 5, 9), (1, 12, 7))] +
    [_case("tile_bf16", B, H, W, c, c, 3, 2) for c in (64, 128) for B, H, W in ((2, 5, 7), (1, 13, 7))] +
    [_case("tile_bf16", 2, 12, 11, 128, 128, 3), _case("tile_bf16", 2, 7, 1, 64, 64, 3), _case("tile_bf16", 2, 1, 9, 64, 64, 3)] +
    [_case("expand", B, H, W, K, N) for K, N in ((128, 512), (256, 1024)) for B, H, W in ((1, 9, 5), (3, 5, 2), (1, 1, 3))] +
    [_case("bal", B, H, W, 64, 128) for B, H, W in ((1, 9, 5), (2, 5, 9))] +
    [_case("bal", B, H, W, 192, 256, 3) for B, H, W in ((7, 5, 3), (2, 3, 7), (2, 7, 1), (3, 1, 5))] +
    [_case("bal", B, H, W, 256, 256, 3, 2) for B, H, W in ((2, 5, 7), (1, 13, 7))] +
    _dual("dual_f32", 64, 128, 64) + _dual("dual_bf16", 128, 256, 512) +
    [_case("fused_f32", B, H, W, cin, 64, 3, n3=n3) for cin, n3 in ((32, 64), (64, 256)) for B, H, W in ((1, 5, 9), (2, 9, 4))] +
    [_case("fused_f32", B, H, W, 32, 64, 3, n3=64) for B, H, W in ((1, 7, 1), (2, 1, 5))] +
    [_case("fused_bf16", B, H, W, 64, 64, 3, n3=256) for B, H, W in ((1, 5, 9), (2, 9, 4), (1, 7, 1), (2, 1, 5))])
BY_NAME = {c.name: c for c in CASES}
assert len(BY_NAME) == len(CASES)


def of_family(family):
    return [c for c in CASES if c.family == family]


def out_extent(c):
    """(Ho, Wo) of the case's (first) convolution."""
    return (c.H + 2 * c.pad - c.k) // c.stride + 1, (c.W + 2 * c.pad - c.k) // c.stride + 1


def tiles(c):
    """The pixel enumerations a case's kernels use: 0 = flat rows, t = tiles of t x t (the Winograd forms)."""
    return (2, 4) if c.family == "wino" else (0,)


# ------------------------------------------------------------------------------------------------
# seeded inputs and their fp64 references: built once per case, shared, never written to
# ------------------------------------------------------------------------------------------------
_DATA = {}


def _randn(rng, shape, bf, scale=1.0):
    t = torch.from_numpy((rng.standard_normal(shape) * scale).astype(np.float32))
    return kr.bf16_round(t) if bf else t


def data(c):
    """-> dict of float32 CPU tensors (bf16 families: rounded to bf16) x, w, res [, x2, w2; w3, res3] and float32 numpy biases."""
    if c.name not in _DATA:
        bf = FAMILIES[c.family].bf16
        rng = np.random.default_rng(zlib.crc32(c.name.encode()))
        Ho, Wo = out_extent(c)
        d = {"x": _randn(rng, (c.B, c.H, c.W, c.cin), bf)}
        d["x"][..., c.cin_real:] = 0
        d["w"] = _randn(rng, (c.cout, c.cin_real, c.k, c.k), bf, 1 / np.sqrt(c.cin_real * c.k * c.k))
        d["bias"] = rng.standard_normal(c.cout).astype(np.float32)
        d["res"] = _randn(rng, (c.B, Ho, Wo, c.cout), bf)
        if c.c2:
            d["x2"] = _randn(rng, (c.B, c.H2, c.W2, c.c2), bf)
            d["w2"] = _randn(rng, (c.cout, c.c2), bf, 1 / np.sqrt(c.c2))
        if c.n3:
            d["w3"] = _randn(rng, (c.n3, 64), bf, 1 / 8)
            d["bias3"] = rng.standard_normal(c.n3).astype(np.float32)
            d["res3"] = _randn(rng, (c.B, c.H, c.W, c.n3), bf)
        _DATA[c.name] = d
    return _DATA[c.name]


def indexed(c, with_res, defect=None, tile=0):
    """The case through conv_indexed (float64 numpy, NHWC), as its entry composes it.  fused_bf16 rounds the map between the two
    convolutions to bf16, as the kernel stores it and its criterion's emulation has it."""
    d = data(c)
    if c.c2:
        return conv_indexed(d["x"], d["w"], d["bias"], None, 1, 0, True, d["x2"], d["w2"], 2, defect=defect)
    if c.n3:
        t2 = conv_indexed(d["x"], d["w"], d["bias"], None, 1, 1, True, defect=defect)
        if c.family == "fused_bf16":
            t2 = kr.bf16_round(torch.from_numpy(t2).float()).double().numpy()
        return conv_indexed(t2, d["w3"].reshape(c.n3, 64, 1, 1), d["bias3"], d["res3"] if with_res else None, 1, 0, True, defect=defect)
    return conv_indexed(d["x"], d["w"], d["bias"], d["res"] if with_res else None, c.stride, c.pad, True, defect=defect, tile=tile)


def index_arrays(c, with_res, defect=None, tile=0):
    """Every index array indexed(c, with_res, defect, tile) gathers or scatters through, in a fixed order."""
    if c.n3:
        parts = [conv_indices(c.B, c.H, c.W, 3, 1, 1, defect=defect), conv_indices(c.B, c.H, c.W, 1, 1, 0, defect=defect)]
        keys = [("pix", "dest"), ("pix", "dest") + (("rrow",) if with_res else ())]
    else:
        parts = [conv_indices(c.B, c.H, c.W, c.k, c.stride, c.pad, c.H2, c.W2, 2 if c.c2 else 1, defect=defect, tile=tile)]
        keys = [("pix", "dest") + (("pix2",) if c.c2 else ()) + (("rrow",) if with_res else ())]
    return [p[k] for p, ks in zip(parts, keys) for k in ks]


def applies(c, with_res, defect, tile=0):
    """Decided from the indices alone: does the defect gather or store anything differently on this case?"""
    clean, bad = index_arrays(c, with_res, None, tile), index_arrays(c, with_res, defect, tile)
    return any(not np.array_equal(a, b) for a, b in zip(clean, bad))


_REFS = {}


def reference(c, with_res):
    """The independent fp64 reference (torch conv2d / einsum in float64: tests/kernel_refs.py) -> float64 tensor, NHWC."""
    if (c.name, with_res) not in _REFS:
        d = data(c)
        if c.c2:
            ref = kr.dual_ref64(d["x"], d["w"][:, :, 0, 0], d["x2"], d["w2"], d["bias"], 2)
        elif c.n3:
            ref = kr.fused_ref64(d["x"], d["w"], d["bias"], d["w3"], d["bias3"], d["res3"] if with_res else None)
        else:
            ref = kr.conv_ref64(d["x"], d["w"], d["bias"], d["res"] if with_res else None, stride=c.stride, pad=c.pad, relu=True)
        _REFS[(c.name, with_res)] = ref
    return _REFS[(c.name, with_res)]


def criterion_reference(c, with_res):
    """What the family's criterion compares with: the fp64 reference; fused_bf16: the fp32 emulation with the map between the
    convolutions rounded to bf16 (kernel_refs.fused_bf16_emulation, test_conv3x3_conv1x1_fused_bf16's)."""
    if c.family != "fused_bf16":
        return reference(c, with_res)
    if (c.name, with_res, "emu") not in _REFS:
        d = data(c)
        _REFS[(c.name, with_res, "emu")] = kr.fused_bf16_emulation(d["x"], d["w"], d["bias"], d["w3"], d["bias3"],
                                                                   d["res3"] if with_res else None)
    return _REFS[(c.name, with_res, "emu")]


def stored(c, y64):
    """A float64 result rounded to the family's storage type -> tensor of that type."""
    return torch.as_tensor(y64).to(torch.bfloat16 if FAMILIES[c.family].bf16 else torch.float32)


def check(c, with_res, got, what=""):
    """The project's own criterion for the family, on a result tensor in its storage type (any device): raises AssertionError.
    fp32: kernel_refs.assert_close_f32 against fp64; a single bf16 convolution: kernel_refs.assert_close_bf16 against fp64;
    fused_bf16: |got - ref| <= |ref| 2^-7 + 2e-2 against the emulation."""
    ref = criterion_reference(c, with_res)
    assert tuple(got.shape) == tuple(ref.shape), (what, tuple(got.shape), tuple(ref.shape))
    if c.family == "fused_bf16":
        d = (got.float().cpu() - ref).abs()
        assert bool((d <= ref.abs() * 2.0 ** -7 + 2e-2).all()), (what, float(d.max()))
    elif FAMILIES[c.family].bf16:
        kr.assert_close_bf16(got, ref, what)
    else:
        kr.assert_close_f32(got, ref, what)


def passes(c, with_res, got):
    try:
        check(c, with_res, got)
    except AssertionError:
        return False
    return True


def scaled_error(c, with_res, got):
    """max |got - fp64| / max(1, max |fp64|): what the GPU test reports per family."""
    ref = reference(c, with_res)
    return float((got.detach().cpu().double() - ref).abs().max()) / max(1.0, float(ref.abs().max()))
