"""What the multi-scan JPEG tests share (not a test module): Pillow's progressive golden streams, the transcoded streams
(jpeg_scans_ref.rescan of baseline golden cases under the scan scripts below, regenerated at test time and checked against the
SHA-256 the generator stored after Pillow had decoded them), the seeded damaged streams and the six of them that also run on
the GPU.  tests/test_jpeg_scans_native.py proves every damaged stream on the host under sanitizers."""
import functools
import hashlib
import os

import numpy as np

import jpeg_cases as jc
import jpeg_scans_ref as sr

GOLDEN = jc.GOLDEN
FUZZ_CASE = "33x17_420_q95_rstrow"    # small, progressive, a restart interval in every scan
FUZZ_SEED, FUZZ_N = 77, 2000

Y, CB, CR, ALL = (0,), (1,), (2,), (0, 1, 2)
SEQ = (0, 63, 0, 0)
SPECTRAL = [(ALL, 0, 0, 0, 0)] + [(c, lo, hi, 0, 0) for c in (Y, CB, CR) for lo, hi in ((1, 5), (6, 63))]
SPECTRAL_GRAY = [(Y, 0, 0, 0, 0), (Y, 1, 5, 0, 0), (Y, 6, 63, 0, 0)]
# chroma AC refined twice (Al 2 -> 1 -> 0), luma DC refined twice, chroma DC in one interleaved scan of two components
TWO_REFINEMENTS = [(Y, 0, 0, 0, 2), ((1, 2), 0, 0, 0, 0), (Y, 1, 63, 0, 0), (CB, 1, 63, 0, 2), (CR, 1, 63, 0, 2), (Y, 0, 0, 2, 1),
                   (CB, 1, 63, 2, 1), (CR, 1, 63, 2, 1), (Y, 0, 0, 1, 0), (CB, 1, 63, 1, 0), (CR, 1, 63, 1, 0)]
# a high band of a smooth image: whole block rows of it are zero, so one EOB run covers many blocks
HIGH_BAND = [(ALL, 0, 0, 0, 0)] + [(c, lo, hi, 0, 0) for c in (Y, CB, CR) for lo, hi in ((1, 20), (21, 63))]
THREE_SCANS = [(Y,) + SEQ, (CB,) + SEQ, (CR,) + SEQ]
Y_THEN_CHROMA = [(Y,) + SEQ, ((1, 2),) + SEQ]

# (name, the baseline golden case it transcodes, rescan's arguments)
TRANSCODED = [
    ("spectral_33x17_420", "33x17_420_q75", dict(script=SPECTRAL)),
    ("spectral_37x29_422", "37x29_422_q90_opt", dict(script=SPECTRAL)),
    ("spectral_48x32_gray", "48x32_gray_q85", dict(script=SPECTRAL_GRAY)),
    ("two_refinements_37x29_420_noise", "37x29_420_q100_noise", dict(script=TWO_REFINEMENTS)),
    ("two_refinements_17x16_444", "17x16_444_q30", dict(script=TWO_REFINEMENTS)),
    ("high_band_160x120_444", "160x120_444_q30", dict(script=HIGH_BAND)),
    ("sof0_three_scans_33x17_420", "33x17_420_q75", dict(script=THREE_SCANS, progressive=False, optimize=False)),
    ("sof0_three_scans_17x16_420", "17x16_420_q75", dict(script=THREE_SCANS, progressive=False)),
    ("sof0_y_then_chroma_37x29_420", "37x29_420_q75", dict(script=Y_THEN_CHROMA, progressive=False)),
    ("sof0_y_then_chroma_48x32_422", "48x32_422_q90_opt", dict(script=Y_THEN_CHROMA, progressive=False, optimize=False)),
    ("sof0_three_scans_rst3_33x17_420", "33x17_420_q75", dict(script=THREE_SCANS, progressive=False, restart=3)),
    ("sof0_three_scans_rst3_37x29_422", "37x29_422_q60_rst3", dict(script=THREE_SCANS, progressive=False, restart=3, optimize=False)),
    ("libjpeg_script_rst3_33x17_420", "33x17_420_q75", dict(script=sr.LIBJPEG_COLOUR, restart=3)),
    ("libjpeg_script_rst3_37x29_420_noise", "37x29_420_q100_noise", dict(script=sr.LIBJPEG_COLOUR, restart=3)),
    ("libjpeg_script_dri_changes_37x29_422", "37x29_422_q90_opt", dict(script=sr.LIBJPEG_COLOUR, restart=[0, 3, 5, 0, 2, 4, 1, 3, 0, 7])),
    ("libjpeg_script_standard_tables_48x32_420", "48x32_420_q75", dict(script=sr.LIBJPEG_COLOUR, optimize=False)),
    ("libjpeg_gray_script_rst3_33x17", "33x17_gray_q85", dict(script=sr.LIBJPEG_GRAY, restart=3)),
]
EOBRUN_CASE, EOBRUN_AT_LEAST = "high_band_160x120_444", 32


@functools.lru_cache(maxsize=None)
def _npz():
    return np.load(os.path.join(GOLDEN, "jpeg_progressive.npz"))


@functools.lru_cache(maxsize=None)
def pillow_cases():
    """[(name, progressive stream bytes as Pillow wrote it, pixels u8[H,W,3] RGB as Pillow decoded them)]"""
    z = _npz()
    off, s = z["offsets"], z["streams"]
    return [(str(n), s[off[i]:off[i + 1]].tobytes(), z[f"px_{i}"]) for i, n in enumerate(z["names"])]


@functools.lru_cache(maxsize=None)
def transcoded_cases(check=True):
    """[(name, stream bytes, the source case's golden pixels)]: regenerated, and the very bytes Pillow decoded for the generator"""
    want = {}
    if check:
        z = _npz()
        want = dict(zip((str(n) for n in z["transcoded_names"]), (str(h) for h in z["transcoded_sha256"])))
    src = {n: (s, px) for n, s, px in jc.small_cases()}
    out = []
    for name, source, kw in TRANSCODED:
        stats = {}
        stream = sr.rescan(src[source][0], stats=stats, **kw)
        if check:
            assert hashlib.sha256(stream).hexdigest() == want[name], f"{name}: rescan no longer writes the bytes Pillow checked"
        if name == EOBRUN_CASE:
            assert stats["eobrun"] >= EOBRUN_AT_LEAST, stats
        out.append((name, stream, src[source][1]))
    return out


def all_small():
    return pillow_cases() + transcoded_cases()


def frames_800x450():
    """[(name, progressive stream bytes, sha256 hex of the RGB pixels, sample positions, sample values)]"""
    z = _npz()
    off, s = z["frame_offsets"], z["frame_streams"]
    return [(str(n), s[off[i]:off[i + 1]].tobytes(), str(z["frame_sha256"][i]), z["frame_sample_pos"][i], z["frame_sample_val"][i])
            for i, n in enumerate(z["frame_names"])]


def fuzz_base():
    return next(s for n, s, _ in pillow_cases() if n == FUZZ_CASE)


def corruptions(stream):
    return jc.corruptions(stream, FUZZ_N, FUZZ_SEED)


def gpu_bad_streams(count=6):
    """The first `count` corruptions of the fuzz stream that the parser accepts at the original size and that cannot be decoded
    (jpeg_cases.gpu_bad_streams' rule): the device must give each a non-zero status.  [(index among the corruptions, bytes)]"""
    base = fuzz_base()
    size = sr.parse(base)
    out = []
    for i, s in enumerate(corruptions(base)):
        try:
            p = sr.parse(s)
        except sr.Refused:
            continue
        if (p["width"], p["height"]) != (size["width"], size["height"]):
            continue
        if isinstance(sr.verdict(s), str):
            out.append((i, s))
            if len(out) == count:
                break
    return out
