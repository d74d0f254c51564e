"""CPU-only checks of the multi-scan JPEG decoder (include/poserisk_hip.h, section j1b): the Python restatement
(tests/jpeg_scans_ref.py) against libjpeg's pixels on Pillow's progressive files and on every transcoded stream, the scan-aware
host parser through the C ABI against the reference's records, its agreement with pr_jpeg_parse on everything that one accepts,
and every refusal of the progression rules on one mutated stream each."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import jpeg_cases as jc
import jpeg_ref as jr
import jpeg_scans_cases as sc
import jpeg_scans_ref as sr
from conftest import REPO
from poserisk_release_amd import _lib, jpeg
from test_jpeg_native import _expected_table


def test_reference_equals_libjpeg_on_every_fixture_and_every_transcoded_stream():
    cases = sc.all_small()
    assert len(sc.pillow_cases()) == 35 and len(sc.transcoded_cases()) == len(sc.TRANSCODED) >= 15
    for name, stream, want in cases:
        got = sr.decode_strict(stream)
        bad = np.argwhere(got != want)
        assert bad.size == 0, f"{name}: {len(bad)} bytes differ, first (row, col, channel) {bad[0].tolist()}"
    for name, stream, want in cases[::5]:
        assert np.array_equal(sr.decode_strict(stream, bgr=True), want[..., ::-1]), name
    # Pillow's progressive files decode to what the baseline files of the same images decode to
    base = {n: px for n, _, px in jc.small_cases()}
    assert sum(np.array_equal(px, base[n]) for n, _, px in sc.pillow_cases() if n in base) >= 30
    assert os.path.getsize(os.path.join(jc.GOLDEN, "jpeg_progressive.npz")) < 1000000


def test_the_fixtures_are_what_the_issue_names():
    for name, stream, _ in sc.pillow_cases():
        p = sr.parse(stream)
        script = [(tuple(s["comps"]), s["ss"], s["se"], s["ah"], s["al"]) for s in p["scans"]]
        assert p["progressive"] and script == (sr.LIBJPEG_GRAY if "gray" in name else sr.LIBJPEG_COLOUR), name
        assert all((s["restart"] > 0) == ("rst" in name) for s in p["scans"]), name
    for name, stream, sha, pos, val in sc.frames_800x450():
        p = sr.parse(stream)
        assert (p["width"], p["height"], p["hs"], p["vs"], len(p["scans"])) == (800, 450, 2, 2, 10) and len(sha) == 64, name
        assert pos.shape == val.shape == (4096,)
        assert [len(s["segments"]) for s in p["scans"]] == ([29, 57, 29, 29, 57, 57, 29, 29, 29, 57] if "rstrow" in name else [1] * 10)
    # the 800x450 progressive frames hold the pixels of jpeg_frames.npz's baseline frames
    baseline = {n: sha for n, _, sha, *_ in jc.frames_800x450()}
    assert [sha for _, _, sha, *_ in sc.frames_800x450()] == [baseline["420_q95"], baseline["420_q95_rstrow"]]
    by_name = dict((n, s) for n, s, _ in sc.transcoded_cases())
    for name, _, kw in sc.TRANSCODED:
        p = sr.parse(by_name[name])
        assert p["progressive"] == kw.get("progressive", True), name
        if isinstance(kw.get("restart"), list):
            assert [s["restart"] for s in p["scans"]] == kw["restart"] and len(set(kw["restart"])) > 3, name
        if kw.get("restart") == 3:      # not a divisor of a row of blocks: 5 luma blocks a row at 33 and 37 wide
            assert any(len(s["comps"]) == 1 and sr.scan_mcus(p, s["comps"])[0] % 3 and len(s["segments"]) > 1 for s in p["scans"]), name


def _check_records(blobs, got):
    frames, segs, huff, pst, H, W, offsets, scans, seg_scan, levels, multi = got
    n_seg = n_scan = 0
    assert not pst.any()
    for f, blob in enumerate(blobs):
        p = sr.parse(blob)
        fr = frames[f]
        assert (fr["width"], fr["height"], fr["ncomp"], fr["hs"], fr["vs"]) == (p["width"], p["height"], p["ncomp"], p["hs"], p["vs"])
        np.testing.assert_array_equal(fr["quant"][:p["ncomp"]], p["quant"])
        assert fr["first_segment"] == n_seg and fr["n_segments"] == sum(len(s["segments"]) for s in p["scans"])
        for s in p["scans"]:
            rec = scans[n_scan]
            k = len(s["comps"])
            assert (rec["frame"], rec["ncomp"], list(rec["comp"][:k]), list(rec["dc_sel"][:k]), list(rec["ac_sel"][:k])) == \
                (f, k, s["comps"], s["dc_sel"], s["ac_sel"])
            assert (rec["ss"], rec["se"], rec["ah"], rec["al"], rec["restart_interval"], rec["level"], rec["n_mcus"]) == \
                (s["ss"], s["se"], s["ah"], s["al"], s["restart"], s["level"], s["n_mcus"])
            assert rec["first_segment"] == n_seg and rec["n_segments"] == len(s["segments"])
            mine = segs[n_seg:n_seg + len(s["segments"])]
            assert [(int(x["begin"] - offsets[f]), int(x["end"] - offsets[f]), int(x["first_mcu"]), int(x["frame"])) for x in mine] == \
                [(b, e, m, f) for b, e, m in s["segments"]]
            assert (seg_scan[n_seg:n_seg + len(s["segments"])] == n_scan).all()
            tabs = huff[rec["huff_set"]]["tab"]
            for (cls, tid), (bits, vals) in s["huff"].items():
                look, maxcode, valoff = _expected_table(bits, vals)
                tab = tabs[2 * cls + tid]
                assert tab["defined"] == 1
                np.testing.assert_array_equal(tab["look"], look)
                np.testing.assert_array_equal(tab["maxcode"][1:], maxcode[1:])
                np.testing.assert_array_equal(tab["valoff"][1:], valoff[1:])
                np.testing.assert_array_equal(tab["vals"][:len(vals)], vals)
            used = {2 * c + t for c, t in s["huff"]}
            assert all(tabs[i]["defined"] == (i in used) for i in range(4))
            n_seg += len(s["segments"])
            n_scan += 1
    assert n_seg == len(segs) and n_scan == len(scans)
    return scans


def test_the_library_parser_equals_the_reference():
    """Scans, levels, segments with their first MCUs, table sets and the latched quantisers, one call per size."""
    groups = {}
    for name, stream, px in sc.all_small():
        groups.setdefault(px.shape[:2], []).append((name, stream))
    assert len(groups) == 5
    for (H, W), cases in groups.items():
        blobs = [s for _, s in cases]
        got = jpeg.parse_scans(blobs)
        assert got[4:6] == (H, W) and got[10] == len(blobs)
        scans = _check_records(blobs, got)
        assert got[9] == 3 == 1 + max(scans["level"])
        assert len(got[2]) < len(scans)                      # identical table sets are stored once
    one = lambda name: jpeg.parse_scans([next(s for n, s, _ in sc.all_small() if n == name)])
    colour, gray, sof0 = one("48x32_420_q75"), one("48x32_gray_q85"), one("sof0_three_scans_33x17_420")
    assert colour[7]["level"].tolist() == [0, 0, 0, 0, 0, 1, 1, 1, 1, 2] and colour[9] == 3
    assert gray[7]["level"].tolist() == [0, 0, 0, 1, 1, 2] and gray[9] == 3
    assert sof0[7]["level"].tolist() == [0, 0, 0] and sof0[9] == 1 and sof0[10] == 1
    # W = 17 at 4:2:0: 3 luma blocks a row in luma's own scans, 4 in the interleaved DC scan (2 MCUs of 2x2)
    p = one("17x16_420_q75")
    assert p[7]["n_mcus"].tolist() == [2, 6, 2, 2, 6, 6, 2, 2, 2, 6]


def test_a_quantiser_redefined_between_scans_does_not_reach_a_component_already_begun():
    name, stream, want = next(c for c in sc.transcoded_cases() if c[0] == "spectral_33x17_420")
    second = [m.start() for m in re.finditer(b"\xff\xda", stream)][1]
    dqt = b"\xff\xdb\x00\x43\x00" + bytes([1] * 64)
    changed = stream[:second] + dqt + stream[second:]
    got = jpeg.parse_scans([stream, changed])
    assert not got[3].any()
    np.testing.assert_array_equal(got[0]["quant"][0], got[0]["quant"][1])
    assert np.array_equal(sr.decode_strict(changed), want)


def test_frames_the_single_scan_parser_accepts_get_the_same_records():
    groups = {}
    for name, stream, px in jc.small_cases():
        groups.setdefault(px.shape[:2], []).append(stream)
    for blobs in groups.values():
        a = jpeg.parse(blobs)
        b = jpeg.parse_scans(blobs)
        assert not a[3].any() and not b[3].any() and b[10] == 0 and b[9] == 1
        assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes() and a[2].tobytes() == b[2].tobytes()
        assert a[4:6] == b[4:6] and len(b[7]) == len(blobs) and b[8].tolist() == np.repeat(np.arange(len(blobs)), a[0]["n_segments"]).tolist()
        assert (b[7]["level"] == 0).all() and (b[7]["se"] == 63).all() and (b[7]["huff_set"] == a[0]["huff_set"]).all()


def _sos(stream):
    at = [m.start() for m in re.finditer(b"\xff\xda", stream)]
    assert len(at) == len(sr.parse(stream)["scans"])
    return at


def _scan_range(stream, i):
    """[SOS marker of scan i, the marker that ends its entropy-coded data)"""
    begin = _sos(stream)[i]
    pos = begin + 2 + (stream[begin + 2] << 8 | stream[begin + 3])
    while not (stream[pos] == 0xFF and stream[pos + 1] != 0 and not 0xD0 <= stream[pos + 1] <= 0xD7):
        pos += 1
    return begin, pos


def _set(stream, i, ss=None, se=None, ahal=None):
    at = _sos(stream)[i]
    tail = at + 5 + 2 * stream[at + 4]
    b = bytearray(stream)
    for off, v in ((0, ss), (1, se), (2, ahal)):
        if v is not None:
            b[tail + off] = v
    return bytes(b)


def _drop(stream, i):
    a, b = _scan_range(stream, i)
    return stream[:a] + stream[b:]


def test_every_refusal_of_the_progression_rules_is_hit_and_named():
    base = next(s for n, s, _ in sc.pillow_cases() if n == "48x32_420_q75")      # libjpeg's ten-scan script
    a1, b1 = _scan_range(base, 1)
    two_components = base[:a1] + b"\xff\xda\x00\x0a\x02\x01\x00\x02\x11\x01\x05\x02" + base[a1 + 10:]
    bad = [
        (sr.SCAN_BAND, "Ss = 0 and", _set(base, 0, se=5)),                       # an SOF2 scan with Ss = 0 and Se != 0
        (sr.SCAN_AC_COMPONENTS, "more than one component", two_components),
        (sr.SCAN_BAND, "Ss > Se", _set(base, 1, ss=6)),
        (sr.SCAN_BAND, "Al > 13", _set(base, 1, ahal=0x0E)),
        (sr.SCAN_FIRST_AH, "first scan", _set(base, 0, ahal=0x10)),
        (sr.SCAN_REFINE, "previous Al", _set(base, 9, ahal=0x32)),              # Ah = 3 where the coefficients stand at 1
        (sr.SCAN_REFINE, "Ah - 1", _set(base, 9, ahal=0x11)),
        (sr.SCAN_AC_BEFORE_DC, "before that component's first DC scan", _drop(base, 0)),
        (sr.SCAN_REFINE_UNSENT, "never sent", _drop(base, 4)),                   # luma 6..63 never sent, then 1..63 refined
        (sr.SCAN_TWICE, "twice", base[:b1] + base[a1:b1] + base[b1:]),           # scan 1 again
        (sr.SCAN_TWICE, "twice", _set(base, 9, ahal=0x21)),                      # luma 1..63 at Al = 1 again
        (sr.SCAN_INCOMPLETE, "incomplete", _drop(base, 9)),                      # the last refinement missing
    ]
    blobs = [base] + [s for _, _, s in bad]
    got = jpeg.parse_scans(blobs)
    assert got[3].tolist() == [0] + [code for code, _, _ in bad]
    assert [sr.parse_status(b) for b in blobs] == got[3].tolist()
    for code, words, _ in bad:
        assert words in jpeg.scan_refusal_name(code), (code, jpeg.scan_refusal_name(code))
    assert "smooth" in jpeg.scan_refusal_name(sr.SCAN_INCOMPLETE)
    assert (got[0]["ncomp"][1:] == 0).all() and len(got[7]) == 10 and got[10] == 1
    assert {code for code, _, _ in bad} == set(range(16, 24))
    # the codes of the single-scan parser keep their words, and SOF1 / arithmetic / 12 bits stay refused
    assert jpeg.scan_refusal_name(jr.TRUNCATED) == jpeg.refusal_name(jr.TRUNCATED)
    sof = base.index(b"\xff\xc2")
    for code, mutated in ((jr.EXTENDED, base[:sof + 1] + b"\xc1" + base[sof + 2:]), (jr.ARITHMETIC, base[:sof + 1] + b"\xca" + base[sof + 2:]),
                          (jr.PRECISION, base[:sof + 4] + b"\x0c" + base[sof + 5:]), (jr.TRUNCATED, base[:-2])):
        assert jpeg.parse_scans([mutated])[3].tolist() == [code] == [sr.parse_status(mutated)]
    # a sequential file keeps refusing spectral selection
    seq = next(s for n, s, _ in sc.transcoded_cases() if n == "sof0_three_scans_33x17_420")
    assert jpeg.parse_scans([_set(seq, 1, se=5)])[3].tolist() == [jr.PROGRESSIVE]
    assert jpeg.parse_scans([_drop(seq, 2)])[3].tolist() == [sr.SCAN_INCOMPLETE]


def test_the_single_scan_parser_and_the_default_still_refuse_these_files():
    prog = next(s for n, s, _ in sc.pillow_cases() if n == "48x32_420_q75")
    seq = next(s for n, s, _ in sc.transcoded_cases() if n == "sof0_three_scans_33x17_420")
    assert jpeg.parse([prog])[3].tolist() == [jr.PROGRESSIVE] and jpeg.parse([seq])[3].tolist() == [jr.SCANS]
    assert "progressive" in jpeg.refusal_name(jpeg.parse([prog])[3][0])
    import inspect
    assert inspect.signature(jpeg.decode_files).parameters["progressive"].default is False
    assert inspect.signature(jpeg.bad_frames).parameters["progressive"].default is False


def test_new_symbols_are_declared_and_bound_and_the_records_are_the_headers_structs():
    hdr = open(os.path.join(REPO, "include", "poserisk_hip.h")).read()
    plain = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    lib = _lib.load()
    for name in ("pr_jpeg_parse_scans", "pr_jpeg_scan_refusal_name", "pr_jpeg_scans_workspace_bytes", "pr_jpeg_decode_scans"):
        assert re.search(r"\b" + name + r"\s*\(", plain) and name in _lib.SIGNATURES and hasattr(lib, name), name
    assert lib.pr_abi_version() == _lib.ABI_VERSION == 16                    # functions and structs were added, nothing changed
    assert jpeg.SCAN_DTYPE.itemsize == 21 * 4 and C.sizeof(_lib.JpegScansArgs) == C.sizeof(_lib.JpegArgs) + 2 * 8 + 2 * 4
    assert lib.pr_jpeg_scans_workspace_bytes(3, 450, 800) == lib.pr_jpeg_workspace_bytes(3, 450, 800) > 0
    assert "j1b" in hdr and "PR_JPEG_E_SCAN_INCOMPLETE = 23" in hdr and "PR_JPEG_E_COUNT = 16" in hdr
    # argument errors come back by name before any device work (no device here)
    args = _lib.JpegScansArgs()
    args.base.F, args.base.H, args.base.W = 1, 8, 8
    assert lib.pr_jpeg_decode_scans(args, None, 0, None) == -1 and "16..4096" in lib.pr_last_error().decode()
    counts = np.zeros(8, np.int32)
    assert lib.pr_jpeg_parse_scans(None, None, 0, 0, 0, None, None, None, 0, None, 0, None, 0, None, counts.ctypes.data_as(C.c_void_p)) == 0
    assert lib.pr_jpeg_parse_scans(None, None, 1, 0, 0, None, None, None, 0, None, 0, None, 0, None, counts.ctypes.data_as(C.c_void_p)) == -1
