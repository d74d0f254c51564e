"""The multi-scan JPEG decoder's two halves on the CPU, under ASan + UBSan.

`csrc/jpeg_scans_host.cc` (the scan-aware parser) and `csrc/jpeg_scans.hip` (the per-level entropy kernel, compiled unchanged
for the host against `tests/native/host_shim.h`), with `csrc/jpeg_host.cc` and `csrc/jpeg.hip` behind them, are built
by g++ into one stand-alone driver, tests/native/jpeg_scans_native.cc, which handles every stream on its own in exact-size heap
blocks.  Checked here, without a GPU: every fixture and every transcoded stream byte for byte against libjpeg's pixels, RGB and
BGR; one progressive stream cut at every byte offset and corrupted 2000 times (no sanitizer report; refused, or ranges inside
the buffer; a stream the reference cannot decode ends with a non-zero status, one it can equals the reference).  Robustness
against bad streams is proven HERE; tests/test_jpeg_scans_gpu.py runs six of these streams once."""
import numpy as np
import pytest

import host_build
import jpeg_cases as jc
import jpeg_scans_cases as sc
import jpeg_scans_ref as sr
from poserisk_release_amd import jpeg

SOURCES = ("jpeg_scans_native.cc", "jpeg_host.cc", "jpeg_scans_host.cc", "jpeg.hip", "jpeg_scans.hip")


@pytest.fixture(scope="module")
def each(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_scans_native")
    exe = host_build.build(d, "jpeg_scans_native", SOURCES[0], sources=SOURCES[1:], stage=SOURCES[1:], shim=True)

    def run(streams, bgr=0):
        """-> per stream dict(parse_status, counts, status, and for an accepted one frame, segments, segment_scan, scans, pixels)"""
        exe.run("each", host_build.pack_streams(d / "pack.bin", streams), d / "out.bin", bgr)
        take, out = host_build.taker(d / "out.bin"), []
        for _ in streams:
            head = take(np.int32, 10)
            rec = dict(parse_status=int(head[0]), counts=head[1:9].copy(), status=int(head[9]))
            if rec["parse_status"] == 0:
                rec["frame"] = take(jpeg.FRAME_DTYPE, 1)[0]
                rec["segments"] = take(jpeg.SEGMENT_DTYPE, int(head[1]))
                rec["segment_scan"] = take(np.int32, int(head[1]))
                rec["scans"] = take(jpeg.SCAN_DTYPE, int(head[5]))
                take(jpeg.HUFF_DTYPE, int(head[2]))
                rec["pixels"] = take(np.uint8, int(head[3]) * int(head[4]) * 3).reshape(int(head[3]), int(head[4]), 3)
            out.append(rec)
        take.done()
        return out
    return run


def test_every_fixture_and_every_transcoded_stream_is_byte_exact_rgb_and_bgr(each):
    cases = sc.all_small()
    assert len(cases) == 35 + len(sc.TRANSCODED)
    for bgr in (0, 1):
        got = each([s for _, s, _ in cases], bgr)
        for (name, stream, want), rec in zip(cases, got):
            assert rec["parse_status"] == 0 and rec["status"] == 0, (name, rec["parse_status"], rec["status"])
            bad = np.argwhere(rec["pixels"] != (want[..., ::-1] if bgr else want))
            assert bad.size == 0, f"{name} bgr={bgr}: {len(bad)} bytes differ, first (row, col, channel) {bad[0].tolist()}"
            p = sr.parse(stream)
            assert [int(s["level"]) for s in rec["scans"]] == [s["level"] for s in p["scans"]], name
            assert [(int(s["begin"]), int(s["end"]), int(s["first_mcu"])) for s in rec["segments"]] == \
                [seg for s in p["scans"] for seg in s["segments"]], name


def test_baseline_streams_get_the_pixels_of_the_single_scan_decoder(each):
    """The mixed-call rule: a frame pr_jpeg_parse accepts is one sequential scan at level 0 for this entry."""
    cases = [c for c in jc.small_cases() if c[0].startswith(("33x17", "37x29"))]
    for (name, _, want), rec in zip(cases, each([s for _, s, _ in cases])):
        assert rec["parse_status"] == 0 and rec["status"] == 0 and rec["counts"][4] == 1 and rec["counts"][5] == 1, name
        assert np.array_equal(rec["pixels"], want), name


def test_truncated_and_corrupted_progressive_streams_end_in_a_refusal_or_a_status(each):
    base = sc.fuzz_base()
    p = sr.parse(base)
    assert (p["width"], p["height"], p["hs"], p["vs"], p["progressive"]) == (33, 17, 2, 2, True) and len(p["scans"]) == 10
    cut, hit = jc.truncations(base), sc.corruptions(base)
    assert len(cut) == len(base) and len(hit) == 2000
    got = each(cut + hit)                                  # the driver checks every accepted stream's ranges against its block
    assert all(r["parse_status"] != 0 for r in got[:len(cut)]), "a stream without its EOI was accepted"
    accepted = bad = 0
    for i, (s, rec) in enumerate(zip(hit, got[len(cut):])):
        want = sr.verdict(s)
        if rec["parse_status"] != 0:
            continue                                       # which refusal damaged bytes get is not part of the contract
        accepted += 1
        assert not (isinstance(want, str) and want == "refused"), f"corruption {i}: the reference's parser refuses what the library accepts"
        if isinstance(want, str):
            bad += 1
            assert rec["status"] != 0, f"corruption {i} cannot be decoded but came back with status 0"
        else:
            assert rec["status"] == 0, f"corruption {i} is a valid stream but came back with status {rec['status']}"
            np.testing.assert_array_equal(rec["pixels"], want, err_msg=f"corruption {i}")
    print(f"corruptions accepted by the parser: {accepted}, of those undecodable: {bad}")
    assert accepted >= 200 and bad >= 50, (accepted, bad)   # the corruptions do reach the kernels
    chosen = sc.gpu_bad_streams()
    assert len(chosen) == 6
    for i, s in chosen:                                     # what the GPU suite runs has passed here, on the same bytes
        rec = got[len(cut) + i]
        assert s == hit[i] and rec["parse_status"] == 0 and rec["status"] != 0
