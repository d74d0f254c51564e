"""The PNG decoder's two halves on the CPU, under ASan + UBSan.

`csrc/png_host.cc` (the chunk walk) and the ONE-LANE instantiation of `csrc/png_device.h` (bit reader, table construction, symbol
decode, every validation decision, Adler-32, unfilter, colour) are built by g++ into one stand-alone program with its own
main, tests/native/png_native.cc, which handles every file on its own in exact-size heap blocks: the file, the gathered stream,
the inflated scanlines, the pixels.  Checked here, without a GPU: every case byte for byte, RGB and BGR; one stream cut at
every byte offset and corrupted 2000 times (no sanitizer report; every stream refused, flagged or equal to the reference, and
the outcome agrees with zlib).  Robustness against bad streams is proven HERE; tests/test_png_gpu.py runs six of them once.

NOT covered by this program: what only the 64-lane form does -- the 64-wide literal and match stores, the ballot ranks of the
table construction, the lane exchange of the unfilter, the gather kernel's copies.  The GPU tests (byte-exact cases, guard bands
around data, descriptors, workspace and output) cover that code."""
import numpy as np
import pytest

import host_build
import png_cases as pc
import png_ref as ref
from poserisk_release_amd import png


@pytest.fixture(scope="module")
def each(tmp_path_factory):
    d = tmp_path_factory.mktemp("png_native")
    exe = host_build.build(d, "png_native", "png_native.cc")

    def run(files, bgr=0):
        """-> per file dict(parse_status, status, and for an accepted one frame, idat, pixels)"""
        exe.run("each", host_build.pack_streams(d / "pack.bin", files), d / "out.bin", bgr)
        take, out = host_build.taker(d / "out.bin"), []
        for _ in files:
            head = take(np.int32, 8)
            rec = dict(parse_status=int(head[0]), status=int(head[5]))
            if rec["parse_status"] == 0:
                rec["frame"] = take(png.FRAME_DTYPE, 1)[0]
                rec["idat"] = take(png.IDAT_DTYPE, int(head[1]))
                rec["pixels"] = take(np.uint8, int(head[3]) * int(head[4]) * 3).reshape(int(head[3]), int(head[4]), 3)
            out.append(rec)
        take.done()
        return out
    return run


def test_every_case_is_byte_exact_rgb_and_bgr(each):
    cases = list(pc.small_cases()) + list(pc.large_frames())
    for bgr in (0, 1):
        got = each([s for _, s, _ in cases], bgr)
        for (name, blob, want), rec in zip(cases, got):
            assert rec["parse_status"] == 0 and rec["status"] == 0, (name, rec["parse_status"], rec["status"])
            bad = np.argwhere(rec["pixels"] != (want[..., ::-1] if bgr else want))
            assert bad.size == 0, f"{name} bgr={bgr}: {len(bad)} bytes differ, first (row, col, channel) {bad[0].tolist()}"
            assert [(int(g["begin"]), int(g["end"])) for g in rec["idat"]] == ref.parse(blob)["idat"], name


def test_truncated_and_corrupted_streams_end_as_zlib_says(each):
    z, nraw = pc.fuzz_base()
    cut, hit, flip = pc.truncations(z), pc.corruptions(z), pc.xor_mutations(z)
    assert len(cut) == len(z) == len(flip) and len(hit) == 2000
    streams = cut + hit + flip
    got = each([pc.wrap(s) for s in streams])
    assert all(r["parse_status"] != 0 or r["status"] != 0 for r in got[:len(cut)]), "a stream without its end was accepted"
    accepted = flagged = 0
    for i, (s, rec) in enumerate(zip(streams, got)):
        want = ref.zlib_verdict(s, nraw)
        pst, st, px = ref.decode(pc.wrap(s))
        assert rec["parse_status"] == pst, (i, rec["parse_status"], pst)
        if pst:
            assert want is None, f"stream {i}: the parser refuses a zlib header zlib accepts"
            continue
        flagged_here = want is None or bool(st & ref.ST_FILTER)             # zlib knows nothing of filter bytes
        assert (rec["status"] != 0) == flagged_here, f"stream {i}: status {rec['status']}, zlib {'raises' if want is None else 'accepts'}"
        assert rec["status"] == st, (i, rec["status"], st)
        if rec["status"]:
            flagged += 1
        else:
            accepted += 1
            np.testing.assert_array_equal(rec["pixels"], px, err_msg=f"stream {i}")
    print(f"streams flagged by the decoder: {flagged}, accepted: {accepted}")
    assert flagged >= 3000 and accepted >= 1


def test_the_gpu_bad_files_have_passed_here_on_the_same_bytes(each):
    bad = pc.gpu_bad_files()
    got = each([b for _, b, _ in bad])
    for (name, blob, bit), rec in zip(bad, got):
        if bit == ref.ST_REFUSED:
            assert rec["parse_status"] == ref.E_CRC, name
        else:
            assert rec["parse_status"] == 0 and rec["status"] == bit, (name, rec["status"])
            assert np.array_equal(rec["pixels"], ref.decode(blob)[2]), name
