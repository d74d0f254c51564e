"""The PNG encoder's two halves on the CPU, under ASan + UBSan.

`csrc/png_enc_host.cc` (plan, bound, workspace size) and the ONE-LANE instantiation of `csrc/png_enc_device.h` (filters, adaptive
choice, tokens, code construction, bit layout, stored fallback, checksum algebra) are built by g++ into one stand-alone program
with its own main, tests/native/png_enc_native.cc, which handles every frame on its own in exact-size heap blocks: the pixels,
each segment's staging area of 5 + n bytes, the file of exactly the bound.  Checked here, without a GPU: every case byte for
byte equal to tests/png_enc_ref.py, RGB and BGR, with no sanitizer report; the argument errors by name.

NOT covered by this program: what only the 64-lane form does -- the cross-lane sums, the words several lanes combine into, the
assemble and place kernels.  tests/test_png_encode_gpu.py (byte-exact cases, guard bands) covers that code."""
import numpy as np
import pytest

import host_build
import png_enc_cases as ec


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("png_enc_native")
    exe = host_build.build(d, "png_enc_native", "png_enc_native.cc")

    def run(*args):
        return exe.run(*args).stdout

    def each(frames):
        """[(px RGB or BGR, filter, mode, bgr)] -> the files"""
        with open(d / "pack.bin", "wb") as f:
            f.write(np.int32(len(frames)).tobytes())
            for px, filt, mode, bgr in frames:
                f.write(np.array([px.shape[0], px.shape[1], filt, mode, bgr], np.int32).tobytes() + np.ascontiguousarray(px).tobytes())
        run("each", str(d / "pack.bin"), str(d / "out.bin"))
        raw, pos, out = open(d / "out.bin", "rb").read(), 0, []
        for _ in frames:
            n = int(np.frombuffer(raw[pos:pos + 4], np.int32)[0])
            out.append(raw[pos + 4:pos + 4 + n])
            pos += 4 + n
        assert pos == len(raw)
        return out
    each.run = run
    return each


def test_every_case_is_byte_exact_rgb_and_bgr(native):
    cases = ec.cases()
    for bgr in (0, 1):
        got = native([(c["px"][..., ::-1] if bgr else c["px"], c["filter"], c["mode"], bgr) for c in cases])
        for c, blob in zip(cases, got):
            want = ec.reference(c["name"])[0]
            assert len(blob) == len(want), f"{c['name']} bgr={bgr}: {len(blob)} bytes, the reference has {len(want)}"
            bad = np.nonzero(np.frombuffer(blob, np.uint8) != np.frombuffer(want, np.uint8))[0]
            assert bad.size == 0, f"{c['name']} bgr={bgr}: {bad.size} bytes differ, the first at {bad[0]}"


def test_plan_bound_and_workspace_argument_errors_by_name(native):
    assert native.run("errors").strip() == "ok"
