"""The JPEG decoder's two halves on the CPU, under ASan + UBSan.

`csrc/jpeg_host.cc` (the marker parser) and `csrc/jpeg.hip` (the kernels, compiled unchanged for the host against
`tests/native/host_shim.h`: a launch = nested loops over workgroups and threads) are built by g++ into one driver,
tests/native/jpeg_native.cc, which handles every stream on its own in exact-size heap blocks.  Checked here, without a GPU:
the parser's descriptors against tests/jpeg_ref.py, every golden case byte for byte against libjpeg's pixels, one stream cut at
every byte offset and corrupted 2000 times (no sanitizer report; refused, or ranges inside the buffer; a stream that cannot be
decoded ends with a non-zero status, one that can equals the reference), and the 32-bit IDCT at its stated bound against the
64-bit reference.  Robustness against bad streams is proven HERE; tests/test_jpeg_gpu.py runs six of these streams once."""
import numpy as np
import pytest

import host_build
import jpeg_cases as jc
import jpeg_ref as jr
from poserisk_release_amd import jpeg


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_native")
    exe = host_build.build(d, "jpeg_native", "jpeg_native.cc", stage=("jpeg.hip", "jpeg_host.cc"), shim=True)

    def each(streams, bgr=0):
        """-> per stream dict(parse_status, counts, status, and for an accepted one frame, segments, huff, pixels)"""
        exe.run("each", host_build.pack_streams(d / "pack.bin", streams), d / "out.bin", bgr)
        take, out = host_build.taker(d / "out.bin"), []
        for _ in streams:
            head = take(np.int32, 6)
            rec = dict(parse_status=int(head[0]), counts=head[1:5].copy(), status=int(head[5]))
            if rec["parse_status"] == 0:
                rec["frame"] = take(jpeg.FRAME_DTYPE, 1)[0]
                rec["segments"] = take(jpeg.SEGMENT_DTYPE, int(head[1]))
                rec["huff"] = take(jpeg.HUFF_DTYPE, 1)[0]
                rec["pixels"] = take(np.uint8, int(head[3]) * int(head[4]) * 3).reshape(int(head[3]), int(head[4]), 3)
            out.append(rec)
        take.done()
        return out

    def idct(coef, quant):
        with open(d / "idct.bin", "wb") as f:
            f.write(np.asarray(coef, np.int16).tobytes() + np.asarray(quant, np.uint16).tobytes())
        exe.run("idct", d / "idct.bin", d / "idct_out.bin")
        raw = np.fromfile(d / "idct_out.bin", np.uint8)
        return raw[:256].reshape(16, 16), int(raw[256:].view(np.int32)[0])
    return each, idct


def _expected_table(bits, vals):
    """The device's decode table for (bits, vals), built from the standard's definition of the codes."""
    look, maxcode, valoff = np.zeros(512, np.uint16), np.full(17, -1, np.int32), np.zeros(17, np.int32)
    maxcode[0] = 0
    code = k = 0
    for l in range(1, 17):
        valoff[l] = k - code
        for _ in range(bits[l - 1]):
            if l <= 9:
                look[code << (9 - l):(code + 1) << (9 - l)] = l << 8 | vals[k]
            code += 1
            k += 1
        if bits[l - 1]:
            maxcode[l] = code - 1
        code <<= 1
    return look, maxcode, valoff


def test_descriptors_equal_the_reference_parse_and_pixels_equal_libjpeg(native):
    each, _ = native
    cases = jc.small_cases()
    assert len(cases) >= 36
    for bgr in (0, 1):
        got = each([s for _, s, _ in cases], bgr)
        for (name, stream, want), rec in zip(cases, got):
            assert rec["parse_status"] == 0 and rec["status"] == 0, (name, rec["parse_status"], rec["status"])
            bad = np.argwhere(rec["pixels"] != (want[..., ::-1] if bgr else want))
            assert bad.size == 0, f"{name} bgr={bgr}: {len(bad)} bytes differ, first (row, col, channel) {bad[0].tolist()}"
            if bgr:
                continue
            p, fr = jr.parse(stream), rec["frame"]
            assert (fr["width"], fr["height"], fr["ncomp"], fr["hs"], fr["vs"], fr["restart_interval"]) == \
                (p["width"], p["height"], p["ncomp"], p["hs"], p["vs"], p["restart"]), name
            assert fr["first_segment"] == 0 and fr["n_segments"] == len(p["segments"]) and fr["huff_set"] == 0, name
            np.testing.assert_array_equal(fr["quant"][:p["ncomp"]], p["quant"], err_msg=name)
            assert list(fr["dc_sel"][:p["ncomp"]]) == p["dc_sel"] and list(fr["ac_sel"][:p["ncomp"]]) == p["ac_sel"], name
            assert [(int(s["begin"]), int(s["end"]), int(s["first_mcu"])) for s in rec["segments"]] == p["segments"], name
            assert (rec["segments"]["frame"] == 0).all()
            for (cls, tid), (bits, vals) in p["huff"].items():
                tab = rec["huff"]["tab"][2 * cls + tid]
                look, maxcode, valoff = _expected_table(bits, vals)
                assert tab["defined"] == 1, name
                np.testing.assert_array_equal(tab["look"], look, err_msg=name)
                np.testing.assert_array_equal(tab["maxcode"][1:], maxcode[1:], err_msg=name)
                np.testing.assert_array_equal(tab["valoff"][1:], valoff[1:], err_msg=name)
                np.testing.assert_array_equal(tab["vals"][:len(vals)], vals, err_msg=name)
            used = {2 * c + t for c, t in p["huff"]}
            assert all(rec["huff"]["tab"][i]["defined"] == (i in used) for i in range(4)), name
    names = [n for n, _, _ in cases]
    assert any("gray" in n for n in names) and any("q100_noise" in n for n in names) and any("_opt" in n for n in names)
    assert any("rstrow" in n for n in names) and any("rst3" in n for n in names) and any(n.startswith("37x29") for n in names)


def test_truncated_and_corrupted_streams_end_in_a_refusal_or_a_status(native):
    each, _ = native
    base = jc.fuzz_base()
    cut, hit = jc.truncations(base), jc.corruptions(base)
    assert len(cut) == len(base) and len(hit) == 2000
    got = each(cut + hit)                                  # the driver checks every accepted stream's ranges against its block
    assert all(r["parse_status"] != 0 for r in got[:len(cut)]), "a stream without its EOI was accepted"
    accepted = bad = 0
    for i, (s, rec) in enumerate(zip(hit, got[len(cut):])):
        if rec["parse_status"] != 0:
            continue                                       # which refusal damaged bytes get is not part of the contract
        accepted += 1
        want = jc.reference_verdict(s)
        assert not (isinstance(want, str) and want == "refused"), f"corruption {i}: the reference's parser refuses what the library accepts"
        if isinstance(want, str):
            bad += 1
            assert rec["status"] != 0, f"corruption {i} cannot be decoded but came back with status 0"
        else:
            assert rec["status"] == 0, f"corruption {i} is a valid stream but came back with status {rec['status']}"
            np.testing.assert_array_equal(rec["pixels"], want, err_msg=f"corruption {i}")
    assert accepted >= 200 and bad >= 50, (accepted, bad)   # the corruptions do reach the decoder
    chosen = jc.gpu_bad_streams()
    assert len(chosen) == 6
    for i, s in chosen:                                     # what the GPU suite runs has passed here, on the same bytes
        rec = got[len(cut) + i]
        assert s == hit[i] and rec["parse_status"] == 0 and rec["status"] != 0


M = np.array([[8192, 11363, 10703, 9633, 8192, 6437, 4433, 2260], [8192, 9633, 4433, -2259, -8192, -11362, -10704, -6436],
              [8192, 6437, -4433, -11362, -8192, 2261, 10704, 9633], [8192, 2260, -10703, -6436, 8192, 9633, -4433, -11363]])


def test_the_32_bit_idct_equals_the_64_bit_reference_at_its_bound(native):
    """The header's bound: every input of either pass within +-35079 makes the 32-bit evaluation exact.  Blocks 0 and 1 sit on
    it: only row 0 of the block is non-zero, so every pass-1 result of column c is exactly 4 d[0][c]; with d[0][c] = +-8769 in
    the sign pattern of the largest rows of the pass (out2: 61214), pass 2 reaches 61214 * 35076 = 2 147 142 264, within 0.02 %
    of 2^31.  Block 2: every coefficient +-1173, the coefficient-only bound, in the sign pattern that maximises sample (0, 0);
    block 3: the same with random signs."""
    _, idct = native
    assert np.abs(M).sum(1).max() == 61214 and 61214 * jr.IDCT_BOUND + (1 << 17) < 2 ** 31 <= 61214 * (jr.IDCT_BOUND + 3) + (1 << 17)
    rng = np.random.default_rng(3)
    coef = np.zeros((4, 64), np.int64)
    coef[0, :8] = np.sign(M[2]) * 8769
    coef[1, :8] = -np.sign(M[2]) * 8769
    coef[2] = 1173 * np.sign(np.outer(M[0], M[0])).reshape(64)
    coef[3] = 1173 * rng.choice([-1, 1], 64)
    quant = np.ones(64, np.int64)

    def reference(c, q):
        px, ok = jr.idct(c * q)
        return px.reshape(2, 2, 8, 8).transpose(0, 2, 1, 3).reshape(16, 16), ok
    want, ok = reference(coef, quant)
    assert ok.all()
    got, status = idct(coef, quant)
    np.testing.assert_array_equal(got, want)
    assert status == 0
    assert len(np.unique(want)) > 2                         # not everything saturated
    # one step beyond: flagged, and computed the same way (still equal where the 64-bit value still fits)
    coef[0, :8] = np.sign(M[2]) * 8770
    got, status = idct(coef, quant)
    assert status == jpeg.ST_IDCT_RANGE
    np.testing.assert_array_equal(got, reference(coef, quant)[0])
    # the same through the quantiser: 2923 * 3 = 8769 and 4385 * 2 = 8770
    c3, q3 = coef.copy(), quant.copy()
    c3[:, :8], q3[:8] = np.sign(coef[:, :8]) * 2923 * (np.abs(coef[:, :8]) > 0), 3
    c3[2:] = 0
    c3[1, :8] = -np.sign(M[2]) * 2923
    got, status = idct(c3, q3)
    np.testing.assert_array_equal(got, reference(c3, q3)[0])
    assert status == 0 and reference(c3, q3)[1].all()
    # far outside (the 64-bit value no longer fits): flagged, nothing else promised
    coef[0, :8] = np.sign(M[2]) * 30000
    assert idct(coef, quant)[1] == jpeg.ST_IDCT_RANGE
