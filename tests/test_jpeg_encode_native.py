"""The JPEG encoder's two halves on the CPU, under ASan + UBSan.

`csrc/jpeg_host.cc` (pr_jpeg_encode_plan, pr_jpeg_encode_bound) and `csrc/jpeg_enc.hip` (the kernels, compiled unchanged for the
host against tests/native/host_shim.h: a launch = nested loops over workgroups and threads) are built by g++
into one stand-alone driver, tests/native/jpeg_enc_native.cc, which runs every call in exact-size heap blocks.  Checked here,
without a GPU: every golden case byte for byte against Pillow's file, the reciprocal quantiser against the division over its whole
range, the 32-bit FDCT at the extremes of 8-bit input against an int64 evaluation, and the capacity rule at its edges."""
import numpy as np
import pytest

import host_build
import jpeg_enc_cases as ec
import jpeg_enc_ref as er

PLAN_BYTES = 32 + 256 + 512 + 64 + 1024 + 32 + 512 + 640


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_enc_native")
    exe = host_build.build(d, "jpeg_enc_native", "jpeg_enc_native.cc", stage=("jpeg_enc.hip", "jpeg_host.cc"), shim=True)

    def run(*args):
        return exe.run(*args).stdout

    def encode(frames, quality, subsampling, restart_interval, bgr=0, capacities=(-1,)):
        """-> ([(capacity, nbytes int32[F], status int32[F], out u8[F, capacity])], plan bytes, bound)"""
        frames = np.ascontiguousarray(frames, np.uint8)
        F, H, W, _ = frames.shape
        hs, vs = er.SAMPLING[subsampling]
        with open(d / "enc.bin", "wb") as f:
            f.write(np.array([F, H, W, hs, vs, restart_interval, quality, bgr, len(capacities)], np.int32).tobytes())
            f.write(np.array(capacities, np.int64).tobytes() + frames.tobytes())
        run("encode", d / "enc.bin", d / "enc_out.bin")
        take, out = host_build.taker(d / "enc_out.bin"), []
        for _ in capacities:
            cap = int(take(np.int64, 1)[0])
            out.append((cap, take(np.int32, F).copy(), take(np.int32, F).copy(), take(np.uint8, F * cap).reshape(F, cap)))
        plan, bound = take(np.uint8, PLAN_BYTES), int(take(np.int64, 1)[0])
        take.done()
        return out, plan, bound

    def fdct(samples):
        samples = np.ascontiguousarray(samples, np.int32).reshape(-1, 64)
        with open(d / "fdct.bin", "wb") as f:
            f.write(np.int32(len(samples)).tobytes() + samples.tobytes())
        run("fdct", d / "fdct.bin", d / "fdct_out.bin")
        return np.fromfile(d / "fdct_out.bin", np.int32).reshape(-1, 8, 8)
    return run, encode, fdct


def test_every_golden_case_is_byte_exact(native):
    _, encode, _ = native
    cases = ec.small_cases() + [ec.canvas_case()]
    assert len(cases) >= 50
    for c in cases:
        for bgr in ((0, 1) if c["src"].shape[0] < 100 else (0,)):
            src = c["src"][..., ::-1] if bgr else c["src"]
            (( _, nbytes, status, out),), _, bound = encode(src[None], c["quality"], c["subsampling"], c["restart_interval"], bgr)
            want = np.frombuffer(c["data"], np.uint8)
            assert status[0] == 0 and nbytes[0] == len(want) <= bound, (c["name"], bgr, status, nbytes, len(want))
            bad = np.nonzero(out[0, :len(want)] != want)[0]
            assert bad.size == 0, f"{c['name']} bgr={bgr}: {bad.size} bytes differ, the first at {bad[0]}"
            assert (out[0, len(want):] == 0xAB).all(), f"{c['name']}: bytes written behind the file"


def test_frames_of_one_call_keep_to_their_slots(native):
    """Three frames in one call (the middle one noise at quality 100), each slot exactly as large as the largest file."""
    _, encode, _ = native
    rng = np.random.default_rng(5)
    smooth = next(c for c in ec.small_cases() if c["name"].startswith("37x29_smooth"))["src"]
    frames = np.stack([smooth, rng.integers(0, 256, smooth.shape, dtype=np.uint8), smooth[::-1].copy()])
    want = [er.encode(f, 100, "4:2:0", 2) for f in frames]
    ((cap, nbytes, status, out),), _, _ = encode(frames, 100, "4:2:0", 2, capacities=(max(len(w) for w in want),))
    for i, w in enumerate(want):
        assert status[i] == 0 and nbytes[i] == len(w)
        assert out[i, :len(w)].tobytes() == w and (out[i, len(w):] == 0xAB).all()


def test_the_quantiser_equals_the_division_over_its_whole_range(native):
    run, _, _ = native
    assert f"{2 * 16385 * 2033} quotients equal the division" in run("quant")
    assert 16384 >= 8192 + 1                       # the largest coefficient the FDCT gives (header, section j2)


def test_the_32_bit_fdct_equals_the_64_bit_reference_on_extreme_blocks(native):
    _, _, fdct = native
    yy, xx = np.mgrid[0:8, 0:8]
    blocks = [np.zeros((8, 8)), np.full((8, 8), 255), 255 * ((yy + xx) & 1), 255 * ((yy + xx + 1) & 1), 255 * (xx & 1), 255 * (yy & 1),
              255 * ((xx + 1) & 1), 255 * ((yy + 1) & 1)]
    for i in range(64):
        for lo, hi in ((0, 255), (255, 0)):
            b = np.full(64, lo)
            b[i] = hi
            blocks.append(b.reshape(8, 8))
    # the sign patterns that drive each output of a pass to its largest value, in both passes
    unit = er._pass(np.eye(8, dtype=np.int64) * (1 << 20), True)
    for k in range(8):
        for l in range(8):
            blocks.append(255 * (np.outer(unit[:, k] > 0, unit[:, l] > 0) | np.outer(unit[:, k] <= 0, unit[:, l] <= 0)))
    blocks = np.array(blocks, np.int64)
    want, pass1 = er.fdct(blocks, with_pass1=True)
    assert er.FDCT_ROW_SUM * er.FDCT_BOUND + (1 << 14) < 2 ** 31 <= er.FDCT_ROW_SUM * (er.FDCT_BOUND + 1) + (1 << 14)
    assert np.abs(np.round(unit * 2.0 ** 11 / 2 ** 20)).sum(0)[[1, 2, 3, 5, 6, 7]].max() == er.FDCT_ROW_SUM    # the DESCALEd rows
    assert np.abs(blocks - 128).max() <= er.FDCT_BOUND and np.abs(pass1).max() <= 4096 <= er.FDCT_BOUND
    assert np.abs(want).max() <= 8192
    np.testing.assert_array_equal(fdct(blocks), want)
    assert np.abs(want).max() >= 7000              # the blocks do reach the far end of the range


def test_capacity_edges_set_overflow_and_leave_the_slot_alone(native):
    _, encode, _ = native
    src = np.random.default_rng(17).integers(0, 256, (17, 33, 3), dtype=np.uint8)
    for subsampling, ri in (("4:2:0", 3), ("4:2:2", -1), ("4:4:4", 0)):
        want = np.frombuffer(er.encode(src, 100, subsampling, ri), np.uint8)
        head = len(er.header(17, 33, 100, *er.SAMPLING[subsampling], ri))
        caps = (0, head, len(want) - 1, len(want), len(want) + 1)
        runs, _, _ = encode(src[None], 100, subsampling, ri, capacities=caps)
        for (cap, nbytes, status, out), asked in zip(runs, caps):
            assert cap == asked
            if cap < len(want):
                assert status[0] == er.ST_OVERFLOW and nbytes[0] == 0 and (out == 0xAB).all(), (subsampling, cap)
            else:
                assert status[0] == 0 and nbytes[0] == len(want), (subsampling, cap)
                assert (out[0, :len(want)] == want).all() and (out[0, len(want):] == 0xAB).all(), (subsampling, cap)


def test_one_overflowing_frame_of_a_call_leaves_its_neighbours_exact(native):
    """Smooth, noise, smooth in one call with a slot one byte short of the noise frame's file: that frame alone reports overflow
    and its slot is untouched; the frames on both sides are byte-exact."""
    _, encode, _ = native
    rng = np.random.default_rng(6)
    smooth = next(c for c in ec.small_cases() if c["name"].startswith("37x29_smooth"))["src"]
    frames = np.stack([smooth, rng.integers(0, 256, smooth.shape, dtype=np.uint8), smooth[:, ::-1].copy()])
    want = [er.encode(f, 100, "4:2:0", -1) for f in frames]
    assert len(want[1]) - 1 > max(len(want[0]), len(want[2]))
    ((cap, nbytes, status, out),), _, _ = encode(frames, 100, "4:2:0", -1, capacities=(len(want[1]) - 1,))
    assert status.tolist() == [0, er.ST_OVERFLOW, 0] and nbytes.tolist() == [len(want[0]), 0, len(want[2])]
    assert (out[1] == 0xAB).all()
    for i in (0, 2):
        assert out[i, :len(want[i])].tobytes() == want[i] and (out[i, len(want[i]):] == 0xAB).all()
