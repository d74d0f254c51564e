"""The people compositor's kernel source and its argument validation on the CPU, under ASan +
UBSan.

`poserisk_release_amd/csrc/compose.hip` (the one kernel behind both entry points) is compiled unchanged for the host against `tests/native/host_shim.h`
(as tests/test_video_native.py has it: a workgroup = 256 threads and a barrier, workgroups one after the other) into a stand-alone
program, `tests/native/compose_people_host.cc`, and run on exact-size heap buffers: the box table, the two line groups, the
u32 sums and every address the kernel forms are checked against the numpy restatement of the contract
(tests/video_people_ref.py), byte for byte, without a GPU -- and `--validate` gives pr_compose_people every argument error in
turn.  Nothing here is loaded into Python.  What this cannot show is anything about the GPU build itself --
tests/test_people_gpu.py does that."""
import numpy as np
import pytest

import host_build
import people_cases as pc


@pytest.fixture(scope="module")
def people_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("compose_people_host")
    exe = host_build.build(d, "compose_people_host", "compose_people_host.cc", stage=("compose.hip",), shim=True, threads=True)

    def run(c, shift=0, with_box=True):
        a = c["atlas"]
        cov = np.asarray(a.cov)
        S, _, CH, CW = cov.shape
        (N, K, _), L, C = c["box"].shape, c["lines"].shape[1], c["text"].shape[2]
        n_frames, H, W, _ = c["frames"].shape
        h = np.zeros(24, np.int32)
        h[:14] = [N, n_frames, H, W, c["dst_h"], c["dst_w"], c["panel_w"], K, L, c["L_img"], C, S, CH, CW]
        h[14:14 + S], h[18:18 + S], h[22], h[23] = a.adv, a.ascent, 1, int(with_box)
        with open(d / "case.bin", "wb") as f:
            for arr in (h, c["frames"], c["src_idx"], c["box"], c["box_rgb"], c["lines"], c["text"], cov):
                f.write(np.ascontiguousarray(arr).tobytes())
        exe.run(d / "case.bin", d / "out.bin", shift)
        shape = (N, c["dst_h"], c["dst_w"] + c["panel_w"], 3)
        raw = np.fromfile(d / "out.bin", np.uint8)
        n = int(np.prod(shape))
        return raw[:n].reshape(shape), raw[n:].view(np.int32)
    run.exe = exe
    return run


def test_every_argument_error_is_refused_before_any_work(people_host):
    assert "0 failures" in people_host.exe.run("--validate").stdout


@pytest.mark.parametrize("shape", pc.SHAPES, ids=lambda s: "K%d_L%d_Limg%d" % s)
@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: "%dx%d_to_%dx%d_p%d" % s)
def test_kernel_source_on_the_host_matches_the_reference(people_host, size, shape):
    c = pc.case(size, shape, seed=sum(size) + sum(shape))
    out, st = people_host(c, shift=(size[0] + shape[0]) % 16)          # out misaligned by 0 .. 15 bytes
    want, want_st = pc.reference(c)
    np.testing.assert_array_equal(st, want_st)
    bad = np.argwhere(out != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first (canvas, row, col, channel) {bad[0].tolist()}"
    assert st.tolist() == [0, 0, 0, 1]
    if shape[2] == 0:                                                  # no frame and no tags: a black image region
        assert not out[3, :, :size[2]].any()
    assert out[:3, :, :size[2]].any() and (shape[2] == shape[1] or out[:, :, size[2]:].any())


def test_wide_rows_and_a_null_box_on_the_host(people_host):
    """4098 bytes a source row (rows that are not 16-byte aligned, 2 destination rows a band) at the product's canvas width, with
    K = 4; then the same call with a NULL box: no outline anywhere."""
    c = pc.case((1366, 45, 720, 24, 280), (4, 10, 4), seed=3, N=2)
    out, st = people_host(c, shift=9)
    want, want_st = pc.reference(c)
    np.testing.assert_array_equal(st, want_st)
    assert np.array_equal(out, want)
    out, _ = people_host(c, with_box=False)
    want, _ = pc.reference(dict(c, box=None))
    assert np.array_equal(out, want)
