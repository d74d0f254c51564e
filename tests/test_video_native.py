"""The compositor's kernel source on the CPU, under ASan + UBSan.

`poserisk_release_amd/csrc/compose.hip` is compiled unchanged for the host against `tests/native/host_shim.h` (a
workgroup = 256 threads and a barrier, workgroups one after the other) and run on exact-size heap buffers: its index
arithmetic, its u32 sums, the rounded division and every address it forms are checked against the numpy restatement of the
contract (tests/video_ref.py), byte for byte, without a GPU.  It is a permanent part of the CPU suite, like
tests/test_host_plan_native.py: the machines that run `-m "not gpu"` have no other way to execute the kernel's arithmetic, and
no GPU run checks addresses against exact-size buffers.  The price is that compose.hip keeps to what the shim defines
(threadIdx / blockIdx, __syncthreads, atomicOr, __uint2float_rn, uint4, one dynamic LDS block); a new intrinsic there needs a
line in the shim.  What this cannot show is anything about the GPU build itself -- tests/test_video_gpu.py does that."""
import numpy as np
import pytest

import host_build
import video_ref as vr
from poserisk_release_amd import video

BOX_RGB = (17, 250, 99)


@pytest.fixture(scope="module")
def compose_host(tmp_path_factory):
    d = tmp_path_factory.mktemp("compose_host")
    exe = host_build.build(d, "compose_host", "compose_host.cc", stage=("compose.hip",), shim=True, threads=True)

    def run(case, shift):
        a = case["atlas"]
        cov = np.asarray(a.cov)
        S, _, CH, CW = cov.shape
        N, L, C = case["lines"].shape[0], case["lines"].shape[1], case["text"].shape[2]
        n_frames, H, W, _ = case["frames"].shape
        h = np.zeros(24, np.int32)
        h[:12] = [N, n_frames, H, W, case["dst_h"], case["dst_w"], case["panel_w"], L, C, S, CH, CW]
        h[12:12 + S], h[16:16 + S], h[20:23], h[23] = a.adv, a.ascent, BOX_RGB, 1
        with open(d / "case.bin", "wb") as f:
            for arr in (h, case["frames"], case["src_idx"], case["box"], case["lines"], case["text"], cov):
                f.write(np.ascontiguousarray(arr).tobytes())
        exe.run(d / "case.bin", d / "out.bin", shift)
        shape = (N, case["dst_h"], case["dst_w"] + case["panel_w"], 3)
        raw = np.fromfile(d / "out.bin", np.uint8)
        n = int(np.prod(shape))
        return raw[:n].reshape(shape), raw[n:].view(np.int32)
    return run


def _case(H, W, N, atlas, seed, dst=None, L=16, C=12):
    rng = np.random.default_rng(seed)
    frames = rng.integers(0, 256, (3, H, W, 3), dtype=np.uint8)
    dst_h, dst_w, panel_w = dst or video.canvas_size(H, W)
    src_idx = rng.integers(0, 3, N).astype(np.int32)
    src_idx[N - 1] = 3 if N > 2 else src_idx[N - 1]              # no such frame
    box = np.array([[5, 4, W - 9, H - 7], [-6, H // 2, W + 3, H + 2], [W // 3, H // 3, W // 3 + 2, H // 3 + 1], [0, 0, -1, -1],
                    [W + 4, 2, W + 40, 9]], np.int32)[np.arange(N) % 5]
    S, _, CH, CW = atlas.cov.shape
    lines = np.zeros((N, L, 5), np.int32)
    lines[..., 0] = rng.integers(dst_w - 3 * CW, dst_w + panel_w + 4, (N, L))
    lines[..., 1] = rng.integers(-3, dst_h + CH + 3, (N, L))
    lines[..., 2] = rng.integers(-1, S + 1, (N, L))                # with classes that do not exist
    lines[..., 3] = rng.integers(-1, C + 4, (N, L))                # with empty lines and lengths beyond C
    lines[..., 4] = rng.integers(0, 1 << 24, (N, L))
    text = rng.integers(0, 256, (N, L, C), dtype=np.uint8)         # half the codes outside 32..127
    return dict(frames=frames, src_idx=src_idx, box=box, lines=lines, text=text, atlas=atlas, dst_h=dst_h, dst_w=dst_w,
                panel_w=panel_w)


def _noise_atlas():
    cov = np.random.default_rng(5).integers(0, 256, (3, 96, 11, 7), dtype=np.uint8)
    return video.Atlas(cov, (7, 5, 3), (9, 4, 0))


@pytest.mark.parametrize("H,W,N,dst,font,shift", [
    (37, 53, 4, None, "noise", 0),                 # upscale 13.6 x, 720 + 280 wide
    (37, 53, 3, (23, 31, 17), "noise", 5),         # downscale, rows of 144 bytes, out misaligned by 5
    (61, 130, 5, (20, 40, 11), "dejavu", 9),       # ratios above 3: four taps
    (90, 160, 3, None, "dejavu", 1),               # the flagship ratio 10 : 9 at a fifth of its size
    (45, 1366, 2, (24, 720, 280), "noise", 0),     # 4098 bytes a row: rows that are not 16-byte aligned, 2 rows a band
])
def test_kernel_source_on_the_host_matches_the_reference(compose_host, H, W, N, dst, font, shift):
    atlas = _noise_atlas() if font == "noise" else video.font_atlas()
    case = _case(H, W, N, atlas, seed=H + W + N, dst=dst)
    out, st = compose_host(case, shift)
    want, want_st = vr.compose(case["frames"], case["src_idx"], case["box"], case["lines"], case["text"], np.asarray(atlas.cov),
                               atlas.adv, atlas.ascent, case["dst_h"], case["dst_w"], case["panel_w"], BOX_RGB)
    np.testing.assert_array_equal(st, want_st)
    bad = np.argwhere(out != want)
    assert bad.size == 0, f"{len(bad)} bytes differ, first (canvas, row, col, channel) {bad[0].tolist()}"
    assert out[:, :, case["dst_w"]:].any() and out[0, :, :case["dst_w"]].any()
