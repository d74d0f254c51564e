"""One call each of the fused YUV4MPEG2 kernel and of the two-step path (convert at the source size, then pr_resize_frames) on N
frames of 1920x1080 420mpeg2 -> 800x450, for a counter or kernel-trace run of its own:

    rocprofv3 --pmc SQ_INSTS_VMEM_RD SQ_INSTS_VMEM_WR SQ_INSTS_VALU SQ_WAVES -d out -o pmc --output-format csv -- \\
        python scripts/exp_y4m_kernels.py 64

The planes are random bytes (no timing or count here depends on content); the payloads sit behind "FRAME\\n", six bytes, so frame
k starts at byte alignment (2 k) % 4 of the chunk, as in a real stream."""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from poserisk_release_amd import frontend, y4m  # noqa: E402

H, W, CHROMA = 1080, 1920, "420mpeg2"


def main():
    n = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    dev = torch.device("cuda", 0)
    w, h = frontend.target_size(W, H)
    fb = W * H + 2 * (W // 2) * (H // 2)
    rng = np.random.default_rng(0)
    chunk = np.empty(n * (fb + 6), np.uint8)
    offsets = np.arange(n, dtype=np.int64) * (fb + 6) + 6
    for k in range(n):
        chunk[k * (fb + 6):k * (fb + 6) + 6] = np.frombuffer(b"FRAME\n", np.uint8)
        chunk[offsets[k]:offsets[k] + fb] = rng.integers(0, 256, fb, dtype=np.uint8)
    data, offs = torch.from_numpy(chunk).to(dev), torch.from_numpy(offsets).to(dev)
    plan = y4m.yuv_plan("601", False)
    rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    out2 = torch.empty_like(out)
    for _ in range(2):
        y4m.yuv_frames(data, offs, H, W, CHROMA, plan, size=(h, w), out=out)
        y4m.yuv_frames(data, offs, H, W, CHROMA, plan, out=rgb)
        frontend.resize_frames(rgb, h, w, out=out2)
    torch.cuda.synchronize()
    assert torch.equal(out, out2)
    print(f"{n} frames: fused and two-step agree")


if __name__ == "__main__":
    main()
