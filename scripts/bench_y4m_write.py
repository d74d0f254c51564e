"""Measure the YUV4MPEG2 writer (poserisk_release_amd/y4m.py, csrc/yuv_enc.hip) on the canvases the Predictor writes: 1000x450
(800x500 frames at 720x450 beside the score panel, scripts/bench_video.py's scene), at 64 and at 256 canvases a call, on one GPU, all in
the same run:

  (a) kernel      pr_yuv_encode alone, per chroma layout, from device events, warmed up, windows of at least half a second,
                  three windows a layout in rotation; each with its share of its byte floor (the RGB read + the stream bytes
                  written, over the streaming rate DESIGN.md uses);
  (b) y4m         compose + convert (420mpeg2) + download into pinned host memory: wall clock around a synchronise;
  (c) rgb_host    for comparison: compose + download of the raw RGB canvases + a float32 numpy conversion to the same 4:2:0
                  planes on the host (what a writer without the kernel would do);
  (d) mjpeg       for comparison: the Motion-JPEG path's compose + jpeg.encode_frames (quality 90) + download of the files.

usage: python scripts/bench_y4m_write.py [--out profiles/y4m_write.json]"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from poserisk_release_amd import _lib, jpeg, y4m  # noqa: E402
import bench_video  # noqa: E402

HBM_BYTES_PER_S = 5.3e12   # achievable streaming rate used for the floors (as scripts/bench_frontend.py)
H, W = 500, 800          # 720x450 beside the 280-wide panel: 1000x450 canvases
CALLS = (64, 256)


def best_of(fn, n=5):
    times = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def window(call, min_s=0.5):
    """Mean milliseconds per call over a window of at least min_s of device time (events around the whole window)."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    n = max(1, int(np.ceil(min_s * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(n):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n, n


def host_420(rgb):
    """u8[h,w,3] -> (Y, U, V) u8, limited-range BT.601 in float32 with the [1 2 1] x [1 1] chroma taps: one frame on the host."""
    f = rgb.astype(np.float32)
    y = f @ np.array([0.299, 0.587, 0.114], np.float32)
    Y = np.rint(16.0 + y * (219.0 / 255.0)).astype(np.uint8)
    p = np.pad(f, ((0, 0), (1, 1), (0, 0)), mode="edge")
    rows = p[:, 0:-2:2] + 2.0 * p[:, 1:-1:2] + p[:, 2::2]
    m = (rows[0::2] + rows[1::2]) * 0.125
    ym = m @ np.array([0.299, 0.587, 0.114], np.float32)
    U = np.rint(128.0 + (m[..., 2] - ym) * (224.0 / 255.0 / 1.772)).astype(np.uint8)
    V = np.rint(128.0 + (m[..., 0] - ym) * (224.0 / 255.0 / 1.402)).astype(np.uint8)
    return Y, U, V


def measure(dev, n):
    compose, _, _ = bench_video.compose_call(n, H, W, dev)
    canvases = compose.keep[0]["out"]
    ch, cw = int(canvases.shape[1]), int(canvases.shape[2])
    assert (cw, ch) == (1000, 450)
    compose()
    torch.cuda.synchronize()
    src_bytes = ch * cw * 3
    kernel, outs = {}, {}
    for chroma in y4m.CHROMAS:
        outs[chroma] = torch.empty((n, y4m.encoded_size(cw, ch, chroma)[2]), dtype=torch.uint8, device=dev)
    calls = {c: (lambda c=c: y4m.encode_frames(canvases, c, out=outs[c])) for c in y4m.CHROMAS}
    for call in calls.values():
        for _ in range(3):
            call()
    rows = {c: [] for c in calls}
    for _ in range(3):                                         # windows in rotation
        for c, call in calls.items():
            ms, k = window(call)
            rows[c].append(dict(ms_per_call=round(ms, 4), calls_in_window=k))
    for c in calls:
        ms = min(r["ms_per_call"] for r in rows[c])
        written = int(outs[c].shape[1])
        floor_ms = n * (src_bytes + written) / HBM_BYTES_PER_S * 1e3
        kernel[c] = dict(windows=rows[c], ms_per_call=ms, us_per_frame=round(ms / n * 1e3, 3), frames_per_s=round(n / ms * 1e3, 1),
                         bytes_read_per_frame=src_bytes, bytes_written_per_frame=written, floor_ms=round(floor_ms, 4),
                         share_of_floor=round(floor_ms / ms, 4))
    record = dict(frames=n, canvas=f"{cw}x{ch}", kernel=kernel)
    # (b) compose + convert + download
    chroma = "420mpeg2"
    pinned = torch.empty(tuple(outs[chroma].shape), dtype=torch.uint8).pin_memory()

    def y4m_path():
        compose()
        y4m.encode_frames(canvases, chroma, out=outs[chroma])
        pinned.copy_(outs[chroma], non_blocking=True)
    y4m_path()
    t = best_of(y4m_path)
    record["y4m"] = dict(ms=[round(x * 1e3, 3) for x in t], frames_per_s=round(n / min(t), 1), host_bytes=int(pinned.numel()))
    # (c) compose + raw RGB download + the conversion on the host
    rgb_host = torch.empty(tuple(canvases.shape), dtype=torch.uint8).pin_memory()
    view = rgb_host.numpy()
    split = {}

    def rgb_path():
        compose()
        rgb_host.copy_(canvases, non_blocking=True)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for k in range(n):
            host_420(view[k])
        split["host_convert_ms"] = round((time.perf_counter() - t0) * 1e3, 1)
    t = best_of(rgb_path, n=2 if n <= 64 else 1)
    record["rgb_host"] = dict(ms=[round(x * 1e3, 1) for x in t], frames_per_s=round(n / min(t), 1), host_bytes=int(rgb_host.numel()),
                              **split)

    def rgb_download():
        compose()
        rgb_host.copy_(canvases, non_blocking=True)
    t = best_of(rgb_download)
    record["rgb_download_only"] = dict(ms=[round(x * 1e3, 3) for x in t], frames_per_s=round(n / min(t), 1))
    # the device result against the host's float conversion, for the record (not a test: the contract is the integer one)
    Y, U, V = host_420(view[0])
    got = pinned[0].numpy()
    record["max_abs_difference_to_the_float_host_conversion"] = int(max(
        np.abs(got[6:6 + ch * cw].astype(int) - Y.ravel()).max(),
        np.abs(got[6 + ch * cw:6 + ch * cw + U.size].astype(int) - U.ravel()).max(),
        np.abs(got[6 + ch * cw + U.size:].astype(int) - V.ravel()).max()))
    del rgb_host, view
    # (d) the Motion-JPEG path
    files = {}

    def mjpeg_path():
        compose()
        buf, nbytes, status = jpeg.encode_frames(canvases, quality=90)
        files["bytes"] = sum(len(b) for b in jpeg.download_files(buf, nbytes))
    mjpeg_path()
    t = best_of(mjpeg_path)
    record["mjpeg"] = dict(ms=[round(x * 1e3, 3) for x in t], frames_per_s=round(n / min(t), 1), host_bytes=files["bytes"],
                           note="quality 90, 4:2:0; lossy, and the files are a fraction of the planes' bytes")
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_y4m_write.py needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    record = dict(device=torch.cuda.get_device_name(0), library=_lib.load().pr_build_info().decode(),
                  video=f"{W}x{H} frames -> 1000x450 canvases, limited range, BT.601", floor_bytes_per_s=HBM_BYTES_PER_S, calls={})
    for n in CALLS:
        record["calls"][str(n)] = measure(dev, n)
        print(n, json.dumps(record["calls"][str(n)]), flush=True)
    print(json.dumps(record))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
