"""Measure the YUV4MPEG2 front end (poserisk_release_amd/y4m.py, csrc/yuv.hip) on 1920x1080 420mpeg2 frames going to 800x450, at 64
and at 256 frames a call, on one GPU:

  (a) kernel      pr_yuv_frames with the downscale fused against pr_yuv_frames at the source size + pr_resize_frames, from device
                  events, warmed up, in alternating windows of at least a second of the same run; each with its share of its own
                  byte floor (the bytes the path must read and write, over the streaming rate DESIGN.md uses);
  (b) pinned      the chunk's stream bytes in pinned host memory -> frames on the device (upload + kernel; wall clock around a
                  synchronise), fused and two-step;
  (c) rgb_upload  for comparison: the same frames as raw RGB in pinned host memory -> device + pr_resize_frames;
  (d) mjpeg_avi   for context: frontend.read_video on a Motion-JPEG AVI of the same pixels (quality 95, 4:2:0);
  and decode_file: y4m.decode on the .y4m file itself (page cache), the whole path a user runs.

The source frames are DISTINCT different frames in rotation.  usage: python scripts/bench_y4m.py [--out profiles/y4m_frontend.json]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from poserisk_release_amd import _lib, frontend, jpeg, mjpeg, y4m  # noqa: E402

HBM_BYTES_PER_S = 5.3e12   # achievable streaming rate used for the floors (as scripts/bench_frontend.py)
H, W, DISTINCT, CHROMA = 1080, 1920, 16, "420mpeg2"
CALLS = (64, 256)


def planes():
    """DISTINCT frames' planes: the golden 800x450 frame enlarged to 1920x1080, rolled by a different offset each, as limited-range
    BT.601 Y, U, V with 2 x 2 mean chroma (content only: no timing here depends on how they were made)."""
    from PIL import Image
    z = np.load(os.path.join(REPO, "tests", "golden", "jpeg_frames.npz"))
    off, s, names = z["offsets"], z["streams"], [str(n) for n in z["names"]]
    i = names.index("444_q95")
    frame = np.asarray(Image.open(io.BytesIO(s[off[i]:off[i + 1]].tobytes())).convert("RGB").resize((W, H), Image.BICUBIC))
    Y, U, V = [], [], []
    for k in range(DISTINCT):
        rgb = np.roll(frame, (37 * k, 53 * k), axis=(0, 1)).astype(np.float64)
        r, g, b = rgb[..., 0], rgb[..., 1], rgb[..., 2]
        y = 0.299 * r + 0.587 * g + 0.114 * b
        mean = lambda p: p.reshape(H // 2, 2, W // 2, 2).mean((1, 3))
        Y.append(np.rint(16 + y * 219 / 255))
        U.append(np.rint(128 + mean(b - y) / 1.772 * 224 / 255))
        V.append(np.rint(128 + mean(r - y) / 1.402 * 224 / 255))
    return [np.clip(np.stack(p), 0, 255).astype(np.uint8) for p in (Y, U, V)]


def best_of(fn, n=5):
    times = []
    for _ in range(n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def window(call, min_s=1.0):
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


def measure(dev, n, Y, U, V, h, w, tmp):
    idx = [i % DISTINCT for i in range(n)]
    path = os.path.join(tmp, f"clip{n}.y4m")
    y4m.write(path, Y[idx], U[idx], V[idx], fps=(30, 1), chroma=CHROMA)
    reader = y4m.Reader(path)
    info = reader.info
    (pinned, offsets), = list(reader.chunks(n))
    reader.close()
    assert len(offsets) == n and pinned.is_pinned()
    host_offsets = torch.from_numpy(offsets).pin_memory()
    plan = y4m.yuv_plan("601", False)
    data, offs = pinned.to(dev), host_offsets.to(dev)
    rgb = torch.empty((n, H, W, 3), dtype=torch.uint8, device=dev)
    out = torch.empty((n, h, w, 3), dtype=torch.uint8, device=dev)
    out2 = torch.empty_like(out)

    def fused():
        y4m.yuv_frames(data, offs, H, W, CHROMA, plan, size=(h, w), out=out)

    def two_step():
        y4m.yuv_frames(data, offs, H, W, CHROMA, plan, out=rgb)
        frontend.resize_frames(rgb, h, w, out=out2)
    for _ in range(2):
        fused()
        two_step()
    torch.cuda.synchronize()
    assert torch.equal(out, out2), "the fused and the two-step path differ"
    rows = {"fused": [], "two_step": []}
    for _ in range(3):                                         # alternating windows of the same run
        for name, call in (("fused", fused), ("two_step", two_step)):
            ms, calls = window(call)
            rows[name].append(dict(ms_per_call=round(ms, 4), calls_in_window=calls))
    fb, src_rgb, dst_rgb = info.frame_bytes, H * W * 3, h * w * 3
    floors = {"fused": dict(read=fb, written=dst_rgb), "two_step": dict(read=fb + src_rgb, written=src_rgb + dst_rgb)}
    kernel = {}
    for name in rows:
        ms = min(r["ms_per_call"] for r in rows[name])
        floor_ms = n * (floors[name]["read"] + floors[name]["written"]) / HBM_BYTES_PER_S * 1e3
        kernel[name] = dict(windows=rows[name], ms_per_call=ms, us_per_frame=round(ms / n * 1e3, 3), frames_per_s=round(n / ms * 1e3, 1),
                            bytes_read_per_frame=floors[name]["read"], bytes_written_per_frame=floors[name]["written"],
                            floor_ms=round(floor_ms, 4), share_of_floor=round(floor_ms / ms, 4))
    kernel["fused_over_two_step"] = round(kernel["two_step"]["ms_per_call"] / kernel["fused"]["ms_per_call"], 3)
    kernel["bound"] = "HBM bytes: the stream bytes + (two-step: the source-size RGB written and read back +) the bytes written, at 5.3 TB/s"

    def from_pinned(convert):
        def run():
            data.copy_(pinned, non_blocking=True)
            offs.copy_(host_offsets, non_blocking=True)
            convert()
        return run
    record = dict(frames=n, stream_bytes=int(pinned.numel()), kernel=kernel, pinned={})
    for name, call in (("fused", fused), ("two_step", two_step)):
        t = best_of(from_pinned(call))
        record["pinned"][name] = dict(ms=[round(x * 1e3, 3) for x in t], frames_per_s=round(n / min(t), 1),
                                      host_bytes_per_s=round(pinned.numel() / min(t) / 1e9, 2))
    # (c) the same frames as raw RGB: upload + resize
    rgb_host = torch.empty((n, H, W, 3), dtype=torch.uint8).pin_memory()
    rgb_host.copy_(rgb.cpu())

    def upload_rgb():
        rgb.copy_(rgb_host, non_blocking=True)
        frontend.resize_frames(rgb, h, w, out=out2)
    t = best_of(upload_rgb)
    record["rgb_upload"] = dict(ms=[round(x * 1e3, 3) for x in t], frames_per_s=round(n / min(t), 1), host_bytes=int(rgb_host.numel()))
    del rgb_host
    # the whole path on the file
    y4m.decode(path, dev, size=(h, w))
    for name, flag in (("fused", True), ("two_step", False)):
        t = best_of(lambda: y4m.decode(path, dev, size=(h, w), fused=flag), n=3)
        record.setdefault("decode_file", {})[name] = dict(ms=[round(x * 1e3, 2) for x in t], frames_per_s=round(n / min(t), 1))
    # (d) a Motion-JPEG AVI of the same pixels
    y4m.yuv_frames(data, offs, H, W, CHROMA, plan, out=rgb)
    avi = os.path.join(tmp, f"clip{n}.avi")
    with mjpeg.AviWriter(avi, W, H, 30.0) as wr:
        for lo in range(0, n, 32):
            buf, nbytes, status = jpeg.encode_frames(rgb[lo:lo + 32], quality=95, subsampling="4:2:0", restart_rows=1)
            assert not bool(status.any())
            for blob in jpeg.download_files(buf, nbytes):
                wr.write(blob)
    frontend.read_video(avi, dev)
    t = best_of(lambda: frontend.read_video(avi, dev), n=3)
    record["mjpeg_avi"] = dict(file_bytes=os.path.getsize(avi), ms=[round(x * 1e3, 2) for x in t], frames_per_s=round(n / min(t), 1),
                               note="quality 95, 4:2:0, a restart marker per MCU row; lossy: other pixels than the stream's")
    os.remove(avi)
    os.remove(path)
    return record


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    torch.cuda.set_device(dev)
    w, h = frontend.target_size(W, H)
    Y, U, V = planes()
    record = dict(device=torch.cuda.get_device_name(0), library=_lib.load().pr_build_info().decode(),
                  video=f"{W}x{H} {CHROMA}, limited range, BT.601 -> {w}x{h}", calls={})
    with tempfile.TemporaryDirectory() as tmp:
        for n in CALLS:
            record["calls"][str(n)] = measure(dev, n, Y, U, V, h, w, tmp)
            print(n, json.dumps(record["calls"][str(n)]), flush=True)
    faster = all(c["kernel"]["fused"]["ms_per_call"] < c["kernel"]["two_step"]["ms_per_call"] for c in record["calls"].values())
    record["fused_is_faster_at_both_call_sizes"] = faster
    print(json.dumps(record))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
