"""Measure the JPEG encoder (pr_jpeg_encode, csrc/jpeg_enc.hip) on composed score canvases: 1000x450, 4:2:0, quality 90, a
restart marker per MCU row, 64 and 256 canvases a call.  The canvases come from pr_compose_video on distinct noise-free frames
(a smooth picture, a track box, a nine-line panel), so that the encoder sees what write_gpu_video gives it.

  a  encode alone: device events around pr_jpeg_encode (canvases already on the device, outputs and workspace allocated once),
     warmed up, the median of the rounds;
  b  compose + encode + download of the used bytes (jpeg.download_files), wall clock with a synchronisation at the end;
  c  what the parent path does with the same canvases: download of the raw canvases, then one PNG per frame through Pillow
     (or cv2.VideoWriter where cv2 is importable), wall clock;
  d  Pillow (libjpeg-turbo) encoding the same pixels to the same bytes on 16 threads from host memory, wall clock.
Also the bytes that cross PCIe per frame on each path.  No threshold: the figures are reported as they are.

usage: python scripts/bench_jpeg_encode.py [--out profiles/jpeg_encode.json] [--batches 64,256] [--rounds 5]"""
import argparse
import io
import json
import os
import sys
import tempfile
import time
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from poserisk_release_amd import _lib, jpeg  # noqa: E402
import bench_video  # noqa: E402

H, W = 500, 800            # the video's frames: at 720 px wide beside the 280 px panel the canvases are 450 x 1000
QUALITY = 90


def smooth_frames(B, dev):
    """B distinct frames with picture-like content (gradients, a disc, mild texture) instead of bench_video.py's noise."""
    y, x = np.mgrid[0:H, 0:W].astype(np.int64)
    out = np.empty((B, H, W, 3), np.uint8)
    for i in range(B):
        h = ((x * 73856093) ^ (y * 19349663) ^ (i * 83492791)) >> 5
        img = np.stack([(x * 255 // (W - 1) + 3 * i + (h & 7)) & 255, (y * 255 // (H - 1) + ((h >> 3) & 7)) & 255,
                        ((x + 2 * y + 5 * i) * 255 // (W + 2 * H) + ((h >> 6) & 7)) & 255], -1)
        disc = (x - 300 - 2 * i) ** 2 + (y - 225) ** 2 < 110 ** 2
        img[disc] = img[disc] // 3 + 20
        out[i] = img
    return torch.from_numpy(out).to(dev)


def wall(fn, rounds):
    times = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return float(np.median(times)), times


def measure(B, dev, rounds):
    compose, frames, _ = bench_video.compose_call(B, H, W, dev)
    frames.copy_(smooth_frames(B, dev))
    canvases = compose.keep[0]["out"]
    assert tuple(canvases.shape[1:]) == (450, 1000, 3), tuple(canvases.shape)
    compose()
    torch.cuda.synchronize()
    # the outputs and the workspace are allocated once, so that (a) times pr_jpeg_encode's memset and kernels and nothing else
    first = jpeg.encode_frames(canvases, quality=QUALITY)
    ws = torch.empty(jpeg.encode_workspace_bytes(B, *canvases.shape[1:3]), dtype=torch.uint8, device=dev)
    enc = lambda: jpeg.encode_frames(canvases, quality=QUALITY, out=first, workspace=ws)
    buf, nbytes, status = enc()
    torch.cuda.synchronize()
    assert not status.any()
    files = jpeg.download_files(buf, nbytes)
    jpeg_bytes = float(np.mean([len(f) for f in files]))
    # a: encode alone, device events
    iters = max(4, 256 // B * 4)
    a_rounds = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            enc()
        e1.record()
        torch.cuda.synchronize()
        a_rounds.append(e0.elapsed_time(e1) / iters)
    a_ms = float(np.median(a_rounds))
    # the clear in front of the kernels: pr_jpeg_encode zeroes the whole unstuffed buffer, F * U chunks of 64 bytes with
    # U = capacity / 64 + segments + 1 (csrc/jpeg_enc.hip, enc_geometry), whatever the frames then fill of it
    cleared = B * (buf.shape[1] // 64 + (canvases.shape[1] + 15) // 16 + 1) * 64
    ws[:cleared].zero_()                                          # loads the fill kernel
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        ws[:cleared].zero_()
    e1.record()
    torch.cuda.synchronize()
    clear_ms = e0.elapsed_time(e1) / iters

    def path_b():
        compose()
        b, n, _ = enc()
        return jpeg.download_files(b, n)
    b_s, b_all = wall(path_b, rounds)

    try:
        import cv2
    except ImportError:
        cv2 = None
    try:
        from PIL import Image
    except ImportError:
        Image = None
    rec = {"batch": B, "jpeg_bytes_per_frame": round(jpeg_bytes, 1), "raw_bytes_per_frame": int(canvases[0].numel()),
           "a_encode_ms_per_call": round(a_ms, 3), "a_encode_frames_per_s": round(B / a_ms * 1e3, 1),
           "a_ms_per_round": [round(v, 3) for v in a_rounds],
           "a_cleared_bytes_per_call": int(cleared), "a_clear_alone_ms_per_call": round(clear_ms, 4),
           "b_compose_encode_download_ms_per_call": round(b_s * 1e3, 2), "b_frames_per_s": round(B / b_s, 1),
           "b_ms_per_round": [round(v * 1e3, 2) for v in b_all]}
    with tempfile.TemporaryDirectory() as tmp:
        def path_c():
            compose()
            host = canvases.cpu().numpy()
            if cv2 is not None:
                vw = cv2.VideoWriter(os.path.join(tmp, "v.mp4"), 0x7634706d, 30.0, (host.shape[2], host.shape[1]))
                for im in host:
                    vw.write(np.ascontiguousarray(im[..., ::-1]))
                vw.release()
            else:
                for i, im in enumerate(host):
                    Image.fromarray(im).save(os.path.join(tmp, '{0:09d}.png'.format(i)))
        if cv2 is not None or Image is not None:
            c_s, c_all = wall(path_c, max(2, rounds // 2))
            rec.update(c_parent_path="cv2.VideoWriter mp4v" if cv2 is not None else "raw download + one PNG per frame (Pillow)",
                       c_parent_ms_per_call=round(c_s * 1e3, 1), c_frames_per_s=round(B / c_s, 1),
                       c_ms_per_round=[round(v * 1e3, 1) for v in c_all])
        else:
            rec["c_parent_path"] = "not measured (neither cv2 nor Pillow is importable)"
    if Image is not None:
        host = canvases.cpu().numpy()

        def one(im):
            out = io.BytesIO()
            Image.fromarray(im).save(out, "JPEG", quality=QUALITY, subsampling=2, optimize=False, restart_marker_rows=1)
            return out.getvalue()
        with ThreadPoolExecutor(16) as pool:
            same = list(pool.map(one, host)) == files
            d_s, d_all = wall(lambda: list(pool.map(one, host)), rounds)
        rec.update(d_pillow_16_threads_ms_per_call=round(d_s * 1e3, 2), d_frames_per_s=round(B / d_s, 1),
                   d_ms_per_round=[round(v * 1e3, 2) for v in d_all], d_bytes_equal_the_gpu_files=bool(same),
                   a_slower_than_d=bool(a_ms > d_s * 1e3))
    else:
        rec["d_pillow_16_threads_ms_per_call"] = "not measured (Pillow is not importable)"
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_encode.json"))
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--rounds", type=int, default=5)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_jpeg_encode.py needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "library": _lib.load().pr_build_info().decode(),
           "canvas": "1000x450 4:2:0 quality 90, a restart marker per MCU row", "host_threads": 16,
           "runs": [measure(int(b), dev, a.rounds) for b in a.batches.split(",")]}
    line = json.dumps(rec, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
