"""Measure the video front end (poserisk_release_amd/frontend.py) on a Motion-JPEG AVI of 256 frames of 1920x1080, 4:2:0, quality
95, once without restart markers (what ffmpeg and cameras write) and once with a marker per MCU row (what this package writes):

  demux       mjpeg.AviReader on the file (host, wall clock; page cache);
  decode      jpeg.decode_files on the demuxed frames at the source size (wall clock around a synchronise);
  resize      pr_resize_frames 1080p -> 800x450 on 256 frames from device events, warmed up, windows of at least a second, against
              its byte floor: the source bytes its taps touch plus the bytes it writes, over the streaming rate DESIGN.md uses;
  end_to_end  frontend.read_video file -> downscaled frames on the device, frames/s (wall clock around a synchronise);
  pillow      for comparison on the same host: Pillow decode + Image.resize (bilinear) on 16 threads.

The timed frames are DISTINCT different frames in rotation.  usage: python scripts/bench_frontend.py [--out profiles/frontend_avi.json]"""
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

from poserisk_release_amd import _lib, frontend, jpeg, mjpeg  # noqa: E402

HBM_BYTES_PER_S = 5.3e12   # achievable streaming rate used for the floors (as scripts/bench_jpeg.py)
H, W, N_FRAMES, DISTINCT = 1080, 1920, 256, 16


def streams():
    """{variant: [DISTINCT streams]}: the golden 800x450 frame enlarged to 1920x1080 and rolled by a different offset each."""
    from PIL import Image
    z = np.load(os.path.join(REPO, "tests", "golden", "jpeg_frames.npz"))
    off, s, names = z["offsets"], z["streams"], [str(n) for n in z["names"]]
    i = names.index("444_q95")
    frame = np.asarray(Image.open(io.BytesIO(s[off[i]:off[i + 1]].tobytes())).convert("RGB").resize((W, H), Image.BICUBIC))
    out = {}
    for variant, kw in (("no_restart", {}), ("restart_per_mcu_row", dict(restart_marker_rows=1))):
        out[variant] = []
        for k in range(DISTINCT):
            buf = io.BytesIO()
            Image.fromarray(np.roll(frame, (37 * k, 53 * k), axis=(0, 1))).save(buf, "JPEG", quality=95, subsampling=2, **kw)
            out[variant].append(buf.getvalue())
    return out


def best_of(fn, n=3):
    times = []
    for _ in range(n):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t0)
    return times


def timed_window(call, min_s=1.0):
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


def resize_floor_bytes(h, w):
    """Bytes one frame's resize touches: every source byte some tap reads (rows x columns the tables name, 3 channels) + h w 3."""
    xofs, _, yofs, _, _ = frontend.resize_plan(H, W, h, w)
    cols = np.union1d(xofs, np.minimum(xofs + 1, W - 1)).size
    rows = np.union1d(yofs, np.minimum(yofs + 1, H - 1)).size
    return rows * cols * 3, h * w * 3


def measure_resize(dev, h, w):
    src = torch.empty((N_FRAMES, H, W, 3), dtype=torch.uint8, device=dev).random_(0, 256)
    out = torch.empty((N_FRAMES, h, w, 3), dtype=torch.uint8, device=dev)
    call = lambda: frontend.resize_frames(src, h, w, out=out)
    call()
    call()
    torch.cuda.synchronize()
    rows = []
    for _ in range(2):
        ms, n = timed_window(call)
        rows.append(dict(ms_per_call=round(ms, 4), calls_in_window=n))
    read, written = resize_floor_bytes(h, w)
    floor_ms = N_FRAMES * (read + written) / HBM_BYTES_PER_S * 1e3
    ms = min(r["ms_per_call"] for r in rows)
    return dict(frames=N_FRAMES, windows=rows, us_per_frame=round(ms / N_FRAMES * 1e3, 3), source_bytes_touched_per_frame=read,
                source_share_touched=round(read / (H * W * 3), 4), bytes_written_per_frame=written, floor_ms=round(floor_ms, 4),
                share_of_floor=round(floor_ms / ms, 4), bound="HBM bytes: the source bytes the taps touch + the bytes written, at 5.3 TB/s")


def measure_pillow(blobs, h, w):
    from concurrent.futures import ThreadPoolExecutor
    from PIL import Image
    one = lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB").resize((w, h), Image.BILINEAR))
    res = []
    with ThreadPoolExecutor(16) as ex:
        for _ in range(2):
            t0 = time.perf_counter()
            np.stack(list(ex.map(one, blobs)))
            res.append(time.perf_counter() - t0)
    return dict(frames=len(blobs), threads=16, seconds=[round(t, 4) for t in res], frames_per_s=round(len(blobs) / min(res), 1),
                note="decode + Image.resize (bilinear); the upload of the result is not included")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda", 0)
    w, h = frontend.target_size(W, H)
    record = dict(device=torch.cuda.get_device_name(0), library=_lib.load().pr_build_info().decode(),
                  video=f"{N_FRAMES} frames of {W}x{H}, 4:2:0, quality 95 -> {w}x{h}", resize=measure_resize(dev, h, w), variants={})
    print("resize", record["resize"], flush=True)
    with tempfile.TemporaryDirectory() as d:
        for variant, distinct in streams().items():
            blobs = [distinct[i % DISTINCT] for i in range(N_FRAMES)]
            path = os.path.join(d, variant + ".avi")
            with mjpeg.AviWriter(path, W, H, 30.0) as wr:
                for b in blobs:
                    wr.write(b)
            demux = []
            for _ in range(3):
                t0 = time.perf_counter()
                got = mjpeg.AviReader(path).frames()
                demux.append(time.perf_counter() - t0)
            assert got == blobs
            chunk = min(frontend.chunk_frames(H, W, 16 << 30), N_FRAMES)
            r = dict(file_bytes=os.path.getsize(path), compressed_bytes_per_frame=sum(map(len, distinct)) // DISTINCT, chunk=chunk,
                     demux_ms=[round(t * 1e3, 2) for t in demux])
            for entropy in ("serial", "sync"):                   # the two entropy stages side by side, the same frames
                buf = torch.empty((N_FRAMES, H, W, 3), dtype=torch.uint8, device=dev)
                _, _, stats = jpeg.decode_files(got, dev, chunk=chunk, out=buf, entropy=entropy, stats=True)
                decode = best_of(lambda: jpeg.decode_files(got, dev, chunk=chunk, out=buf, entropy=entropy))
                del buf
                torch.cuda.empty_cache()
                frontend.read_video(path, dev, entropy=entropy)
                e2e = best_of(lambda: frontend.read_video(path, dev, entropy=entropy))
                r[entropy] = dict(decode_ms=[round(t * 1e3, 2) for t in decode], decode_frames_per_s=round(N_FRAMES / min(decode), 1),
                                  end_to_end_ms=[round(t * 1e3, 2) for t in e2e], end_to_end_frames_per_s=round(N_FRAMES / min(e2e), 1))
                if entropy == "sync":
                    st = stats[:DISTINCT].cpu().numpy()
                    r[entropy].update(rounds=sorted(int(v) for v in st[:, 1]), fell_back=int(st[:, 2].sum()))
            if variant == "no_restart":
                r["pillow_16_threads"] = measure_pillow(blobs, h, w)
            record["variants"][variant] = r
            print(variant, r, flush=True)
    print(json.dumps(record))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
