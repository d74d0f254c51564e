"""Measure the PNG encoder (pr_png_encode, csrc/png_enc.hip) on what the report path gives it: 1000x450 composed score canvases
(pr_compose_video on distinct smooth frames, as scripts/bench_jpeg_encode.py makes them) and 800x450 noisy RGB frames (a smooth
picture with three bits of noise a sample: a camera's frame as the mesh writer sees it), 64 and 256 frames a call.

  a  encode alone, per mode and filter: device events around pr_png_encode (frames on the device, outputs and workspace
     allocated once), warmed up, the median of the rounds;
  b  compose + encode + download of the used bytes (png.download_files), wall clock with a synchronisation at the end
     (canvases only: the noisy frames have no compose step, theirs is encode + download);
  c  today's path: download of the raw frames, then one PNG per frame through Pillow (poserisk_release_amd/sinks.py's save_png), wall clock;
  d  Pillow on 16 threads from host memory at compress_level 1 and at its default, wall clock;
  e  bytes per frame of each of the above and of pr_jpeg_encode at quality 90.
No threshold: the figures are reported as they are, the rows where the GPU loses to (d) included.

usage: python scripts/bench_png_encode.py [--out profiles/png_encode.json] [--batches 64,256] [--rounds 3]
(the committed profile's own command line is in its `command` field)"""
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

from poserisk_release_amd import _lib, jpeg, png  # noqa: E402
import bench_jpeg_encode as bj  # noqa: E402
import bench_video  # noqa: E402

VARIANTS = (("rle", "adaptive"), ("rle", "sub"), ("rle", "up"), ("rle", "paeth"), ("rle", "none"), ("stored", "none"))


def noisy_frames(B, dev):
    """B distinct 800 x 450 frames: bench_jpeg_encode's smooth picture cut to 450 rows, plus three bits of noise a sample."""
    base = bj.smooth_frames(B, dev)[:, :450].contiguous()
    gen = torch.Generator(device=dev).manual_seed(450)
    return (base + torch.randint(0, 8, base.shape, dtype=torch.uint8, device=dev, generator=gen)).contiguous()


def events(fn, iters, rounds):
    out = []
    for _ in range(rounds):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(iters):
            fn()
        e1.record()
        torch.cuda.synchronize()
        out.append(e0.elapsed_time(e1) / iters)
    return float(np.median(out)), out


def measure(kind, B, dev, rounds):
    if kind == "canvas":
        compose, frames, _ = bench_video.compose_call(B, bj.H, bj.W, dev)
        frames.copy_(bj.smooth_frames(B, dev))
        images = compose.keep[0]["out"]
        compose()
    else:
        compose, images = (lambda: None), noisy_frames(B, dev)
    torch.cuda.synchronize()
    Hh, Ww = int(images.shape[1]), int(images.shape[2])
    cap = png.encode_bound(Hh, Ww)
    out = (torch.empty((B, cap), dtype=torch.uint8, device=dev), torch.empty(B, dtype=torch.int32, device=dev),
           torch.empty(B, dtype=torch.int32, device=dev))
    ws = torch.empty(png.encode_workspace_bytes(B, Hh, Ww), dtype=torch.uint8, device=dev)
    rec = {"frames": f"{Ww}x{Hh} {kind}", "batch": B, "raw_bytes_per_frame": int(images[0].numel()), "a_encode": []}
    iters = max(2, 128 // B * 2)
    for mode, filt in VARIANTS:
        enc = lambda: png.encode_frames(images, filter=filt, mode=mode, out=out, workspace=ws)
        buf, nbytes, status = enc()
        torch.cuda.synchronize()
        assert not status.any()
        ms, all_ms = events(enc, iters, rounds)
        rec["a_encode"].append({"mode": mode, "filter": filt, "ms_per_call": round(ms, 3), "frames_per_s": round(B / ms * 1e3, 1),
                                "ms_per_round": [round(v, 3) for v in all_ms],
                                "bytes_per_frame": round(float(nbytes.float().mean()), 1)})
    enc = lambda: png.encode_frames(images, out=out, workspace=ws)

    def path_b():
        compose()
        b, n, _ = enc()
        return png.download_files(b, n)
    files = path_b()
    b_s, b_all = bj.wall(path_b, rounds)
    rec.update(b_path="compose + encode + download" if kind == "canvas" else "encode + download",
               b_ms_per_call=round(b_s * 1e3, 2), b_frames_per_s=round(B / b_s, 1), b_ms_per_round=[round(v * 1e3, 2) for v in b_all],
               b_bytes_per_frame=round(float(np.mean([len(f) for f in files])), 1))
    jbuf, jn, jst = jpeg.encode_frames(images, quality=90)
    rec["e_jpeg_q90_bytes_per_frame"] = round(float(jn.float().mean()), 1)
    try:
        from PIL import Image
    except ImportError:
        rec["c_today"] = rec["d_pillow_16_threads"] = "not measured (Pillow is not importable)"
        return rec
    host = images.cpu().numpy()
    assert all(np.array_equal(np.asarray(Image.open(io.BytesIO(f)).convert("RGB")), im) for f, im in zip(files[:4], host[:4]))
    from poserisk_release_amd.sinks import save_png as _save_png   # what write_gpu_video's Pillow sink calls per frame
    with tempfile.TemporaryDirectory() as tmp:
        def path_c():
            compose()
            for i, im in enumerate(images.cpu().numpy()):
                _save_png(os.path.join(tmp, '{0:09d}.png'.format(i)), im)
        c_s, c_all = bj.wall(path_c, 2)
        sizes = [os.path.getsize(os.path.join(tmp, n)) for n in os.listdir(tmp)]
    rec.update(c_today="raw download + one PNG per frame (Pillow, default level)", c_ms_per_call=round(c_s * 1e3, 1),
               c_frames_per_s=round(B / c_s, 1), c_ms_per_round=[round(v * 1e3, 1) for v in c_all],
               c_bytes_per_frame=round(float(np.mean(sizes)), 1), c_bytes_over_pcie_per_frame=int(images[0].numel()))
    rec["d_pillow_16_threads"] = []
    best_a = min(v["ms_per_call"] for v in rec["a_encode"] if v["mode"] == "rle" and v["filter"] == "adaptive")
    for level in (1, None):
        def one(im):
            o = io.BytesIO()
            Image.fromarray(im).save(o, "PNG", **({} if level is None else {"compress_level": level}))
            return o.tell()
        with ThreadPoolExecutor(16) as pool:
            sizes = list(pool.map(one, host))
            d_s, d_all = bj.wall(lambda: list(pool.map(one, host)), max(2, rounds // 2))
        rec["d_pillow_16_threads"].append({"compress_level": "default" if level is None else level, "ms_per_call": round(d_s * 1e3, 1),
                                           "frames_per_s": round(B / d_s, 1), "ms_per_round": [round(v * 1e3, 1) for v in d_all],
                                           "bytes_per_frame": round(float(np.mean(sizes)), 1),
                                           "gpu_rle_adaptive_is_slower": bool(best_a > d_s * 1e3)})
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "png_encode.json"))
    ap.add_argument("--batches", default="64,256")
    ap.add_argument("--rounds", type=int, default=3)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png_encode.py needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    rec = {"device": torch.cuda.get_device_name(0), "library": _lib.load().pr_build_info().decode(), "host_threads": 16,
           "command": "python scripts/bench_png_encode.py --batches %s --rounds %d" % (a.batches, a.rounds),
           "runs": [measure(kind, int(b), dev, a.rounds) for kind in ("canvas", "noisy") for b in a.batches.split(",")]}
    line = json.dumps(rec, indent=1)
    print(line)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        f.write(line + "\n")


if __name__ == "__main__":
    main()
