"""Measure the multi-scan JPEG decoder (pr_jpeg_decode_scans, csrc/jpeg_scans.hip) on progressive 800x450 4:2:0 quality-95 frames
against the single-scan decoders on the baseline encoding of the same pixels, in one run, every list run twice (A B A B):

  a  progressive          pr_jpeg_decode_scans on progressive frames without restart markers (libjpeg's ten-scan script)
  b  progressive_restart  pr_jpeg_decode_scans on progressive frames with a restart marker per MCU row
  c  baseline_serial      pr_jpeg_decode (one lane per restart segment) on the restart-free baseline frames: the yardstick of a
  d  baseline_sync        pr_jpeg_decode_sync on those
  e  pillow               Pillow on 16 threads decoding the progressive files of a (host only; "not measured" without Pillow)

at 64, 256 and 1024 frames a call: descriptors and bytes already on the device, two warm-up calls, device events around a
window of at least 20 calls and at least a second.  The frames are DISTINCT different frames in rotation (scripts/bench_jpeg.py,
`streams`), encoded both ways by Pillow; without Pillow only the golden frame is there (`distinct_streams` says which it was).

`--trace-run` decodes a dozen calls of 256 progressive frames and nothing else: run it under `rocprofv3 --kernel-trace --stats --
python scripts/bench_jpeg_progressive.py --trace-run`, then `--kernel-stats <kernel_stats.csv>` adds the per-kernel times.

usage: python scripts/bench_jpeg_progressive.py [--out profiles/jpeg_progressive.json] [--chunks 64,256,1024]
       python scripts/bench_jpeg_progressive.py --trace-run
       python scripts/bench_jpeg_progressive.py --kernel-stats <csv> [--out ...]      (no GPU needed)"""
import argparse
import csv
import io
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

import bench_jpeg as bj  # noqa: E402
from poserisk_release_amd import _lib, jpeg  # noqa: E402

H, W = bj.H, bj.W
MIN_CALLS, MIN_SECONDS = 20, 1.0


def streams():
    """{'progressive', 'progressive_restart', 'baseline'}: [stream, ...], the same pixels frame by frame."""
    z = np.load(os.path.join(REPO, "tests", "golden", "jpeg_progressive.npz"))
    off, s = z["frame_offsets"], z["frame_streams"]
    out = {"progressive": [s[off[0]:off[1]].tobytes()], "progressive_restart": [s[off[1]:off[2]].tobytes()],
           "baseline": [bj.streams()["no_restart"][0]]}
    try:
        from PIL import Image, ImageFile
    except ImportError:
        return out
    ImageFile.MAXBLOCK = 1 << 24
    frame = np.asarray(Image.open(io.BytesIO(out["baseline"][0])).convert("RGB"))
    for i in range(1, bj.DISTINCT):
        img = Image.fromarray(np.roll(frame, (37 * i, 53 * i), axis=(0, 1)))
        for name, kw in (("progressive", dict(progressive=True)), ("progressive_restart", dict(progressive=True, restart_marker_rows=1)),
                         ("baseline", {})):
            buf = io.BytesIO()
            img.save(buf, "JPEG", quality=95, subsampling=2, **kw)
            out[name].append(buf.getvalue())
    return out


def scans_call(blobs, chunk, dev):
    """-> (callable enqueuing one pr_jpeg_decode_scans of `chunk` frames, out tensor, status tensor)"""
    items = bj.repeated(blobs, chunk)
    blob = b"".join(items)
    frames, segs, huff, pst, h, w, offsets, scans, seg_scan, levels, multi = jpeg.parse_scans(items)
    assert not pst.any() and (h, w) == (H, W) and multi == chunk
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    t = dict(data=up(np.frombuffer(blob, np.uint8)), frames=up(frames), segs=up(segs), huff=up(huff), scans=up(scans), seg_scan=up(seg_scan),
             out=torch.empty((chunk, H, W, 3), dtype=torch.uint8, device=dev), status=torch.empty(chunk, dtype=torch.int32, device=dev),
             ws=torch.empty(jpeg.workspace_bytes(chunk, H, W), dtype=torch.uint8, device=dev))
    args = _lib.JpegScansArgs(_lib.JpegArgs(t["data"].data_ptr(), t["frames"].data_ptr(), t["segs"].data_ptr(), t["huff"].data_ptr(),
                                            t["out"].data_ptr(), t["status"].data_ptr(), len(blob), chunk, H, W, len(segs), len(huff), 0),
                              t["scans"].data_ptr(), t["seg_scan"].data_ptr(), len(scans), levels)
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    call = lambda: _lib.check(lib.pr_jpeg_decode_scans(args, t["ws"].data_ptr(), t["ws"].numel(), stream), "pr_jpeg_decode_scans")
    call.keep = (t, args)
    call.shape = dict(segments=len(segs), scans=len(scans), levels=levels, table_sets=len(huff))
    return call, t["out"], t["status"]


def timed_window(call):
    """Mean milliseconds per call from device events around a window of >= MIN_CALLS calls and >= MIN_SECONDS."""
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    call()
    b.record()
    b.synchronize()
    n = max(MIN_CALLS, int(np.ceil(MIN_SECONDS * 1e3 / max(a.elapsed_time(b), 1e-3))))
    a.record()
    for _ in range(n):
        call()
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / n, n


def pillow_rate(blobs, n=256, threads=16):
    try:
        from PIL import Image
    except ImportError:
        return "not measured"
    from concurrent.futures import ThreadPoolExecutor
    items = bj.repeated(blobs, n)
    decode = lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
    with ThreadPoolExecutor(threads) as ex:
        list(ex.map(decode, items[:threads]))
        t0 = time.perf_counter()
        list(ex.map(decode, items))
        dt = time.perf_counter() - t0
    return round(n / dt, 1)


def measure(dev, chunks):
    s = streams()
    ways = [("a", "progressive", "scans"), ("b", "progressive_restart", "scans"), ("c", "baseline", "serial"), ("d", "baseline", "sync")]
    rows = []
    for run in (1, 2):
        for chunk in chunks:
            reference = None
            for key, variant, entry in ways:
                call, out, status = scans_call(s[variant], chunk, dev) if entry == "scans" else bj.decode_call(s[variant], chunk, dev, entry)
                call()
                call()
                torch.cuda.synchronize()
                assert not status.any()
                if reference is None:
                    reference = out[:bj.DISTINCT].clone()
                if "restart" not in variant:                              # the same pixels whichever encoding and entry
                    assert torch.equal(out[:bj.DISTINCT], reference), (variant, chunk, entry)
                ms, n = timed_window(call)
                row = dict(run=run, key=key, stream=variant, entry=entry, chunk=chunk, ms_per_call=round(ms, 3), calls_in_window=n,
                           frames_per_s=round(chunk / ms * 1e3, 1), distinct_streams=len(s[variant]),
                           bytes_per_frame=int(np.mean([len(b) for b in s[variant]])))
                if entry == "scans":
                    row.update(call.shape)
                rows.append(row)
                print(json.dumps(row), flush=True)
                del call, out, status
                torch.cuda.empty_cache()
        rows.append(dict(run=run, key="e", stream="progressive", entry="pillow_16_threads", frames_per_s=pillow_rate(s["progressive"])))
        print(json.dumps(rows[-1]), flush=True)
    return rows


def summary(rows, chunks):
    out = {}
    for chunk in chunks:
        ms = lambda key: [r["ms_per_call"] for r in rows if r.get("chunk") == chunk and r["key"] == key]
        a, b, c, d = ms("a"), ms("b"), ms("c"), ms("d")
        ratios = [x / y for x, y in zip(a, c)]
        out[str(chunk)] = dict(a_over_c=[round(r, 3) for r in ratios], a_over_c_mean=round(float(np.mean(ratios)), 3),
                               a_over_c_spread=round(float(max(ratios) - min(ratios)), 3),
                               run_to_run={k: round(abs(v[0] - v[1]) / min(v), 4) for k, v in zip("abcd", (a, b, c, d))},
                               frames_per_s={k: round(chunk / float(np.mean(v)) * 1e3, 1) for k, v in zip("abcd", (a, b, c, d))})
    return out


def kernel_stats(path):
    rows = []
    with open(path) as f:
        for r in csv.DictReader(f):
            if "jpeg" in r.get("Name", ""):
                rows.append(dict(kernel=r["Name"].split("::")[2].split("(")[0] if r["Name"].count("::") > 1 else r["Name"], calls=int(r["Calls"]), total_ms=round(float(r["TotalDurationNs"]) / 1e6, 3),
                                 mean_ms=round(float(r["AverageNs"]) / 1e6, 4), max_ms=round(float(r["MaxNs"]) / 1e6, 4),
                                 min_ms=round(float(r["MinNs"]) / 1e6, 4)))
    return rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "jpeg_progressive.json"))
    ap.add_argument("--chunks", default="64,256,1024")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-stats")
    a = ap.parse_args()
    chunks = [int(c) for c in a.chunks.split(",")]
    if a.kernel_stats:
        record = json.load(open(a.out)) if os.path.exists(a.out) else {}
        record["kernel_stats_progressive_chunk_256"] = kernel_stats(a.kernel_stats)
        json.dump(record, open(a.out, "w"), indent=1)
        return
    dev = torch.device("cuda", 0)
    if a.trace_run:
        call, out, status = scans_call(streams()["progressive"], 256, dev)
        for _ in range(bj.TRACE_CALLS):
            call()
        torch.cuda.synchronize()
        assert not status.any()
        return
    rows = measure(dev, chunks)
    record = json.load(open(a.out)) if os.path.exists(a.out) else {}
    record.update(workload="800x450 4:2:0 quality 95", device=torch.cuda.get_device_name(0), rows=rows, summary=summary(rows, chunks),
                  method=f"device events, 2 warm-up calls, windows of >= {MIN_CALLS} calls and >= {MIN_SECONDS} s, every list twice")
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    json.dump(record, open(a.out, "w"), indent=1)
    print(json.dumps(record["summary"], indent=1))


if __name__ == "__main__":
    main()
