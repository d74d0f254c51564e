"""Measure the JPEG decoder on 800x450 4:2:0 quality-95 frames -- what cv2.imwrite writes, the streams of
tests/golden/jpeg_frames.npz -- with and without restart markers, with the entropy stage both ways side by side in one run:
"serial" (pr_jpeg_decode, csrc/jpeg.hip: one lane per restart segment) and "sync" (pr_jpeg_decode_sync, csrc/jpeg_sync.hip: one
lane per sub-sequence; the rows carry the frames' rounds and how many fell back; `--sync-sweep 64,128,256` adds rows at other
sub-sequence sizes with 64 rounds allowed, from which the defaults were chosen):

  decode      frames/s of pr_jpeg_decode alone from device events (descriptors and bytes already on the device), at chunk sizes
              64, 256 and 1024, warmed up, windows of at least a second, the whole list run twice in the same process;
  files       jpeg.decode_files on file bytes in host memory (parse + pinned staging + upload + decode), wall clock;
  pillow      for comparison on the same host: Pillow on 16 threads plus the upload of its output ("not measured" where Pillow
              is not importable);
  raw_h2d     the upload of the same frames as a raw uint8 array from pinned memory;
  end_to_end  Predictor on a folder of JPEG frames + tracking.pkl -> scores, against the same frames as frames.npy -> scores, B = 64, fp32.

`--trace-run --variant V` only decodes a dozen chunks of 256 of one variant: run it under `rocprofv3 --kernel-trace --stats --
python scripts/bench_jpeg.py --trace-run --variant V` for per-kernel times, then `--kernel-stats <kernel_stats.csv> --variant V`
adds them, each against its byte floor, to the JSON.  The timed frames are DISTINCT different frames in rotation (see streams).

usage: python scripts/bench_jpeg.py [--out profiles/jpeg_decode.json] [--chunks 64,256,1024] [--skip-e2e] [--decode-only]
                                    [--sync-sweep 64,128,256]
       python scripts/bench_jpeg.py --trace-run [--entropy sync]
       python scripts/bench_jpeg.py --kernel-stats <csv> --out profiles/jpeg_decode.json      (no GPU needed)"""
import argparse
import csv
import json
import os
import pickle
import sys
import tempfile
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)

from poserisk_release_amd import _lib, jpeg  # noqa: E402

HBM_BYTES_PER_S = 5.3e12   # achievable streaming rate used for the floors (as scripts/bench_render.py)
H, W = 450, 800

TRACE_CALLS = 12   # decode calls of a --trace-run
DISTINCT = 16   # different frames per variant, so that the lanes of a wave do not all take the same branches

_STREAMS = {}


def streams():
    """{variant: [stream, ...]}: DISTINCT different 800x450 4:2:0 quality-95 frames per variant -- the golden frame's content
    rolled by a different offset each and encoded by Pillow, as tests/golden/make_jpeg_golden.py does for its four streams.  Without
    Pillow there is only the golden stream itself: every lane then decodes the same bits, which is the decoder's best case
    (`distinct_streams` in the record says which it was)."""
    if _STREAMS:
        return _STREAMS
    z = np.load(os.path.join(REPO, "tests", "golden", "jpeg_frames.npz"))
    off, s, names = z["offsets"], z["streams"], [str(n) for n in z["names"]]
    get = lambda n: s[off[names.index(n)]:off[names.index(n) + 1]].tobytes()
    _STREAMS.update({"no_restart": [get("420_q95")], "restart_per_mcu_row": [get("420_q95_rstrow")]})
    try:
        from PIL import Image
    except ImportError:
        return _STREAMS
    import io
    frame = np.asarray(Image.open(io.BytesIO(get("444_q95"))).convert("RGB"))
    for variant, kw in (("no_restart", {}), ("restart_per_mcu_row", dict(restart_marker_rows=1))):
        for i in range(1, DISTINCT):
            buf = io.BytesIO()
            Image.fromarray(np.roll(frame, (37 * i, 53 * i), axis=(0, 1))).save(buf, "JPEG", quality=95, subsampling=2, **kw)
            _STREAMS[variant].append(buf.getvalue())
    return _STREAMS


def repeated(blobs, n):
    return [blobs[i % len(blobs)] for i in range(n)]


def decode_call(blobs, chunk, dev, entropy="serial", sync_opts=None):
    """-> (callable enqueuing one pr_jpeg_decode / pr_jpeg_decode_sync of `chunk` frames, the streams in rotation; out tensor;
    status tensor); call.stats is the sync entry's per-frame statistics tensor (None for serial)."""
    items = repeated(blobs, chunk)
    blob = b"".join(items)
    frames, segs, huff, pst, h, w, offsets = jpeg.parse(items)
    assert not pst.any() and (h, w) == (H, W)
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a).view(np.uint8).reshape(-1).copy()).to(dev)
    t = dict(data=up(np.frombuffer(blob, np.uint8)), frames=up(frames), segs=up(segs), huff=up(huff),
             out=torch.empty((chunk, H, W, 3), dtype=torch.uint8, device=dev), status=torch.empty(chunk, dtype=torch.int32, device=dev),
             ws=torch.empty(jpeg.workspace_bytes(chunk, H, W) if entropy == "serial" else
                            jpeg.sync_workspace_bytes(chunk, H, W, len(blob), len(segs), sync_opts), dtype=torch.uint8, device=dev))
    args = _lib.JpegArgs(t["data"].data_ptr(), t["frames"].data_ptr(), t["segs"].data_ptr(), t["huff"].data_ptr(), t["out"].data_ptr(),
                         t["status"].data_ptr(), len(blob), chunk, H, W, len(segs), len(huff), 0)
    lib, stream = _lib.load(), torch.cuda.current_stream(dev).cuda_stream
    if entropy == "serial":
        call = lambda: _lib.check(lib.pr_jpeg_decode(args, t["ws"].data_ptr(), t["ws"].numel(), stream), "pr_jpeg_decode")
        call.stats = None
    else:
        t["stats"] = torch.zeros((chunk, 4), dtype=torch.int32, device=dev)
        opts = None if sync_opts is None else _lib.JpegSyncOpts(*sync_opts)
        call = lambda: _lib.check(lib.pr_jpeg_decode_sync(args, opts, t["stats"].data_ptr(), t["ws"].data_ptr(), t["ws"].numel(), stream),
                                  "pr_jpeg_decode_sync")
        call.stats = t["stats"]
    call.keep = (t, args)
    return call, t["out"], t["status"]


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


def measure_decode(dev, chunks, sweep=()):
    rows = []
    ways = [("serial", None), ("sync", None)] + [("sync", (S, 64)) for S in sweep]
    for run in (1, 2):
        for variant, blobs in streams().items():
            for chunk in chunks:
                reference = None
                for entropy, opts in ways:
                    call, out, status = decode_call(blobs, chunk, dev, entropy, opts)
                    call()
                    call()
                    torch.cuda.synchronize()
                    assert not status.any()
                    if reference is None:
                        reference = out[:DISTINCT].clone()
                    assert torch.equal(out[:DISTINCT], reference), (variant, chunk, entropy, opts)   # the same pixels either way
                    ms, n = timed_window(call)
                    row = dict(run=run, stream=variant, chunk=chunk, entropy=entropy, ms_per_call=round(ms, 3), calls_in_window=n,
                               frames_per_s=round(chunk / ms * 1e3, 1), distinct_streams=len(blobs),
                               compressed_bytes_per_frame=sum(map(len, blobs)) // len(blobs))
                    if call.stats is not None:
                        st = call.stats[:len(blobs)].cpu().numpy()             # the distinct frames, once each
                        row.update(sync_opts="default" if opts is None else list(opts), subseq_per_frame=int(st[:, 0].mean()),
                                   rounds=sorted(int(r) for r in st[:, 1]), fell_back=int(st[:, 2].sum()))
                    rows.append(row)
                    print(row, flush=True)
                    del call, out, status
                    torch.cuda.empty_cache()
    return rows


def measure_files(dev, chunks, n_frames=1024):
    out = {}
    for variant, blobs in streams().items():
        items = repeated(blobs, n_frames)
        for chunk in chunks:
            for entropy in ("serial", "sync"):
                jpeg.decode_files(items, dev, chunk=chunk, entropy=entropy)
                torch.cuda.synchronize()
                best = []
                for _ in range(3):
                    t0 = time.perf_counter()
                    jpeg.decode_files(items, dev, chunk=chunk, entropy=entropy)
                    torch.cuda.synchronize()
                    best.append(time.perf_counter() - t0)
                key = f"{variant}_chunk{chunk}_{entropy}"
                out[key] = dict(frames=n_frames, seconds=[round(b, 4) for b in best], frames_per_s=round(n_frames / min(best), 1))
                print("files", key, out[key], flush=True)
    return out


def measure_pillow(dev, n_frames=256):
    try:
        from PIL import Image
    except ImportError:
        return "not measured (Pillow is not importable on this host)"
    import io
    from concurrent.futures import ThreadPoolExecutor
    items = repeated(streams()["no_restart"], n_frames)
    one = lambda b: np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
    res = {}
    with ThreadPoolExecutor(16) as ex:
        for _ in range(2):
            t0 = time.perf_counter()
            arr = np.stack(list(ex.map(one, items)))
            t1 = time.perf_counter()
            torch.from_numpy(arr).to(dev)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res = dict(frames=n_frames, threads=16, decode_s=round(t1 - t0, 4), upload_s=round(t2 - t1, 4),
                       frames_per_s=round(n_frames / (t2 - t0), 1), decode_only_frames_per_s=round(n_frames / (t1 - t0), 1))
    return res


def measure_raw_h2d(dev, n_frames=256):
    host = torch.empty((n_frames, H, W, 3), dtype=torch.uint8).pin_memory()
    host.random_(0, 256)
    devt = torch.empty(host.shape, dtype=torch.uint8, device=dev)
    devt.copy_(host, non_blocking=True)
    torch.cuda.synchronize()
    ms, n = timed_window(lambda: devt.copy_(host, non_blocking=True))
    return dict(frames=n_frames, bytes=host.numel(), ms=round(ms, 3), gb_per_s=round(host.numel() / ms / 1e6, 2),
                frames_per_s=round(n_frames / ms * 1e3, 1))


def measure_end_to_end(dev, n_frames=256):
    import types
    from poserisk_release_amd import dropin, synth
    dropin.install()
    from core import base
    from models import hmr
    from smpl import SMPL
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=dev)
    args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1)
    pred = base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=64)
    items = repeated(streams()["no_restart"], n_frames)
    track = {1: {"bbox": np.tile(np.array([[380, 225, 170, 330]], np.float32), (n_frames, 1)), "frames": np.arange(n_frames)}}
    res = {}
    with tempfile.TemporaryDirectory() as d:
        for name in ("jpg", "npy"):
            os.makedirs(os.path.join(d, name))
            with open(os.path.join(d, name, "tracking.pkl"), "wb") as f:
                pickle.dump(track, f)
        for i in range(n_frames):
            with open(os.path.join(d, "jpg", "{0:09d}.jpg".format(i)), "wb") as f:
                f.write(items[i])
        frames, _ = jpeg.decode_files(items, dev)
        np.save(os.path.join(d, "npy", "frames.npy"), frames.cpu().numpy())
        del frames
        for name in ("jpg", "npy", "jpg", "npy"):
            t0 = time.perf_counter()
            fr, bgr, fps, tr = pred.load_front_end(os.path.join(d, name), d)
            torch.cuda.synchronize()
            t1 = time.perf_counter()
            out = pred.score_frames(fr, tr, synth.EXAMPLE_INFO, bgr=bgr)
            torch.cuda.synchronize()
            t2 = time.perf_counter()
            res.setdefault(name, []).append(dict(front_end_s=round(t1 - t0, 4), score_s=round(t2 - t1, 4),
                                                 frames_per_s=round(n_frames / (t2 - t0), 1)))
            print("end_to_end", name, res[name][-1], flush=True)
            assert len(out["frames"]) == n_frames
    return dict(frames=n_frames, batch=64, precision="fp32", jpeg_folder=res["jpg"], frames_npy=res["npy"],
                note="files in a temporary directory (page cache); the first pass of each is the cold one")


def kernel_stats(path, record, variant):
    """rocprofv3's kernel_stats.csv of a --trace-run -> per-kernel mean times at chunk 256, each against its byte floor.  The
    clear of the coefficient workspace is the runtime's fill kernel (the 1 KB clear of the status words runs the same kernel:
    its calls are in the count; the time given is the slowest fill, which is the workspace's 2.2 MB a frame)."""
    chunk = 256
    pw, ph = (W + 15) // 16 * 16, (H + 15) // 16 * 16
    samples = pw * ph * 3 // 2                                   # 4:2:0: luma + two quarter planes, block padded
    comp = {r["stream"]: r["compressed_bytes_per_frame"] for r in record.get("decode", [])}.get(variant, 0)
    floors = {"jpeg_entropy_kernel": ("compressed bytes in + non-zero int16 coefficients out (at most 2 B a sample); bound by the "
                                      "serial dependent chain of one lane per segment, not by bytes", comp + 2 * samples),
              "fillBuffer": ("the clear of the int16 coefficient workspace, sized for 4:4:4 (3 padded planes): 2 B a sample written",
                             2 * 3 * pw * ph),
              "jpeg_idct_kernel": ("int16 coefficients in, u8 samples out", 3 * samples),
              "jpeg_colour_kernel": ("u8 planes in, 3 B a pixel out", samples + 3 * H * W),
              "jpeg_sync_decode_kernel": ("all launches of a call together (cold pass, rounds, write pass): compressed bytes in once a "
                                          "pass + coefficients out once; bound by the dependent chain of one sub-sequence", comp + 2 * samples),
              "jpeg_sync_map_kernel": ("one lane per segment: 4 B a sub-sequence written", 0),
              "jpeg_sync_scan_kernel": ("one lane per segment: a serial walk over its sub-sequences' counts", 0)}
    out = {}
    with open(path) as f:
        for row in csv.DictReader(f):
            name = row.get("Name") or row.get("KernelName") or ""
            for k, (what, nbytes) in floors.items():
                if k in name:
                    mean_ms = float(row["AverageNs"]) / 1e6
                    if k.startswith("jpeg_sync"):            # several launches a decode call: their sum, per call of the trace run
                        mean_ms = float(row["TotalDurationNs"]) / 1e6 / TRACE_CALLS
                    if k == "fillBuffer":                    # two fills a decode call: the slowest one is the workspace's
                        mean_ms = float(row["MaxNs"]) / 1e6
                    floor_ms = chunk * nbytes / HBM_BYTES_PER_S * 1e3
                    if not nbytes:
                        out[k] = dict(calls=int(row["Calls"]), mean_ms=round(mean_ms, 4), bound=what)
                        continue
                    out[k] = dict(calls=int(row["Calls"]), mean_ms=round(mean_ms, 4), total_ms=round(float(row["TotalDurationNs"]) / 1e6, 3)
                                  if "TotalDurationNs" in row else None, bytes_per_call=chunk * nbytes, bound=what,
                                  floor_ms=round(floor_ms, 4), share_of_floor=round(floor_ms / mean_ms, 4))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--chunks", default="64,256,1024")
    ap.add_argument("--skip-e2e", action="store_true")
    ap.add_argument("--decode-only", action="store_true", help="the device-event rates alone (A/B of ablation builds)")
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--kernel-stats", default=None)
    ap.add_argument("--variant", default="no_restart", choices=("no_restart", "restart_per_mcu_row"))
    ap.add_argument("--entropy", default="serial", choices=("serial", "sync"), help="which entry --trace-run decodes with")
    ap.add_argument("--sync-sweep", default="", help="further sub-sequence sizes for the device-event rates, 64 rounds allowed")
    a = ap.parse_args()
    if a.kernel_stats:
        record = json.load(open(a.out)) if a.out and os.path.exists(a.out) else {}
        key = a.variant if a.entropy == "serial" else a.variant + "_sync"
        record.setdefault("kernels_chunk256", {})[key] = kernel_stats(a.kernel_stats, record, a.variant)
        print(json.dumps(record["kernels_chunk256"][key], indent=1))
        if a.out:
            json.dump(record, open(a.out, "w"), indent=1)
        return
    dev = torch.device("cuda", 0)
    if a.trace_run:
        call, out, status = decode_call(streams()[a.variant], 256, dev, a.entropy)
        for _ in range(TRACE_CALLS):
            call()
        torch.cuda.synchronize()
        assert not status.any()
        return
    chunks = [int(c) for c in a.chunks.split(",")]
    record = dict(device=torch.cuda.get_device_name(0), library=_lib.load().pr_build_info().decode(), frame="800x450 4:2:0 quality 95",
                  decode=measure_decode(dev, chunks, [int(v) for v in a.sync_sweep.split(",") if v]))
    if not a.decode_only:
        record.update(files=measure_files(dev, chunks),
                  pillow_16_threads=measure_pillow(dev), raw_h2d=measure_raw_h2d(dev))
    if not a.skip_e2e and not a.decode_only:
        record["end_to_end"] = measure_end_to_end(dev)
    print(json.dumps(record))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            json.dump(record, f, indent=1)


if __name__ == "__main__":
    main()
