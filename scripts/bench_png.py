"""Measures the PNG decoder (poserisk_release_amd/png.py) and writes profiles/png_decode.json.

Workload: 800 x 450 RGB frames (a synthetic scene with sensor-like noise, 16 distinct frames cycled) written three ways -- by
Pillow at its default level, by Pillow at compress_level=1, by the stored-only writer of tests/png_cases.py -- decoded 64, 256
and 1024 frames a call.  Yardsticks in the same run on the same box: Pillow on 16 threads decoding the same files, a raw upload
of the same pixels from pinned memory, pr_jpeg_decode_sync on Pillow's q95 JPEG encoding of the same pixels.  And a folder of
256 PNG frames to scores end to end (the Predictor with synthetic weights).

    python scripts/bench_png.py            runs every step as a child process under its own `timeout`, one after the other; the
                                           first step that fails ends the run with its exit status
    python scripts/bench_png.py --step S   one step (make | png | pillow | upload | jpeg | folder), results to --work/S.json
"""
import argparse
import io
import json
import os
import pickle
import subprocess
import sys
import tempfile
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))
STEPS = (("make", 300), ("png", 420), ("pillow", 240), ("upload", 120), ("jpeg", 240), ("folder", 300))   # (name, seconds)
CALLS = (64, 256, 1024)
H, W, DISTINCT = 450, 800, 16


def _frames():
    import numpy as np
    y, x = np.mgrid[0:H, 0:W]
    out = []
    for k in range(DISTINCT):
        scene = np.stack([(x + 13 * k) * 255 // (W + 13 * DISTINCT), y * 255 // H, ((x // 16 + (y + 5 * k) // 16) % 2) * 200], axis=2)
        noise = np.random.default_rng(k).normal(0, 6, scene.shape)
        out.append((scene + noise).clip(0, 255).astype(np.uint8))
    return out


def step_make(work):
    import numpy as np
    from PIL import Image
    import png_cases as pc
    frames = _frames()
    files = {"pillow_default": [], "pillow_level1": [], "stored": [], "jpeg_q95": []}
    for px in frames:
        for key, kw in (("pillow_default", {}), ("pillow_level1", {"compress_level": 1})):
            b = io.BytesIO()
            Image.fromarray(px).save(b, "PNG", **kw)
            files[key].append(b.getvalue())
        files["stored"].append(pc.png(W, H, 2, pc.stored(pc.filter_rows(px.reshape(H, W * 3), 3, 0))))
        b = io.BytesIO()
        Image.fromarray(px).save(b, "JPEG", quality=95)
        files["jpeg_q95"].append(b.getvalue())
    with open(os.path.join(work, "files.pkl"), "wb") as f:
        pickle.dump(dict(files=files, pixels=np.stack(frames)), f)
    import torch
    from poserisk_release_amd import _lib
    res = {k: dict(mean_bytes=int(np.mean([len(b) for b in v]))) for k, v in files.items()}
    res["device"] = torch.cuda.get_device_name(0) if torch.cuda.is_available() else "none"
    res["library"] = _lib.load().pr_build_info().decode()
    return res


def _load(work):
    with open(os.path.join(work, "files.pkl"), "rb") as f:
        return pickle.load(f)


def _time_gpu(fn, reps=3):
    import torch
    fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(reps):
        t = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    return sorted(times)[len(times) // 2]


def step_png(work):
    import numpy as np
    import torch
    from poserisk_release_amd import png
    d = _load(work)
    dev = torch.device("cuda", 0)
    out = {}
    for key in ("pillow_default", "pillow_level1", "stored"):
        files = d["files"][key]
        got, st = png.decode_files(files, dev)
        assert not st.any() and np.array_equal(got.cpu().numpy(), d["pixels"]), key      # what is timed is right
        for n in CALLS:
            batch = [files[i % DISTINCT] for i in range(n)]
            sec = _time_gpu(lambda: png.decode_files(batch, dev, chunk=n))
            out[f"{key}_{n}"] = dict(frames=n, seconds=round(sec, 5), frames_per_s=round(n / sec, 1), ms_per_frame_in_flight=round(1e3 * sec, 2))
    return out


def step_pillow(work):
    from concurrent.futures import ThreadPoolExecutor
    import numpy as np
    from PIL import Image
    d = _load(work)
    out = {}

    def one(b):
        return np.asarray(Image.open(io.BytesIO(b)).convert("RGB"))
    for key in ("pillow_default", "pillow_level1", "stored"):
        batch = [d["files"][key][i % DISTINCT] for i in range(256)]
        one(batch[0])                                                # first use of the decoder is not a decode time
        t = time.perf_counter()
        for b in batch[:8]:
            one(b)
        single = (time.perf_counter() - t) / 8
        with ThreadPoolExecutor(16) as ex:
            list(ex.map(one, batch[:32]))
            t = time.perf_counter()
            list(ex.map(one, batch))
            sec = time.perf_counter() - t
        out[key] = dict(frames=256, threads=16, seconds=round(sec, 4), frames_per_s=round(256 / sec, 1), one_frame_one_thread_ms=round(1e3 * single, 2))
    return out


def step_upload(work):
    import torch
    d = _load(work)
    out = {}
    for n in CALLS:
        host = torch.from_numpy(d["pixels"]).repeat((n // DISTINCT, 1, 1, 1)).pin_memory()
        dst = torch.empty_like(host, device="cuda")
        sec = _time_gpu(lambda: dst.copy_(host, non_blocking=True))
        out[str(n)] = dict(frames=n, seconds=round(sec, 5), frames_per_s=round(n / sec, 1))
    return out


def step_jpeg(work):
    import torch
    from poserisk_release_amd import jpeg
    d = _load(work)
    dev = torch.device("cuda", 0)
    out = {}
    for n in CALLS:
        batch = [d["files"]["jpeg_q95"][i % DISTINCT] for i in range(n)]
        _, st = jpeg.decode_files(batch, dev, chunk=n, entropy="sync")
        assert not st.any()
        sec = _time_gpu(lambda: jpeg.decode_files(batch, dev, chunk=n, entropy="sync"))
        out[str(n)] = dict(frames=n, entry="pr_jpeg_decode_sync", seconds=round(sec, 5), frames_per_s=round(n / sec, 1))
    return out


def step_folder(work):
    import types
    import numpy as np
    import torch
    from poserisk_release_amd import dropin, synth
    dropin.install()
    from core import base
    from models import hmr
    from smpl import SMPL
    d = _load(work)
    clip = os.path.join(work, "clip")
    os.makedirs(clip, exist_ok=True)
    n = 256
    for i in range(n):
        with open(os.path.join(clip, "{0:09d}.png".format(i)), "wb") as f:
            f.write(d["files"]["pillow_default"][i % DISTINCT])
    track = {1: {"bbox": np.stack([np.array([400 + (i % 40), 225, 170, 330], np.float32) for i in range(n)]), "frames": np.arange(n)}}
    with open(os.path.join(clip, "tracking.pkl"), "wb") as f:
        pickle.dump(track, f)
    info = os.path.join(work, "info.json")
    with open(info, "w") as f:
        json.dump(synth.EXAMPLE_INFO, f)
    dev = torch.device("cuda", 0)
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=dev)
    args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1)
    pred = base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=64)
    pred(clip, info, os.path.join(work, "out0"))
    torch.cuda.synchronize()
    times = []
    for r in range(3):
        t = time.perf_counter()
        out = pred(clip, info, os.path.join(work, f"out{r + 1}"))
        torch.cuda.synchronize()
        times.append(time.perf_counter() - t)
    sec = sorted(times)[1]
    return dict(frames=n, scored=int(len(out["frames"])), seconds=round(sec, 4), frames_per_s=round(n / sec, 1),
                note="folder of Pillow-default PNG files on disk -> REBA / RULA scores and report files, synthetic weights")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--step")
    ap.add_argument("--work")
    ap.add_argument("--out", default=os.path.join(REPO, "profiles", "png_decode.json"))
    a = ap.parse_args()
    if a.step:
        res = globals()["step_" + a.step](a.work)
        with open(os.path.join(a.work, a.step + ".json"), "w") as f:
            json.dump(res, f)
        return 0
    record = dict(workload=f"{W}x{H} RGB, {DISTINCT} distinct frames cycled; medians of 3 timed calls behind one warm-up call, host file "
                           "bytes in memory -> pixels on the device (parse, one upload, three kernels), synchronised",
                  calls=list(CALLS))
    with tempfile.TemporaryDirectory() as work:
        for name, limit in STEPS:
            r = subprocess.run(["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name, "--work", work])
            if r.returncode != 0:
                print(f"bench_png: step {name} ended with status {r.returncode}; nothing after it was started", file=sys.stderr)
                return r.returncode
            with open(os.path.join(work, name + ".json")) as f:
                got = json.load(f)
            if name == "make":                                     # which device and build the record is of: top level
                record["device"], record["library"] = got.pop("device"), got.pop("library")
            record[{"make": "files", "png": "gpu_png_decode", "pillow": "pillow_16_threads", "upload": "raw_upload",
                    "jpeg": "gpu_jpeg_q95", "folder": "folder_to_scores"}[name]] = got
            print(name, json.dumps(record[list(record)[-1]]), flush=True)
            with open(a.out, "w") as f:                            # kept up to date: a later step's failure loses nothing
                json.dump(record, f, indent=1)
                f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
