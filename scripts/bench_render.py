"""Time the mesh overlay (pr_render_overlay, csrc/render.hip) at the flagship shape: B crops over B distinct 800x450 frames,
a closed synthetic body with SMPL's counts (V = 6890, F = 13776) at person size, REBA-like part colours.  Prints ms per
batch, frames/s, the HBM traffic floor, and the numpy reference's time for one frame (tests/raster_ref.py).

usage: python scripts/bench_render.py [--batch 64] [--iters 50] [--rounds 1] [--warmup 5] [--out profiles/<name>.json]
(--rounds R: ms_per_batch is the median of R timed rounds of --iters calls, each listed in ms_per_round)"""
import argparse
import json
import os
import sys
import time

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

from poserisk_release_amd import _lib, render, synth  # noqa: E402

HBM_BYTES_PER_S = 5.3e12   # achievable streaming rate used for the floor (MI355X_MICROARCH.md)


def scene(B, H, W, seed=0):
    rng = np.random.default_rng(seed)
    v, faces = synth.closed_body()
    verts, cams, boxes = [], [], []
    for _ in range(B):
        a = rng.uniform(-0.6, 0.6)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        verts.append(v @ R.T)
        cams.append([rng.uniform(0.85, 1.0), rng.normal(0, 0.05), rng.normal(0, 0.05)])
        h = rng.uniform(0.7, 0.9) * H
        boxes.append([rng.uniform(0.3, 0.7) * W, rng.uniform(0.45, 0.55) * H, h, h])
    return np.array(verts, np.float32), faces, np.array(cams, np.float32), np.array(boxes, np.float32)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=1)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--height", type=int, default=450)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_render.py needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    B, H, W = a.batch, a.height, a.width
    verts, faces, cam, bb = scene(B, H, W)
    rng = np.random.default_rng(1)
    frames = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    fpart = render.face_parts(synth.smpl_model(V=6890, seed=2)["weights"], faces, "REBA")
    rgb = render.part_colours(rng.integers(1, 6, (B, 10)).astype(np.int32), "REBA")
    v_d = torch.from_numpy(verts).to(dev)
    f_d = torch.from_numpy(faces).to(dev)
    kw = dict(scale=1.2, face_part=torch.from_numpy(fpart).to(dev), part_rgb=torch.from_numpy(rgb).to(dev), alpha=0.6)
    out = torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev)
    c_d, b_d = torch.from_numpy(cam).to(dev), torch.from_numpy(bb).to(dev)
    # the kernel alone (the wrapper's host-side face check and uploads are per call; time the C entry as a user's loop would)
    lib = _lib.load()
    V, F = verts.shape[1], faces.shape[0]
    nb = lib.pr_render_workspace_bytes(B, V, F, H, W)
    ws = torch.empty((nb,), dtype=torch.uint8, device=dev)
    fp_d, rgb_d = kw["face_part"].to(torch.int32).contiguous(), kw["part_rgb"].contiguous()
    args = _lib.RenderArgs(v_d.data_ptr(), f_d.data_ptr(), c_d.data_ptr(), b_d.data_ptr(), frames.data_ptr(), None,
                           fp_d.data_ptr(), rgb_d.data_ptr(), out.data_ptr(), None, None, None,
                           B, V, F, rgb_d.shape[1], B, H, W, 0, 1.2, 0.6)
    stream = torch.cuda.current_stream(dev).cuda_stream
    for _ in range(a.warmup):
        _lib.check(lib.pr_render_overlay(args, ws.data_ptr(), nb, stream), "pr_render_overlay")
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    rounds = []
    for _ in range(a.rounds):
        e0.record()
        for _ in range(a.iters):
            lib.pr_render_overlay(args, ws.data_ptr(), nb, stream)
        e1.record()
        torch.cuda.synchronize()
        rounds.append(e0.elapsed_time(e1) / a.iters)
    ms = float(np.median(rounds))
    # the wrapper end to end (host face check, uploads, workspace) for comparison
    t0 = time.perf_counter()
    for _ in range(5):
        render.overlay(frames, v_d, faces, c_d, b_d, out=out, **kw)
    torch.cuda.synchronize()
    wrapper_ms = (time.perf_counter() - t0) / 5 * 1e3
    _, fid = render.overlay(frames, v_d, faces, c_d, b_d, return_face_id=True, **kw)
    coverage = float((fid >= 0).float().mean())
    floor_bytes = B * H * W * (8 + 8 + 3 + 3)       # clear + key read + frame read + out write
    # the numpy reference on one frame
    import raster_ref as rr
    t0 = time.perf_counter()
    vfx = rr.vert_fx(verts[:1], cam[:1], bb[:1], 1.2, H, W)
    keys = rr.raster_keys(vfx[0], faces, H, W)
    rr.composite(frames[0].cpu().numpy(), rr.face_id(keys), rr.face_colours(verts[0], faces, fpart, rgb[0]), 0.6)
    numpy_ms = (time.perf_counter() - t0) * 1e3
    rec = {"batch": B, "height": H, "width": W, "V": V, "F": F, "ms_per_batch": round(ms, 4), "ms_per_round": [round(x, 4) for x in rounds],
           "frames_per_s": round(B / ms * 1e3, 1), "wrapper_ms_per_batch": round(wrapper_ms, 3),
           "covered_fraction": round(coverage, 4), "traffic_floor_bytes": floor_bytes,
           "traffic_floor_ms": round(floor_bytes / HBM_BYTES_PER_S * 1e3, 4),
           "numpy_ms_per_frame": round(numpy_ms, 1), "speedup_vs_numpy_per_frame": round(numpy_ms / (ms / B), 1),
           "device": torch.cuda.get_device_name(0), "library": _lib.load().pr_build_info().decode()}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
