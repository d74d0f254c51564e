"""Time the people mesh overlay (pr_render_people, csrc/render.hip): 64 canvases of 800x450, closed
synthetic bodies with SMPL's counts (V = 6890, F = 13776), REBA-like part colours, depth steps from render.people_z_step.

(a) K = 1 body a canvas through pr_render_people against pr_render_overlay on the same inputs (scripts/bench_render.py's
    scene) in the same process, alternating round by round; whether the two write the same bytes.  The only comparison with
    a baseline.
(b) K = 4 and K = 16 bodies a canvas (N = 256 and 1024 meshes), of different sizes across the frame.
Per case: ms per batch (median of the rounds), canvases/s, the covered fraction, the bytes a call cannot avoid -- per canvas
pixel 8 (key clear) + 8 (key read) + 3 (frame) + 3 (out), per vertex 12 (read) + 16 + 16 (fixed point written and read) --
and the share of the HBM streaming floor reached; and what a mesh beyond the first costs, from K = 1 to 4 and 4 to 16.

usage: python scripts/bench_people_mesh.py [--batch 64] [--iters 30] [--rounds 7] [--warmup 3] [--out profiles/people_mesh.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from poserisk_release_amd import _lib, render, synth  # noqa: E402
import bench_render  # noqa: E402
import bench_video  # noqa: E402

HBM_BYTES_PER_S = bench_render.HBM_BYTES_PER_S
SCALE, ALPHA = 1.2, 0.6


def crowd(B, K, H, W, seed):
    """K bodies on each of B canvases, mesh n = canvas n // K: (verts, faces, cam, bboxes, canvas)."""
    rng = np.random.default_rng(seed)
    v, faces = synth.closed_body()
    verts, cams, boxes = [], [], []
    for _ in range(B * K):
        a = rng.uniform(-0.6, 0.6)
        R = np.array([[np.cos(a), 0, np.sin(a)], [0, 1, 0], [-np.sin(a), 0, np.cos(a)]])
        verts.append(v @ R.T)
        cams.append([rng.uniform(0.85, 1.0), rng.normal(0, 0.05), rng.normal(0, 0.05)])
        h = rng.uniform(0.4, 0.9) * H
        boxes.append([rng.uniform(0.15, 0.85) * W, rng.uniform(0.45, 0.55) * H, h, h])
    return np.array(verts, np.float32), faces, np.array(cams, np.float32), np.array(boxes, np.float32), np.arange(B * K, dtype=np.int32) // K


def people_call(scene, frames, fpart, rgb, dev):
    """-> (callable that enqueues one pr_render_people, its out tensor, its face_id tensor)."""
    verts, faces, cam, bb, canvas = scene
    M, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    N, V, F = verts.shape[0], verts.shape[1], faces.shape[0]
    z = render.people_z_step(cam, bb, SCALE, H, W)
    t = dict(v=torch.from_numpy(verts).to(dev), f=torch.from_numpy(faces).to(dev), c=torch.from_numpy(cam).to(dev), b=torch.from_numpy(bb).to(dev),
             canvas=torch.from_numpy(canvas).to(dev), z=torch.from_numpy(z).to(dev), fp=torch.from_numpy(fpart).to(dev),
             rgb=torch.from_numpy(rgb).to(dev), out=torch.empty((M, H, W, 3), dtype=torch.uint8, device=dev),
             fid=torch.empty((M, H, W), dtype=torch.int32, device=dev))
    lib = _lib.load()
    nb = lib.pr_render_people_workspace_bytes(N, M, V, F, H, W)
    t["ws"] = torch.empty((nb,), dtype=torch.uint8, device=dev)
    stream = torch.cuda.current_stream(dev).cuda_stream

    def args(face_id):
        return _lib.RenderPeopleArgs(t["v"].data_ptr(), t["f"].data_ptr(), t["c"].data_ptr(), t["b"].data_ptr(), frames.data_ptr(),
                                     t["canvas"].data_ptr(), None, t["z"].data_ptr(), t["fp"].data_ptr(), t["rgb"].data_ptr(), t["out"].data_ptr(),
                                     t["fid"].data_ptr() if face_id else None, None, None, None, N, M, V, F, rgb.shape[1], M, H, W, 0, SCALE, ALPHA)
    _lib.check(lib.pr_render_people(args(True), t["ws"].data_ptr(), nb, stream), "pr_render_people")      # once with face_id: the coverage
    timed = args(False)
    call = lambda: _lib.check(lib.pr_render_people(timed, t["ws"].data_ptr(), nb, stream), "pr_render_people")
    call.keep = (t, timed)
    return call, t["out"], t["fid"]


def overlay_call(scene, frames, fpart, rgb, dev):
    """pr_render_overlay on the K = 1 scene, as scripts/bench_render.py calls it -> (callable, its out tensor)."""
    verts, faces, cam, bb, _ = scene
    B, H, W = int(frames.shape[0]), int(frames.shape[1]), int(frames.shape[2])
    V, F = verts.shape[1], faces.shape[0]
    t = dict(v=torch.from_numpy(verts).to(dev), f=torch.from_numpy(faces).to(dev), c=torch.from_numpy(cam).to(dev), b=torch.from_numpy(bb).to(dev),
             fp=torch.from_numpy(fpart).to(dev), rgb=torch.from_numpy(rgb).to(dev), out=torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev))
    lib = _lib.load()
    nb = lib.pr_render_workspace_bytes(B, V, F, H, W)
    t["ws"] = torch.empty((nb,), dtype=torch.uint8, device=dev)
    a = _lib.RenderArgs(t["v"].data_ptr(), t["f"].data_ptr(), t["c"].data_ptr(), t["b"].data_ptr(), frames.data_ptr(), None, t["fp"].data_ptr(),
                        t["rgb"].data_ptr(), t["out"].data_ptr(), None, None, None, B, V, F, rgb.shape[1], B, H, W, 0, SCALE, ALPHA)
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda: _lib.check(lib.pr_render_overlay(a, t["ws"].data_ptr(), nb, stream), "pr_render_overlay")
    call.keep = (t, a)
    return call, t["out"]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--height", type=int, default=450)
    ap.add_argument("--width", type=int, default=800)
    ap.add_argument("--people", default="1,4,16")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_people_mesh.py needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    B, H, W = a.batch, a.height, a.width
    Ks = [int(k) for k in a.people.split(",")]
    rng = np.random.default_rng(1)
    frames = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    faces = synth.closed_body()[1]
    fpart = render.face_parts(synth.smpl_model(V=6890, seed=2)["weights"], faces, "REBA").astype(np.int32)
    colours = lambda n: render.part_colours(rng.integers(1, 6, (n, 10)).astype(np.int32), "REBA")
    one = bench_render.scene(B, H, W) + (np.arange(B, dtype=np.int32),)
    rgb1 = colours(B)
    calls, outs, fids, meshes = {}, {}, {}, {}
    calls["render_overlay"], outs["render_overlay"] = overlay_call(one, frames, fpart, rgb1, dev)
    for K in Ks:
        scene = one if K == 1 else crowd(B, K, H, W, seed=K)
        name = f"render_people_K{K}"
        calls[name], outs[name], fids[name] = people_call(scene, frames, fpart, rgb1 if K == 1 else colours(B * K), dev)
        meshes[name] = B * K
    for call in calls.values():
        for _ in range(a.warmup):
            call()
    torch.cuda.synchronize()
    same_bytes = bool(torch.equal(outs["render_overlay"], outs["render_people_K1"])) if 1 in Ks else None
    rounds = {k: [] for k in calls}
    for _ in range(a.rounds):                                     # alternating: every round times each of them once
        for k, call in calls.items():
            rounds[k].append(bench_video.time_ms(call, a.iters))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    V = one[0].shape[1]

    def shape(k):
        n = meshes.get(k, B)
        nb = B * H * W * (8 + 8 + 3 + 3) + n * V * (12 + 16 + 16)
        rec = {"meshes": n, "ms_per_batch": round(med[k], 4), "canvases_per_s": round(B / med[k] * 1e3, 1), "floor_bytes": nb,
               "floor_ms": round(nb / HBM_BYTES_PER_S * 1e3, 4), "share_of_floor": round(nb / HBM_BYTES_PER_S * 1e3 / med[k], 4)}
        if k in fids:
            rec["covered_fraction"] = round(float((fids[k] >= 0).float().mean()), 4)
        return rec
    rec = {"batch": B, "iters": a.iters, "rounds": a.rounds, "frame": [H, W], "V": V, "F": int(faces.shape[0]), **{k: shape(k) for k in med}}
    if 1 in Ks:
        spread = max(rounds["render_overlay"]) - min(rounds["render_overlay"])
        rec["K1_bytes_equal_render_overlay"] = same_bytes
        rec["K1_over_render_overlay"] = round(med["render_people_K1"] / med["render_overlay"], 4)
        rec["K1_within_render_overlay_spread"] = bool(med["render_people_K1"] <= med["render_overlay"] + spread)
    steps = [(lo, hi) for lo, hi in zip(Ks, Ks[1:])]
    rec["ms_per_added_mesh"] = {f"K{lo}_to_K{hi}": round((med[f"render_people_K{hi}"] - med[f"render_people_K{lo}"]) / (B * (hi - lo)), 6)
                                for lo, hi in steps}
    rec["ms_per_round"] = {k: [round(x, 4) for x in v] for k, v in rounds.items()}
    rec.update(floor_bytes_per_s=HBM_BYTES_PER_S, device=torch.cuda.get_device_name(0), library=_lib.load().pr_build_info().decode())
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
