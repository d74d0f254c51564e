"""Time the annotated-video compositor (pr_compose_video, csrc/compose.hip): B canvases from B distinct frames, a track box on
every frame and a REBA panel of nine lines, at 800x450 (the flagship shape) and 1920x1080.  In the same process, alternating
with it round by round, the mesh overlay (pr_render_overlay) on the same 800x450 frames with scripts/bench_render.py's scene:
the compositor streams fewer bytes and rasterises nothing, so it has to be the faster of the two.  Prints one JSON line: ms per
batch, frames/s, the bytes moved computed from the shapes, and the share of the HBM streaming floor reached.

usage: python scripts/bench_video.py [--batch 64] [--iters 200] [--rounds 7] [--warmup 5] [--out profiles/<name>.json]"""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from poserisk_release_amd import _lib, render, synth, video  # noqa: E402
import bench_render  # noqa: E402

HBM_BYTES_PER_S = bench_render.HBM_BYTES_PER_S


def compose_call(B, H, W, dev, seed=0):
    """-> (callable that enqueues one pr_compose_video of B canvases, frames tensor, bytes moved per call)."""
    rng = np.random.default_rng(seed)
    frames = torch.from_numpy(rng.integers(0, 256, (B, H, W, 3), dtype=np.uint8)).to(dev)
    dst_h, dst_w, panel_w = video.canvas_size(H, W)
    items = ['Trunk', 'Neck', 'Leg', 'Upper_arm (L,R)', 'Lower_arm (L,R)', 'Wrist (L,R)']
    logs = np.array([[f"{rng.integers(1, 5)},{rng.integers(1, 5)}" if "(L,R)" in it else str(rng.integers(1, 5)) for it in items]
                     for _ in range(B)])
    h = rng.uniform(0.7, 0.9, B) * H
    bboxes = np.stack([rng.uniform(0.3, 0.7, B) * W, rng.uniform(0.45, 0.55, B) * H, h, h], 1).astype(np.float32)
    draw = video.draw_list("REBA", B, bboxes, (0, np.arange(B), B), rng.integers(1, 13, B), items, logs, dst_h)
    lines, codes = video.pack_lines(draw.text)
    atlas = video.font_atlas()
    t = dict(box=torch.from_numpy(draw.box).to(dev), lines=torch.from_numpy(lines).to(dev), text=torch.from_numpy(codes).to(dev),
             cov=torch.from_numpy(np.array(atlas.cov)).to(dev),
             out=torch.empty((B, dst_h, dst_w + panel_w, 3), dtype=torch.uint8, device=dev))
    args = _lib.ComposeArgs(frames.data_ptr(), None, t["box"].data_ptr(), t["lines"].data_ptr(), t["text"].data_ptr(),
                            t["cov"].data_ptr(), t["out"].data_ptr(), None, B, B, H, W, dst_h, dst_w, panel_w,
                            lines.shape[1], codes.shape[2], 3, video.CELL_H, video.CELL_W)
    args.adv[:3], args.ascent[:3] = atlas.adv, atlas.ascent
    args.box_rgb[:3] = video.GREEN
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda: _lib.check(lib.pr_compose_video(args, stream), "pr_compose_video")
    call.keep = (t, args)                                         # the tensors the argument struct points into
    return call, frames, B * 3 * (H * W + dst_h * (dst_w + panel_w))


def overlay_call(frames, dev):
    """One pr_render_overlay on `frames` with bench_render.py's scene -> (callable, its traffic floor in bytes)."""
    B, H, W, _ = frames.shape
    verts, faces, cam, bb = bench_render.scene(B, H, W)
    rng = np.random.default_rng(1)
    fpart = render.face_parts(synth.smpl_model(V=6890, seed=2)["weights"], faces, "REBA")
    rgb = render.part_colours(rng.integers(1, 6, (B, 10)).astype(np.int32), "REBA")
    t = dict(v=torch.from_numpy(verts).to(dev), f=torch.from_numpy(faces).to(dev), c=torch.from_numpy(cam).to(dev),
             b=torch.from_numpy(bb).to(dev), fp=torch.from_numpy(fpart).to(dev).to(torch.int32).contiguous(),
             rgb=torch.from_numpy(rgb).to(dev).contiguous(), out=torch.empty((B, H, W, 3), dtype=torch.uint8, device=dev))
    lib = _lib.load()
    V, F = verts.shape[1], faces.shape[0]
    nb = lib.pr_render_workspace_bytes(B, V, F, H, W)
    t["ws"] = torch.empty((nb,), dtype=torch.uint8, device=dev)
    args = _lib.RenderArgs(t["v"].data_ptr(), t["f"].data_ptr(), t["c"].data_ptr(), t["b"].data_ptr(), frames.data_ptr(), None,
                           t["fp"].data_ptr(), t["rgb"].data_ptr(), t["out"].data_ptr(), None, None, None,
                           B, V, F, t["rgb"].shape[1], B, H, W, 0, 1.2, 0.6)
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda: _lib.check(lib.pr_render_overlay(args, t["ws"].data_ptr(), nb, stream), "pr_render_overlay")
    call.keep = (t, args)
    return call, B * H * W * (8 + 8 + 3 + 3)


def time_ms(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_video.py needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    B = a.batch
    compose, frames, nbytes = compose_call(B, 450, 800, dev)
    overlay, overlay_floor = overlay_call(frames, dev)
    compose_hd, _, nbytes_hd = compose_call(B, 1080, 1920, dev, seed=2)
    calls = {"compose_800x450": compose, "overlay_800x450": overlay, "compose_1920x1080": compose_hd}
    for call in calls.values():
        for _ in range(a.warmup):
            call()
    torch.cuda.synchronize()
    rounds = {k: [] for k in calls}
    for _ in range(a.rounds):                                     # alternating: every round times each of them once
        for k, call in calls.items():
            rounds[k].append(time_ms(call, a.iters))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    shape = lambda ms, nb: {"ms_per_batch": round(ms, 4), "frames_per_s": round(B / ms * 1e3, 1), "bytes_per_batch": nb,
                            "traffic_floor_ms": round(nb / HBM_BYTES_PER_S * 1e3, 4),
                            "share_of_floor": round(nb / HBM_BYTES_PER_S * 1e3 / ms, 4)}
    rec = {"batch": B, "iters": a.iters, "rounds": a.rounds,
           "compose_800x450": shape(med["compose_800x450"], nbytes),
           "compose_1920x1080": shape(med["compose_1920x1080"], nbytes_hd),
           "overlay_800x450": shape(med["overlay_800x450"], overlay_floor),
           "compose_over_overlay": round(med["compose_800x450"] / med["overlay_800x450"], 4),
           "compose_no_slower_than_overlay": bool(med["compose_800x450"] <= med["overlay_800x450"]),
           "ms_per_round": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
           "floor_bytes_per_s": HBM_BYTES_PER_S,
           "device": torch.cuda.get_device_name(0), "library": _lib.load().pr_build_info().decode()}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    if not rec["compose_no_slower_than_overlay"]:
        raise SystemExit("pr_compose_video is slower than pr_render_overlay on the same frames")


if __name__ == "__main__":
    main()
