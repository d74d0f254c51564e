"""Time scoring every tracked person.  Two measurements, one JSON line:

(a) the people compositor (pr_compose_people, csrc/compose.hip): 64 canvases of 800x450 with K = 1, 4 and 16 people a
    frame (boxes, tags and a people panel from video.people_draw_list), against pr_compose_video on the same frames
    (scripts/bench_video.py's call) in the same process, alternating round by round -- and, as `compose_people_as_video`,
    pr_compose_video's own box and nine-line panel through pr_compose_people (K = 1, L_img = 0): the same bytes out.  That
    pair runs at bench_video.py's second shape, 1920x1080, too (`compose_video_1920x1080`,
    `compose_people_as_video_1920x1080`).  While the two entries had a kernel each, this pair was the gate for serving both
    from one (profiles/compose_one_kernel.json); now that they share it, it shows that a colour in the parameter block costs
    what a colour table does.  The K = 1 people canvas itself has less text than the score panel.  Per variant: ms per
    batch, frames/s, the bytes moved computed from the shapes and the share of the HBM streaming floor reached, as DESIGN.md
    3.8 computes it.
(b) Predictor.score_people on a synthetic clip with 4 tracks of unequal length (synthetic weights), against the sum of 4
    Predictor.score_frames runs on single-track dicts: wall-clock ms, synchronised, median of the rounds.

usage: python scripts/bench_people.py [--batch 64] [--iters 200] [--rounds 7] [--warmup 5] [--out profiles/people.json]"""
import argparse
import json
import os
import sys
import time
import types

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))

from poserisk_release_amd import _lib, synth, video  # noqa: E402
import bench_video  # noqa: E402

HBM_BYTES_PER_S = bench_video.HBM_BYTES_PER_S
NAMES = ("Negligible risk", "Low risk. Change may be needed.", "Medium risk. Further Investigate. Change Soon.",
         "High risk. Investigate and implement change", "Very high risk. Implement change")


def people_call(B, H, W, K, frames, dev, seed=0):
    """-> (callable that enqueues one pr_compose_people of B canvases with K people in every frame, bytes moved per call)."""
    rng = np.random.default_rng(seed + K)
    dst_h, dst_w, panel_w = video.canvas_size(H, W)
    people = []
    for k in range(K):
        h = rng.uniform(0.3, 0.9, B) * H
        boxes = np.stack([rng.uniform(0.1, 0.9, B) * W, rng.uniform(0.4, 0.6, B) * H, h * 0.5, h], 1).astype(np.float32)
        levels = rng.integers(1, 6, B)
        people.append(dict(id=k + 1, frames=np.arange(B), bboxes=boxes, scores=rng.integers(1, 13, B), levels=levels,
                           names=[NAMES[l - 1] for l in levels]))
    draw = video.people_draw_list("REBA", B, people, dst_h, dst_w, H, W)
    lines, codes, L_img = video.pack_people(draw, 0, B)
    atlas = video.font_atlas()
    t = dict(box=torch.from_numpy(draw.box).to(dev), rgb=torch.from_numpy(draw.box_rgb).to(dev), lines=torch.from_numpy(lines).to(dev),
             text=torch.from_numpy(codes).to(dev), cov=torch.from_numpy(np.array(atlas.cov)).to(dev),
             out=torch.empty((B, dst_h, dst_w + panel_w, 3), dtype=torch.uint8, device=dev))
    args = _lib.ComposePeopleArgs(frames.data_ptr(), None, t["box"].data_ptr(), t["rgb"].data_ptr(), t["lines"].data_ptr(),
                                  t["text"].data_ptr(), t["cov"].data_ptr(), t["out"].data_ptr(), None, B, B, H, W, dst_h, dst_w, panel_w,
                                  K, lines.shape[1], L_img, codes.shape[2], 3, video.CELL_H, video.CELL_W)
    args.adv[:3], args.ascent[:3] = atlas.adv, atlas.ascent
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda: _lib.check(lib.pr_compose_people(args, stream), "pr_compose_people")
    call.keep = (t, args)                                         # the tensors the argument struct points into
    return call, B * 3 * (H * W + dst_h * (dst_w + panel_w))


def reduction_call(single, frames, dev):
    """pr_compose_video's own workload (bench_video.compose_call's box, nine-line panel and colour) through pr_compose_people
    with K = 1 and L_img = 0 -> (callable, whether the two kernels' canvases are equal byte for byte)."""
    t, a = single.keep
    B = a.N
    rgb = torch.tensor(list(video.GREEN) + [0], dtype=torch.uint8, device=dev).repeat(B, 1, 1).contiguous()
    out = torch.empty_like(t["out"])
    args = _lib.ComposePeopleArgs(frames.data_ptr(), None, t["box"].data_ptr(), rgb.data_ptr(), t["lines"].data_ptr(), t["text"].data_ptr(),
                                  t["cov"].data_ptr(), out.data_ptr(), None, B, B, a.H, a.W, a.dst_h, a.dst_w, a.panel_w, 1, a.L, 0, a.C,
                                  a.S, a.CH, a.CW)
    args.adv[:], args.ascent[:] = a.adv[:], a.ascent[:]
    lib = _lib.load()
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda: _lib.check(lib.pr_compose_people(args, stream), "pr_compose_people")
    call.keep = (rgb, out, args)
    single(), call()
    torch.cuda.synchronize()
    return call, bool(torch.equal(out, t["out"]))


def score_clip(dev, batch_size, rounds):
    """(b): 96 frames of 320x240, tracks of 96, 70, 45 and 35 frames (each above the 0.33 * 96 frames filter_tracks asks for) -> (ms of score_people, ms of 4 score_frames, launches)."""
    from poserisk_release_amd import dropin
    dropin.install()
    from core import base
    from models import hmr
    from smpl import SMPL
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=dev)
    args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1)
    pred = base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=batch_size)
    rng = np.random.default_rng(3)
    F = 96
    frames = torch.from_numpy(rng.integers(0, 256, (F, 240, 320, 3), dtype=np.uint8)).to(dev)
    tr = {}
    for pid, (first, n, w) in enumerate([(0, 96, 90), (10, 70, 70), (30, 45, 50), (60, 35, 30)]):
        tr[pid] = {'bbox': np.stack([np.array([60 + 60 * pid + i % 7, 120, w, 2 * w], np.float32) for i in range(n)]),
                   'frames': np.arange(first, first + n)}
    singles = [{pid: t} for pid, t in tr.items()]

    def timed(fn):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3
    together = lambda: pred.score_people(frames, tr, synth.EXAMPLE_INFO)
    apart = lambda: [pred.score_frames(frames, s, synth.EXAMPLE_INFO) for s in singles]
    together(), apart()                                           # warm-up: the plan, the pipeline's lanes, the pinned buffers
    ms = {"score_people": [], "score_frames_x4": []}
    for _ in range(rounds):
        ms["score_people"].append(timed(together))
        ms["score_frames_x4"].append(timed(apart))
    rows = [len(t['frames']) for t in tr.values()]
    assert len(together()["ids"]) == len(rows)
    launches = {"score_people": -(-sum(rows) // batch_size), "score_frames_x4": sum(-(-n // batch_size) for n in rows)}
    return ms, launches, rows


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=64)
    ap.add_argument("--iters", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_people.py needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    B, H, W = a.batch, 450, 800
    single, frames, nbytes = bench_video.compose_call(B, H, W, dev)
    calls = {"compose_video": single}
    calls["compose_people_as_video"], same_bytes = reduction_call(single, frames, dev)
    for K in (1, 4, 16):
        calls[f"compose_people_K{K}"], _ = people_call(B, H, W, K, frames, dev)
    single_hd, frames_hd, nbytes_hd = bench_video.compose_call(B, 1080, 1920, dev, seed=2)
    calls["compose_video_1920x1080"] = single_hd
    calls["compose_people_as_video_1920x1080"], same_bytes_hd = reduction_call(single_hd, frames_hd, dev)
    for call in calls.values():
        for _ in range(a.warmup):
            call()
    torch.cuda.synchronize()
    rounds = {k: [] for k in calls}
    for _ in range(a.rounds):                                     # alternating: every round times each of them once
        for k, call in calls.items():
            rounds[k].append(bench_video.time_ms(call, a.iters))
    med = {k: float(np.median(v)) for k, v in rounds.items()}
    def shape(k):
        hd = k.endswith("_1920x1080")
        ms, nb, base = med[k], nbytes_hd if hd else nbytes, med["compose_video_1920x1080" if hd else "compose_video"]
        return {"ms_per_batch": round(ms, 4), "frames_per_s": round(B / ms * 1e3, 1), "bytes_per_batch": nb,
                "traffic_floor_ms": round(nb / HBM_BYTES_PER_S * 1e3, 4), "share_of_floor": round(nb / HBM_BYTES_PER_S * 1e3 / ms, 4),
                "over_compose_video": round(ms / base, 4)}
    # the people kernel serves pr_compose_video's workload when its median is within pr_compose_video's own spread of rounds
    gate = {s: bool(med["compose_people_as_video" + s] <= med["compose_video" + s] + max(rounds["compose_video" + s])
                    - min(rounds["compose_video" + s])) for s in ("", "_1920x1080")}
    ms, launches, rows = score_clip(dev, a.batch, a.rounds)
    smed = {k: float(np.median(v)) for k, v in ms.items()}
    rec = {"batch": B, "iters": a.iters, "rounds": a.rounds, "frame": [H, W],
           **{k: shape(k) for k in med},
           "as_video_bytes_equal": same_bytes, "as_video_bytes_equal_1920x1080": same_bytes_hd,
           "as_video_within_compose_video_spread": {"800x450": gate[""], "1920x1080": gate["_1920x1080"]},
           "as_video_within_10_percent_of_compose_video": bool(med["compose_people_as_video"] <= 1.10 * med["compose_video"]),
           "ms_per_round": {k: [round(x, 4) for x in v] for k, v in rounds.items()},
           "score": {"track_rows": rows, "batch_size": a.batch, "pipeline_launches": launches,
                     "score_people_ms": round(smed["score_people"], 3), "score_frames_x4_ms": round(smed["score_frames_x4"], 3),
                     "people_over_x4": round(smed["score_people"] / smed["score_frames_x4"], 4),
                     "ms_per_round": {k: [round(x, 3) for x in v] for k, v in ms.items()}},
           "floor_bytes_per_s": HBM_BYTES_PER_S,
           "device": torch.cuda.get_device_name(0), "library": _lib.load().pr_build_info().decode()}
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
