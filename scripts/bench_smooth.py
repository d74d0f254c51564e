"""Time the temporal smoothing of tracks (pr_smooth_tracks, csrc/smooth.hip).  Four measurements, one
JSON line, at (median_radius, sigma) = (2, 1.5) and (15, 5) on 4 tracks of 2 048 rows:

(a) the two launches alone, by device events after a warm-up, against the byte floor -- every input read once, every output
    written once -- at the HBM streaming rate the other benches use;
(b) smooth.smooth_tracks plus the back half run again from the smoothed rotations (ops.pose_to_euler, the SMPL layer's
    joint_cam in chunks), wall clock, synchronised;
(c) Predictor.score_people on 4 tracks of 96 / 70 / 45 / 35 frames (synthetic weights, bench_people.py's clip) with the
    knobs off and on, alternating in one process: the added share against the knobs-off time of the same run;
(d) tests/smooth_ref.py's numpy arithmetic on the same rows on 16 host threads (every track cut into pieces with the 30 rows
    of halo the two stages reach, so the rows' values are those of the whole track), wall clock -- and the largest
    difference between its rotations and the GPU's.

usage: python scripts/bench_smooth.py [--tracks 4] [--rows 2048] [--iters 50] [--rounds 7] [--warmup 5] [--out profiles/smooth.json]"""
import argparse
import ctypes as C
import json
import os
import sys
import time
import types
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))
sys.path.insert(0, os.path.join(REPO, "tests"))

from poserisk_release_amd import _lib, ops, smooth, synth  # noqa: E402
import bench_video  # noqa: E402
import smooth_cases  # noqa: E402
import smooth_ref  # noqa: E402

HBM_BYTES_PER_S = bench_video.HBM_BYTES_PER_S
PAIRS = ((2, 1.5), (15, 5.0))
HOST_THREADS = 16


def jittery_rows(tracks, rows, seed=0):
    """`tracks` tracks of `rows` consecutive frames each: the tests' slowly moving pose with 0.03 rad of jitter per frame."""
    rng = np.random.default_rng(seed)
    rot, betas, cam = (np.concatenate(x) for x in zip(*[smooth_cases.jittery_track(rng, np.arange(rows)) for _ in range(tracks)]))
    return rot, betas, cam, np.tile(np.arange(rows, dtype=np.int32), tracks), np.arange(tracks + 1) * rows


def kernel_call(rot, betas, cam, frame_no, track_start, m, sigma, dev):
    """-> (callable that enqueues one pr_smooth_tracks on preallocated tensors, the output rotmat tensor)."""
    lib = _lib.load()
    N = rot.shape[0]
    t = dict(rot=torch.from_numpy(rot).to(dev), betas=torch.from_numpy(betas).to(dev), cam=torch.from_numpy(cam).to(dev),
             fno=torch.from_numpy(frame_no).to(dev))
    o = dict(rot=torch.empty_like(t["rot"]), betas=torch.empty_like(t["betas"]), cam=torch.empty_like(t["cam"]),
             status=torch.empty((N,), dtype=torch.int32, device=dev), replaced=torch.empty((N,), dtype=torch.int32, device=dev),
             ws=torch.empty((lib.pr_smooth_workspace_bytes(N, 1, 1),), dtype=torch.uint8, device=dev))
    params = _lib.SmoothParams(m, 0, sigma)
    ins = _lib.SmoothInputs(t["rot"].data_ptr(), t["betas"].data_ptr(), t["cam"].data_ptr())
    outs = _lib.SmoothOutputs(o["rot"].data_ptr(), o["betas"].data_ptr(), o["cam"].data_ptr(), o["replaced"].data_ptr())
    starts = (C.c_int * len(track_start))(*[int(s) for s in track_start])
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda: _lib.check(lib.pr_smooth_tracks(C.byref(params), C.byref(ins), t["fno"].data_ptr(), starts, len(track_start) - 1, N,
                                                   C.byref(outs), o["status"].data_ptr(), o["ws"].data_ptr(), stream), "pr_smooth_tracks")
    call.keep = (t, o, params, ins, outs, starts)
    return call, o["rot"]


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def host_reference(rot, betas, cam, frame_no, track_start, m, sigma):
    """(d): -> (ms, rotmat f64[N,24,3,3]) on HOST_THREADS threads."""
    halo = 2 * smooth_ref.MAX_RADIUS
    jobs = []
    per_track = max(1, HOST_THREADS // max(len(track_start) - 1, 1))
    for a, b in zip(track_start[:-1], track_start[1:]):
        cuts = np.linspace(a, b, per_track + 1).astype(int)
        for p0, p1 in zip(cuts[:-1], cuts[1:]):
            if p1 > p0:
                jobs.append((max(a, p0 - halo), min(b, p1 + halo), p0, p1))

    def piece(job):
        lo, hi, p0, p1 = job
        r = smooth_ref.smooth(rot[lo:hi], frame_no[lo:hi], [0, hi - lo], m, sigma, betas=betas[lo:hi], cam=cam[lo:hi])
        return p0, p1, np.asarray(r["rotmat"], np.float64)[p0 - lo:p1 - lo]
    t0 = time.perf_counter()
    with ThreadPoolExecutor(max_workers=HOST_THREADS) as ex:
        parts = list(ex.map(piece, jobs))
    ms = (time.perf_counter() - t0) * 1e3
    out = np.empty(rot.shape, np.float64)
    for p0, p1, r in parts:
        out[p0:p1] = r
    return ms, out


def score_clip(dev, batch_size, rounds, m, sigma):
    """(c): bench_people.py's clip -> (ms of score_people per round with the knobs off, with them on)."""
    from poserisk_release_amd import dropin
    dropin.install()
    from core import base
    from models import hmr
    from smpl import SMPL
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=dev)
    make = lambda **knobs: base.Predictor(types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1, **knobs),
                                          spin_model=model, smpl_model=smpl, batch_size=batch_size)
    off, on = make(), make(smooth_median_radius=m, smooth_sigma=sigma)
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.integers(0, 256, (96, 240, 320, 3), dtype=np.uint8)).to(dev)
    tr = {}
    for pid, (first, n, w) in enumerate([(0, 96, 90), (10, 70, 70), (30, 45, 50), (60, 35, 30)]):
        tr[pid] = {'bbox': np.stack([np.array([60 + 60 * pid + i % 7, 120, w, 2 * w], np.float32) for i in range(n)]),
                   'frames': np.arange(first, first + n)}
    run = {"off": lambda: off.score_people(frames, tr, synth.EXAMPLE_INFO), "on": lambda: on.score_people(frames, tr, synth.EXAMPLE_INFO)}
    for fn in run.values():
        fn()                                                      # warm-up: the plan, the pipeline's lanes, the pinned buffers
    ms = {k: [] for k in run}
    for _ in range(rounds):                                       # alternating
        for k, fn in run.items():
            ms[k].append(wall_ms(fn))
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=4)
    ap.add_argument("--rows", type=int, default=2048)
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_smooth.py needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    rot, betas, cam, frame_no, track_start = jittery_rows(a.tracks, a.rows)
    N = rot.shape[0]
    floor_bytes = N * (229 * 4 + 4) + N * (229 * 4 + 8)           # rotmat, cam, betas, frame_no in; the three, status, replaced out
    from poserisk_release_amd.smpl_layer import SMPLLayer
    layer = SMPLLayer(synth.smpl_model(V=6890, seed=2), device=dev, max_batch=256)
    rec = {"tracks": a.tracks, "rows_per_track": a.rows, "rows": N, "iters": a.iters, "rounds": a.rounds, "tile_rows": _lib.load().pr_smooth_tile_rows(),
           "floor_bytes": floor_bytes, "floor_bytes_per_s": HBM_BYTES_PER_S, "floor_ms": round(floor_bytes / HBM_BYTES_PER_S * 1e3, 5)}
    d_rot, d_betas, d_cam = (torch.from_numpy(x).to(dev) for x in (rot, betas, cam))
    for m, sigma in PAIRS:
        call, out_rot = kernel_call(rot, betas, cam, frame_no, track_start, m, sigma, dev)
        for _ in range(a.warmup):
            call()
        torch.cuda.synchronize()
        kernel = [bench_video.time_ms(call, a.iters) for _ in range(a.rounds)]

        def whole():
            sm = smooth.smooth_tracks(d_rot, frame_no, track_start, m, sigma, betas=d_betas, cam=d_cam)
            aa, eul, st = ops.pose_to_euler(sm["rotmat"])
            jc = torch.empty((N, 24, 3), dtype=torch.float32, device=dev)
            for lo in range(0, N, 256):
                layer.joint_cam(aa[lo:lo + 256], out=jc[lo:lo + 256])
            return eul, jc
        for _ in range(2):
            whole()
        back = [wall_ms(whole) for _ in range(a.rounds)]
        host_ms, host_rot = host_reference(rot, betas, cam, frame_no, track_start, m, sigma)
        k_ms, b_ms = float(np.median(kernel)), float(np.median(back))
        rec[f"m{m}_sigma{sigma:g}"] = {
            "two_launches_ms": round(k_ms, 5), "share_of_floor": round(floor_bytes / HBM_BYTES_PER_S * 1e3 / k_ms, 5),
            "rows_per_s": round(N / k_ms * 1e3, 1), "two_launches_ms_per_round": [round(x, 5) for x in kernel],
            "smooth_plus_back_half_ms": round(b_ms, 4), "smooth_plus_back_half_ms_per_round": [round(x, 4) for x in back],
            "numpy_16_threads_ms": round(host_ms, 2), "back_half_loses_to_numpy": bool(b_ms > host_ms),
            "max_abs_rotation_difference_to_numpy": float(np.abs(out_rot.cpu().numpy().astype(np.float64) - host_rot).max())}
    m, sigma = PAIRS[0]
    ms = score_clip(dev, 64, a.rounds, m, sigma)
    off, on = float(np.median(ms["off"])), float(np.median(ms["on"]))
    rec["score_people"] = {"track_rows": [96, 70, 45, 35], "median_radius": m, "sigma": sigma, "knobs_off_ms": round(off, 3), "knobs_on_ms": round(on, 3),
                           "added_share": round((on - off) / off, 5), "ms_per_round": {k: [round(x, 3) for x in v] for k, v in ms.items()}}
    rec.update(device=torch.cuda.get_device_name(0), library=_lib.load().pr_build_info().decode())
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
