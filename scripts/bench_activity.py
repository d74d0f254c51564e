"""Time the derivation of REBA's activity score and RULA's muscle use from the tracks (pr_activity_tracks, csrc/activity.hip;
INTEGRATION.md 1o).  One JSON line, at 4 tracks of 4 096 rows, 30 fps, the default parameters (H = 1 800) and again with H = 300,
on two kinds of rows: `still` (0.2 degrees of jitter: every window is walked to its end, the worst case) and `moving` (the
smoothing tests' jittery track: most lanes stop early):

(a) the three launches, by device events after a warm-up, against two floors named by reasoning, not by a counter run: the
    float64 vector rate (every dot of every window, 18 flops each, at the spec rate) and the byte floor (the scored joints and
    the frame numbers read once, flags and adds written once, at the HBM streaming rate the other benches use).  Per stage:
    `--trace-run` only repeats the call a dozen times; run it under a kernel trace with statistics and hand the resulting
    kernel_stats.csv back with `--stats-csv`;
(b) tests/activity_ref.py's numpy arithmetic on the still rows on 16 host threads, wall clock -- and that its integers equal
    the GPU's;
(c) Predictor.score_people on bench_smooth.py's four-track clip with the knob off and on, alternating in one process
    (hold_seconds = 1 so that the short clip holds whole windows), the run-to-run spread of the knob-off time, and -- with
    `--parent DIR`, a built checkout of the parent commit -- the knob-off time there, in child processes before and after.

usage: python scripts/bench_activity.py [--tracks 4] [--rows 4096] [--iters 20] [--rounds 7] [--warmup 3] [--parent DIR]
                                        [--stats-csv FILE] [--out profiles/activity.json]
       python scripts/bench_activity.py --trace-run
       python scripts/bench_activity.py --clip-only [--repo DIR]"""
import argparse
import csv
import ctypes as C
import json
import os
import subprocess
import sys
import time
import types

import numpy as np

HERE = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
REPO = os.path.abspath(sys.argv[sys.argv.index("--repo") + 1]) if "--repo" in sys.argv else HERE
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "scripts"))
sys.path.insert(0, os.path.join(REPO, "tests"))

import torch  # noqa: E402

from poserisk_release_amd import _lib, synth  # noqa: E402

FP64_VECTOR_FLOPS = 78.6e12      # the spec rate of the float64 vector pipe
HOST_THREADS = 16
FPS = 30.0
HOLDS = (60.0, 10.0)             # seconds: H = 1 800 and 300 frames
KERNELS = ("events_kernel", "window_kernel", "spread_kernel")


def wall_ms(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def time_ms(call, iters):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(iters):
        call()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / iters


def rows_of(kind, tracks, rows, seed=0):
    import activity_cases
    import smooth_cases
    rng = np.random.default_rng(seed)
    if kind == "still":
        rot = np.concatenate([activity_cases.track(rng, np.zeros(rows)) for _ in range(tracks)])
    else:
        rot = np.concatenate([smooth_cases.jittery_track(rng, np.arange(rows))[0] for _ in range(tracks)])
    return rot, np.tile(np.arange(rows, dtype=np.int32), tracks), np.arange(tracks + 1) * rows


def kernel_call(rot, frame_no, track_start, par, dev):
    """-> (callable that enqueues one pr_activity_tracks on preallocated tensors, flags, adds)."""
    lib = _lib.load()
    N = rot.shape[0]
    t = dict(rot=torch.from_numpy(rot).to(dev), fno=torch.from_numpy(frame_no).to(dev))
    o = dict(flags=torch.empty((N, 4), dtype=torch.int32, device=dev), adds=torch.empty((N, 4), dtype=torch.int32, device=dev),
             ws=torch.empty((lib.pr_activity_workspace_bytes(N),), dtype=torch.uint8, device=dev))
    params = _lib.ActivityParams(par["hold_frames"], par["rapid_frames"], par["gap_frames"], par["rep_events"], par["dot_static"],
                                 par["dot_move"], par["dot_rapid"])
    starts = (C.c_int * len(track_start))(*[int(s) for s in track_start])
    stream = torch.cuda.current_stream(dev).cuda_stream
    call = lambda: _lib.check(lib.pr_activity_tracks(C.byref(params), t["rot"].data_ptr(), t["fno"].data_ptr(), starts, len(track_start) - 1, N,
                                                     o["flags"].data_ptr(), o["adds"].data_ptr(), o["ws"].data_ptr(), stream), "pr_activity_tracks")
    call.keep = (t, o, params, starts)
    return call, o["flags"], o["adds"]


def window_dots(track_start, H):
    """The (row, member) pairs of every window W_i(H) on consecutive frame numbers: what a kernel without early exit computes."""
    return int(sum(int(np.minimum(np.arange(b - a), H).sum()) + (b - a) for a, b in zip(track_start[:-1], track_start[1:])))


def score_clip(dev, batch_size, rounds, knob=True):
    """(c): bench_smooth.py's clip -> ms of score_people per round with the knob off and (where this tree has the knob) on."""
    from poserisk_release_amd import dropin
    dropin.install()
    from core import base
    from core.config import cfg
    from models import hmr
    from smpl import SMPL
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=dev)
    make = lambda **knobs: base.Predictor(types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1, **knobs),
                                          spin_model=model, smpl_model=smpl, batch_size=batch_size)
    rng = np.random.default_rng(3)
    frames = torch.from_numpy(rng.integers(0, 256, (96, 240, 320, 3), dtype=np.uint8)).to(dev)
    tr = {}
    for pid, (first, n, w) in enumerate([(0, 96, 90), (10, 70, 70), (30, 45, 50), (60, 35, 30)]):
        tr[pid] = {'bbox': np.stack([np.array([60 + 60 * pid + i % 7, 120, w, 2 * w], np.float32) for i in range(n)]),
                   'frames': np.arange(first, first + n)}
    off = make()
    run = {"off": lambda: off.score_people(frames, tr, synth.EXAMPLE_INFO)}
    if knob and "ACTIVITY" in cfg:
        cfg.ACTIVITY.update(hold_seconds=1.0)
        on = make(derive_activity=True)
        run["on"] = lambda: on.score_people(frames, tr, synth.EXAMPLE_INFO, fps=FPS)
    for fn in run.values():
        fn()                                                      # warm-up: the plan, the pipeline's lanes, the pinned buffers
    ms = {k: [] for k in run}
    for _ in range(rounds):                                       # alternating
        for k, fn in run.items():
            ms[k].append(wall_ms(fn))
    return ms


def clip_child(repo, rounds):
    """score_clip's knob-off times in a fresh process on the tree at `repo` (this one, or a built checkout of the parent)."""
    r = subprocess.run([sys.executable, os.path.abspath(__file__), "--clip-only", "--rounds", str(rounds), "--repo", repo], capture_output=True,
                       text=True, timeout=900)
    if r.returncode != 0:
        raise RuntimeError(f"the clip run on {repo} failed:\n{r.stdout[-2000:]}\n{r.stderr[-4000:]}")
    return json.loads(r.stdout.strip().splitlines()[-1])["off"]


def stage_stats(path):
    """A kernel trace's kernel_stats.csv -> {kernel: mean microseconds} for the three stages."""
    out = {}
    with open(path, newline="") as f:
        for row in csv.DictReader(f):
            for k in KERNELS:
                if k in row.get("Name", ""):
                    out[k] = {"calls": int(row["Calls"]), "mean_us": round(float(row["AverageNs"]) / 1e3, 3), "share_percent": float(row["Percentage"])}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--tracks", type=int, default=4)
    ap.add_argument("--rows", type=int, default=4096)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--parent", default=None)
    ap.add_argument("--repo", default=None)
    ap.add_argument("--stats-csv", default=None)
    ap.add_argument("--trace-run", action="store_true")
    ap.add_argument("--clip-only", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_activity.py needs the GPU (there is no CPU path to time)")
    dev = torch.device("cuda", 0)
    if a.clip_only:
        print(json.dumps(score_clip(dev, 64, a.rounds, knob=False)))
        return
    import activity_ref
    import bench_video
    from poserisk_release_amd import activity
    if a.trace_run:                                               # a dozen calls of the worst case and nothing else
        rot, frame_no, track_start = rows_of("still", a.tracks, a.rows)
        call, _, _ = kernel_call(rot, frame_no, track_start, activity.check_parameters(FPS), dev)
        for _ in range(12):
            call()
        torch.cuda.synchronize()
        return
    lib = _lib.load()
    N = a.tracks * a.rows
    floor_bytes = N * (12 * 36 + 4) + N * 32                      # the scored joints and frame_no in; flags and adds out
    rec = {"tracks": a.tracks, "rows_per_track": a.rows, "rows": N, "fps": FPS, "iters": a.iters, "rounds": a.rounds,
           "tile_rows": lib.pr_activity_tile_rows(), "chunk_rows": lib.pr_activity_chunk_rows(), "floor_bytes": floor_bytes,
           "floor_bytes_per_s": bench_video.HBM_BYTES_PER_S, "byte_floor_ms": round(floor_bytes / bench_video.HBM_BYTES_PER_S * 1e3, 5),
           "fp64_vector_flops_per_s": FP64_VECTOR_FLOPS, "bounds": "both named by reasoning (spec rates and counted work), neither by a counter run"}
    for hold in HOLDS:
        par = activity.check_parameters(FPS, hold_seconds=hold)
        H = par["hold_frames"]
        entry = {"hold_frames": H, "rapid_frames": par["rapid_frames"], "gap_frames": par["gap_frames"]}
        for kind in ("still", "moving"):
            rot, frame_no, track_start = rows_of(kind, a.tracks, a.rows)
            call, flags, adds = kernel_call(rot, frame_no, track_start, par, dev)
            for _ in range(a.warmup):
                call()
            torch.cuda.synchronize()
            per_round = [time_ms(call, a.iters) for _ in range(a.rounds)]
            ms = float(np.median(per_round))
            flops = window_dots(track_start, H) * 12 * 18
            e = {"three_launches_ms": round(ms, 5), "three_launches_ms_per_round": [round(x, 5) for x in per_round], "rows_per_s": round(N / ms * 1e3, 1),
                 "window_flops_without_early_exit": flops, "fp64_floor_ms": round(flops / FP64_VECTOR_FLOPS * 1e3, 5),
                 "share_of_fp64_vector_rate": round(flops / FP64_VECTOR_FLOPS * 1e3 / ms, 5),
                 "share_of_byte_floor": round(floor_bytes / bench_video.HBM_BYTES_PER_S * 1e3 / ms, 5),
                 "rows_flagged": {k: int(v) for k, v in zip(activity.KINDS, (flags != 0).sum(0).tolist())}}
            if kind == "still":                                   # (b)
                t0 = time.perf_counter()
                ref = activity_ref.activity(rot, frame_no, track_start, H, par["rapid_frames"], par["gap_frames"], par["rep_events"],
                                            par["dot_static"], par["dot_move"], par["dot_rapid"], threads=HOST_THREADS)
                host_ms = (time.perf_counter() - t0) * 1e3
                e.update(numpy_16_threads_ms=round(host_ms, 1), gpu_beats_numpy=bool(ms < host_ms),
                         equal_to_numpy=bool(np.array_equal(flags.cpu().numpy(), ref["flags"]) and np.array_equal(adds.cpu().numpy(), ref["adds"])))
            entry[kind] = e
        rec[f"hold_{hold:g}s"] = entry
    if a.stats_csv:
        rec["per_stage_still_default"] = stage_stats(a.stats_csv)
    ms = score_clip(dev, 64, a.rounds)
    if a.parent:                                                  # parent, this tree, parent: each in a fresh process
        before, mine, after = clip_child(a.parent, a.rounds), clip_child(HERE, a.rounds), clip_child(a.parent, a.rounds)
    off, on = float(np.median(ms["off"])), float(np.median(ms["on"]))
    spread = (max(ms["off"]) - min(ms["off"])) / off
    rec["score_people"] = {"track_rows": [96, 70, 45, 35], "hold_seconds": 1.0, "knob_off_ms": round(off, 3), "knob_on_ms": round(on, 3),
                           "added_share": round((on - off) / off, 5), "knob_off_spread": round(spread, 5),
                           "ms_per_round": {k: [round(x, 3) for x in v] for k, v in ms.items()}}
    if a.parent:
        p, m = float(np.median(before + after)), float(np.median(mine))
        child_spread = max((max(x) - min(x)) / np.median(x) for x in (before, mine, after))
        rec["score_people"].update(parent_knob_off_ms=round(p, 3), this_tree_knob_off_ms_in_a_child=round(m, 3),
                                   child_ms_per_round={"parent_before": [round(x, 3) for x in before], "this_tree": [round(x, 3) for x in mine],
                                                       "parent_after": [round(x, 3) for x in after]},
                                   knob_off_against_parent=round((m - p) / p, 5), child_spread=round(float(child_spread), 5),
                                   beyond_spread=bool(abs(m - p) / p > child_spread))
    rec.update(device=torch.cuda.get_device_name(0), library=lib.pr_build_info().decode())
    line = json.dumps(rec)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
