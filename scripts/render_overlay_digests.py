"""SHA-256 digests of everything pr_render_overlay writes (out, face_id, vert_fx, status) on a fixed set of seeded scenes:
the pin under tests/test_render_gpu.py::test_bytes_are_those_of_the_recorded_build.  The committed file,
tests/render_overlay_digests.json, is written by the build BEFORE a change to the rasteriser and compared on the build after
it; the file records which commit and toolchain it came from.

The scenes are tests/people_mesh_cases.py's soup, grid and spanning (so the big-face queue is used) at 37 x 53 with N = 7,
bgr, alpha 0.35, and at 96 x 128 with N = 5, alpha 1; each holds one NaN vertex, one frame_idx out of range and a permuted
frame_idx with a repeat.

usage: python scripts/render_overlay_digests.py --commit <the commit the library was built from> [--out tests/render_overlay_digests.json]"""
import argparse
import hashlib
import json
import os
import sys

import numpy as np

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, REPO)
sys.path.insert(0, os.path.join(REPO, "tests"))

DIGESTS = os.path.join(REPO, "tests", "render_overlay_digests.json")
SHAPES = ((37, 53, 7, True, 0.35), (96, 128, 5, False, 1.0))          # H, W, N, bgr, alpha
BUILDERS = ("soup", "grid", "spanning")
P = 5


def cases():
    """-> [(name, keyword arguments of render.overlay without the frames, frames u8[n_frames,H,W,3])]"""
    import people_mesh_cases as pmc
    made = []
    for H, W, N, bgr, alpha in SHAPES:
        for k, builder in enumerate(BUILDERS):
            sc = getattr(pmc, builder)(N, H, W, seed=11 * H + k)
            rng = np.random.default_rng(H + k)
            sc["verts"][N // 2, 1] = np.nan                            # one invalid vertex
            n_frames = N - 2
            fidx = np.concatenate([rng.permutation(n_frames), [1, n_frames + 3]]).astype(np.int32)   # a repeat, and no such frame
            fidx = fidx[rng.permutation(N)]
            kw = dict(verts=sc["verts"], faces=sc["faces"], cam=sc["cam"], bboxes=sc["bboxes"], scale=pmc.SCALE, frame_idx=fidx,
                      face_part=np.arange(len(sc["faces"]), dtype=np.int32) % P, part_rgb=pmc.part_table(N, P, seed=H + k),
                      alpha=alpha, bgr=bgr)
            made.append((f"{builder}_{H}x{W}_N{N}", kw, pmc.frames(n_frames, H, W, seed=k)))
    return made


def digests(device="cuda"):
    """-> {case: {out, face_id, vert_fx, status: sha256 of the array's bytes (C order, little endian)}} on the loaded build."""
    import torch
    from poserisk_release_amd import render
    got = {}
    for name, kw, frames in cases():
        arrays = render.overlay(torch.from_numpy(frames).to(device), return_face_id=True, return_vert_fx=True, return_status=True, **kw)
        got[name] = {what: hashlib.sha256(np.ascontiguousarray(t.cpu().numpy()).tobytes()).hexdigest()
                     for what, t in zip(("out", "face_id", "vert_fx", "status"), arrays)}
    return got


def main():
    import torch
    from poserisk_release_amd import _lib
    ap = argparse.ArgumentParser()
    ap.add_argument("--commit", required=True, help="the commit the loaded library was built from")
    ap.add_argument("--out", default=DIGESTS)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("render_overlay_digests.py needs the GPU (there is no CPU path to digest)")
    rec = {"commit": a.commit, "library": _lib.load().pr_build_info().decode(), "hip": torch.version.hip, "torch": torch.__version__,
           "device": torch.cuda.get_device_name(0), "digests": digests()}
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1, sort_keys=True)
        f.write("\n")
    print(json.dumps(rec["digests"]))


if __name__ == "__main__":
    main()
