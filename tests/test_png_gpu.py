"""The PNG decoder on the GPU: every case of tests/png_cases.py byte for byte in RGB and BGR, a mixed batch of more frames than
one workgroup has waves, the 800 x 450 frames, six bad files beside good ones, the entry between guard bands, and the Predictor on
a folder of PNG frames.  No test provokes a fault: the bad files are inputs section j4 defines an answer for, and
tests/test_png_native.py has run the same bytes through the same decoding text on the host under sanitizers."""
import ctypes as C
import hashlib
import json
import os
import pickle

import numpy as np
import pytest
import torch

import guard_band as gb
import png_cases as pc
import png_ref as ref
from poserisk_release_amd import _lib, dropin, png, synth

dropin.install()
from core import base  # noqa: E402
from models import hmr  # noqa: E402
from smpl import SMPL  # noqa: E402

pytestmark = pytest.mark.gpu


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} bytes differ, first (frame, row, col, channel) {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


@pytest.mark.parametrize("size", pc.SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_every_small_case_is_byte_exact_in_rgb_and_bgr(gpu_device, size):
    cases = pc.by_size()[size]
    assert len(cases) >= 11
    W, H = size
    for bgr in (False, True):
        frames, status = png.decode_files([s for _, s, _ in cases], gpu_device, bgr=bgr)      # one call per size
        assert tuple(frames.shape) == (len(cases), H, W, 3) and frames.dtype == torch.uint8 and frames.is_cuda
        assert status.cpu().tolist() == [0] * len(cases), [(n, s) for (n, _, _), s in zip(cases, status.cpu().tolist()) if s]
        want = np.stack([px[..., ::-1] if bgr else px for _, _, px in cases])
        got = frames.cpu().numpy()
        assert np.array_equal(got, want), f"{W}x{H} bgr={bgr} {[n for n, _, _ in cases]}: " + _first_difference(got, want)


def test_a_mixed_batch_of_70_frames_equals_the_single_frame_decodes(gpu_device):
    """70 frames of 160 x 90 -- more than the four waves of one inflate workgroup, every stream kind and colour type, in seeded
    order -- in one call."""
    cases = pc.by_size()[(160, 90)]
    order = np.random.default_rng(70).integers(0, len(cases), 70)
    order[:len(cases)] = np.random.default_rng(71).permutation(len(cases))   # every case at least once
    frames, status = png.decode_files([cases[i][1] for i in order], gpu_device, chunk=70)
    assert status.cpu().tolist() == [0] * 70
    got = frames.cpu().numpy()
    single = {}
    for pos, i in enumerate(order):
        if i not in single:
            one, st = png.decode_files([cases[i][1]], gpu_device)
            assert st.cpu().tolist() == [0], cases[i][0]
            single[i] = one.cpu().numpy()[0]
            assert np.array_equal(single[i], cases[i][2]), cases[i][0]
        assert np.array_equal(got[pos], single[i]), f"position {pos} ({cases[i][0]}): " + _first_difference(got[pos][None], single[i][None])


def test_eight_frames_of_800x450_match_at_every_position(gpu_device):
    large = pc.large_frames()
    order = [0, 1, 2, 2, 0, 1, 1, 0]
    frames, status = png.decode_files([large[i][1] for i in order], gpu_device, chunk=8)
    assert tuple(frames.shape) == (8, 450, 800, 3) and status.cpu().tolist() == [0] * 8
    got = frames.cpu().numpy()
    spos = np.random.default_rng(5).integers(0, 450 * 800 * 3, 4096)
    for pos, i in enumerate(order):
        name, _, want = large[i]
        flat = got[pos].reshape(-1)
        if hashlib.sha256(flat.tobytes()).hexdigest() != hashlib.sha256(want.tobytes()).hexdigest():
            off = np.nonzero(flat[spos] != want.reshape(-1)[spos])[0]
            where = [(int(spos[o]) // 2400, int(spos[o]) % 2400 // 3, int(spos[o]) % 3, int(flat[spos[o]]), int(want.reshape(-1)[spos[o]]))
                     for o in off[:5]]
            pytest.fail(f"position {pos} ({name}): SHA-256 differs; {len(off)} of 4096 samples differ, (row, col, channel, got, want) "
                        f"{where}; " + _first_difference(got[pos][None], want[None]))


def test_bad_files_in_a_good_batch_get_their_status_bit_and_touch_nothing_else(gpu_device):
    """One file for each status bit (tests/png_cases.py::gpu_bad_files: among them a distance before the start of the output and
    an output that would overrun), each between good frames, decoded once into the middle of a pre-filled tensor."""
    good = [(s, px) for n, s, px in pc.by_size()[(160, 90)]]
    bad = pc.gpu_bad_files()
    assert [b for _, _, b in bad] == [1, 2, 4, 8, 16, 32]
    batch, want = [], []
    for k in range(18):
        if k % 3 == 1:
            batch.append(bad[k // 3][1])
            want.append(bad[k // 3][2])
        else:
            s, px = good[(k - k // 3) % len(good)]
            batch.append(s)
            want.append(px)
    guard = torch.full((20, 90, 160, 3), 0x5A, dtype=torch.uint8, device=gpu_device)
    frames, status = png.decode_files(batch, gpu_device, out=guard[1:19])
    torch.cuda.synchronize()
    st, got = status.cpu().tolist(), frames.cpu().numpy()
    for k, w in enumerate(want):
        if isinstance(w, int):
            assert st[k] == w, f"bad file at position {k} ({bad[k // 3][0]}): status {st[k]}, expected {w}"
            if w <= 8:
                assert not got[k].any(), f"{bad[k // 3][0]}: a refused or undecodable frame has zero pixels"
            else:                                                           # FILTER or CHECKSUM alone: the pixels its bytes give
                px = ref.decode(bad[k // 3][1])[2]
                assert np.array_equal(got[k], px), f"{bad[k // 3][0]}: " + _first_difference(got[k][None], px[None])
        else:
            assert st[k] == 0 and np.array_equal(got[k], w), f"good frame at position {k}: status {st[k]}"
    assert (guard[0] == 0x5A).all() and (guard[19] == 0x5A).all()          # nothing outside the call's frames was written
    words = png.bad_frames(batch, status)
    assert [i for i, _ in words] == [k for k, w in enumerate(want) if isinstance(w, int)] and all(w for _, w in words)
    assert "CRC" in words[0][1]


def _raw_call(gpu_device, blobs, ws_short=0):
    """pr_png_decode between guard bands on the files' bytes, the three descriptor arrays, the workspace and the output: every
    tensor starts right behind a guard and ends right in front of one.  -> (return code, outputs or None)."""
    fr, idat, pal, pst, H, W, offsets = png.parse(blobs)
    data = np.frombuffer(b"".join(blobs), np.uint8)
    F = len(blobs)
    need = png.workspace_bytes(F, H, W, data.size)
    assert need > 0 and need % 16 == 0
    ins = dict(data=torch.from_numpy(data.copy()), frames=torch.from_numpy(np.frombuffer(fr.tobytes(), np.uint8).copy()),
               idat=torch.from_numpy(np.frombuffer(idat.tobytes(), np.uint8).copy()),
               palettes=torch.from_numpy(np.ascontiguousarray(pal).reshape(-1).copy() if pal.size else np.zeros(768, np.uint8)))
    outs = dict(out=((F, H, W, 3), torch.uint8), status=((F,), torch.int32), workspace=((need,), torch.uint8))
    rc = []

    def fn(i, o):
        args = _lib.PngArgs(i["data"].data_ptr(), i["frames"].data_ptr(), i["idat"].data_ptr(), i["palettes"].data_ptr(),
                            o["out"].data_ptr(), o["status"].data_ptr(), data.size, F, H, W, len(idat), max(len(pal), 1), 0)
        rc.append(_lib.load().pr_png_decode(args, o["workspace"].data_ptr(), need - ws_short,
                                            torch.cuda.current_stream(gpu_device).cuda_stream))
    exempt = ("out", "workspace") if not ws_short else ("out", "workspace", "status")
    res = gb.run_guarded(fn, ins, outs, device=gpu_device, may_hold_canary=exempt)
    return rc[0], res, pst


def test_the_entry_stays_inside_its_tensors_and_refuses_a_short_workspace(gpu_device):
    cases = pc.by_size()[(160, 90)]
    blobs = [s for _, s, _ in cases] + [b for _, b, _ in pc.gpu_bad_files()]
    rc, res, pst = _raw_call(gpu_device, blobs)
    assert rc == 0
    st = res["status"].cpu().tolist()
    assert st[:len(cases)] == [0] * len(cases) and st[len(cases):] == [1, 2, 4, 8, 16, 32] and pst[len(cases)] != 0
    got = res["out"].cpu().numpy()
    for k, (name, _, px) in enumerate(cases):
        assert np.array_equal(got[k], px), name
    for k, (name, blob, bit) in enumerate(pc.gpu_bad_files()):
        want = ref.decode(blob)[2] if bit >= 16 else np.zeros((90, 160, 3), np.uint8)
        assert np.array_equal(got[len(cases) + k], want), name
    # one byte short: refused with PR_ERR_CAPACITY before any device work
    rc, res, _ = _raw_call(gpu_device, blobs, ws_short=1)
    assert rc == -4
    assert bool((res["out"] == gb.CANARY_U8).all()) and bool((res["status"] == gb.CANARY_I32).all())
    assert bool((res["workspace"] == gb.CANARY_U8).all())


# ---- the Predictor on a folder of PNG frames -------------------------------------------------------------------------------
N_FRAMES = 9
TRACK_FRAMES = [1, 2, 3, 4, 5, 6, 8]


def _track():
    return {8: {'bbox': np.stack([np.array([380 + 9 * i, 225 - 4 * i, 170, 330], np.float32) for i in range(len(TRACK_FRAMES))]),
                'frames': np.array(TRACK_FRAMES)}}


def _predictor(gpu_device):
    import types
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=gpu_device)
    args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=True, debug_joints="L_Hip,Neck", debug_frame=-1)
    return base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=4)


def test_predictor_on_a_folder_of_png_frames(gpu_device, tmp_path):
    large = pc.large_frames()
    clip = tmp_path / "clip"
    clip.mkdir()
    for i in range(N_FRAMES):
        (clip / ("{0:09d}".format(i) + (".png" if i % 4 else ".PNG"))).write_bytes(large[(i * 2) % 3][1])
    with open(clip / "tracking.pkl", "wb") as f:
        pickle.dump(_track(), f)
    (clip / "notes.txt").write_text("not a frame")
    info = tmp_path / "info.json"
    info.write_text(json.dumps(synth.EXAMPLE_INFO))
    pred = _predictor(gpu_device)
    out = pred(str(clip), str(info), str(tmp_path / "out"))
    assert out["frames"].tolist() == TRACK_FRAMES and out["fps"] == 30.0          # fps.txt is optional
    arr = np.stack([large[(i * 2) % 3][2] for i in range(N_FRAMES)])
    npy = tmp_path / "npy"
    npy.mkdir()
    np.save(npy / "frames.npy", arr)
    with open(npy / "tracking.pkl", "wb") as f:
        pickle.dump(_track(), f)
    want = pred(str(npy), str(info), str(tmp_path / "out_npy"))
    for k in ("result", "joint_cam", "frames"):
        assert np.array_equal(np.asarray(out[k]), np.asarray(want[k])), k
    for t in ("reba", "rula"):
        np.testing.assert_array_equal(np.asarray(out[t][0], np.float64), np.asarray(want[t][0], np.float64), err_msg=t)
        for part in (1, 2):
            assert np.array_equal(np.asarray(out[t][part]), np.asarray(want[t][part])), (t, part)
    for name in ("reba_result.txt", "rula_result.txt"):
        a, b = (tmp_path / "out" / name).read_bytes(), (tmp_path / "out_npy" / name).read_bytes()
        assert a == b and len(a) > 0, name
    # a damaged frame raises, naming the file and the reason
    victim = clip / "000000005.png"
    data = victim.read_bytes()
    victim.write_bytes(data[:len(data) // 2])
    with pytest.raises(RuntimeError, match=r"000000005\.png.*ends inside a chunk"):
        pred(str(clip), str(info), str(tmp_path / "out_bad"))
