"""The video front end on the MI355X: pr_resize_frames against tests/resize_ref.py bit for bit and inside guard bands,
frontend.read_video on hand-built Motion-JPEG AVI files against resize_ref(jpeg_ref decode), the round trip of the package's own
AVI output, and the Predictor on a `.avi` with a tracking sidecar, with a stand-in tracker, with neither, and on the folder that
`prepare` writes."""
import ctypes as C
import io
import json
import os
import pickle
import sys
import types

import numpy as np
import pytest
import torch
from PIL import Image

import avi_cases as ac
import guard_band as gb
import jpeg_cases as jc
import jpeg_ref
import resize_ref as rr
from poserisk_release_amd import _lib, dropin, frontend, jpeg, mjpeg, synth

dropin.install()
from core import base  # noqa: E402
from core.config import cfg  # noqa: E402
from models import hmr  # noqa: E402
from smpl import SMPL  # noqa: E402

pytestmark = pytest.mark.gpu
PAIR_IDS = [f"{W}x{H}-{w}x{h}" for (H, W), (h, w) in rr.SMALL_PAIRS]


def _three(H, W, seed):
    c = rr.contents(H, W, seed=seed)
    return np.stack([c["noise"], c["checker"], c["gradient"]])


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} bytes differ, first (frame, row, col, channel) {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


# ---- the kernel ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pair", rr.SMALL_PAIRS, ids=PAIR_IDS)
def test_resize_equals_the_reference_bit_for_bit(gpu_device, pair):
    """Three frames a call (noise, a 0 / 255 checker, a gradient); 53x37 -> 23x17 is 1173 bytes a frame, so frames 2 and 3 start
    unaligned; then the same call with the output's first byte at alignments 1, 2 and 3."""
    (H, W), (h, w) = pair
    frames = _three(H, W, H + W)
    want = rr.resize(frames, h, w)
    src = torch.from_numpy(frames).to(gpu_device)
    got = frontend.resize_frames(src, h, w)
    assert got.shape == (3, h, w, 3) and got.dtype == torch.uint8
    assert np.array_equal(got.cpu().numpy(), want), _first_difference(got.cpu().numpy(), want)
    n = 3 * h * w * 3
    for shift in (1, 2, 3):
        big = torch.full((n + 8,), 0x5A, dtype=torch.uint8, device=gpu_device)
        assert big.data_ptr() % 4 == 0
        out = big[shift:shift + n].view(3, h, w, 3)
        assert frontend.resize_frames(src, h, w, out=out) is out
        assert np.array_equal(out.cpu().numpy(), want), (shift, _first_difference(out.cpu().numpy(), want))
        assert bool((big[:shift] == 0x5A).all()) and bool((big[shift + n:] == 0x5A).all()), shift


def test_resize_on_a_non_default_stream_and_with_no_frames(gpu_device):
    (H, W), (h, w) = rr.SMALL_PAIRS[0]
    frames = _three(H, W, 5)
    src = torch.from_numpy(frames).to(gpu_device)
    torch.cuda.synchronize()
    side = torch.cuda.Stream(gpu_device)
    with torch.cuda.stream(side):
        got = frontend.resize_frames(src, h, w)
    side.synchronize()
    assert np.array_equal(got.cpu().numpy(), rr.resize(frames, h, w))
    assert frontend.resize_frames(src[:0], h, w).shape == (0, h, w, 3)
    with pytest.raises(_lib.PoseRiskHipError, match="GPU only"):
        frontend.resize_frames(torch.from_numpy(frames), h, w)
    with pytest.raises(ValueError, match="out must be"):
        frontend.resize_frames(src, h, w, out=torch.empty((3, h, w + 1, 3), dtype=torch.uint8, device=gpu_device))


@pytest.mark.parametrize("pair", rr.SMALL_PAIRS, ids=PAIR_IDS)
def test_resize_stays_inside_its_tensors(gpu_device, pair):
    """Source, tables and output each in the middle of an arena (tests/guard_band.py): nothing is written outside dst, nothing is
    left unwritten, and no value from outside src or the tables reaches the output (it equals the reference).  The int16 weight
    tables travel as the int32 words they are stored in."""
    (H, W), (h, w) = pair
    xofs, xcoef, yofs, ycoef, mode = frontend.resize_plan(H, W, h, w)
    lib = _lib.load()
    tables = {"xofs": torch.from_numpy(xofs), "xcoef": torch.from_numpy(xcoef.view(np.int32).copy()),
              "yofs": torch.from_numpy(yofs), "ycoef": torch.from_numpy(ycoef.view(np.int32).copy())}

    def call(ins, outs):
        _lib.check(lib.pr_resize_frames(ins["src"].data_ptr(), 3, H, W, outs["dst"].data_ptr(), h, w, ins["xofs"].data_ptr(),
                                        ins["xcoef"].data_ptr(), ins["yofs"].data_ptr(), ins["ycoef"].data_ptr(), mode,
                                        torch.cuda.current_stream(gpu_device).cuda_stream), "pr_resize_frames")
    frames = _three(H, W, 11)
    outs = gb.run_guarded(call, dict(src=torch.from_numpy(frames), **tables), {"dst": ((3, h, w, 3), torch.uint8)},
                          device=gpu_device, may_hold_canary=("dst",))          # noise may legitimately give 0x5A: compared below
    assert np.array_equal(outs["dst"].cpu().numpy(), rr.resize(frames, h, w))
    flat = np.full((3, H, W, 3), 200, np.uint8)                                 # no output equals the canary: every byte was written
    outs = gb.run_guarded(call, dict(src=torch.from_numpy(flat), **tables), {"dst": ((3, h, w, 3), torch.uint8)}, device=gpu_device)
    assert bool((outs["dst"] == 200).all())


# ---- read_video ---------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def clip():
    """12 frames of 100x48 written by Pillow (4:2:0 and 4:2:2, with and without restart markers) and what the front end must
    make of them at max_w = 44: resize_ref(jpeg_ref decode), 44x21."""
    px = ac.clip_pixels()
    files = ac.clip_frames(px)
    assert any(b"\xff\xdd" in f[:700] for f in files) and any(b"\xff\xdd" not in f[:700] for f in files)
    decoded = np.stack([jpeg_ref.decode(f) for f in files])
    assert frontend.target_size(100, 48, max_w=44) == (44, 21)
    want = rr.resize(decoded, 21, 44)
    want.setflags(write=False)
    return files, decoded, want


def _write(path, data):
    with open(path, "wb") as f:
        f.write(data)
    return str(path)


def test_read_video_equals_the_reference_whole_chunked_and_without_tables(gpu_device, clip, tmp_path):
    files, decoded, want = clip
    path = _write(tmp_path / "clip.avi", ac.plain_avi(files, 100, 48, rate=24, scale=1))
    got, fps = frontend.read_video(path, gpu_device, max_w=44)
    assert got.shape == (12, 21, 44, 3) and got.is_cuda and fps == 24.0
    assert np.array_equal(got.cpu().numpy(), want), _first_difference(got.cpu().numpy(), want)
    per = 48 * 100 * 3 + jpeg.workspace_bytes(1, 48, 100)
    assert frontend.chunk_frames(48, 100, 5 * per) == 5
    chunked, _ = frontend.read_video(path, gpu_device, max_w=44, max_bytes=5 * per)                 # chunks of 5, 5 and 2
    assert torch.equal(chunked, got)
    bgr, _ = frontend.read_video(path, gpu_device, max_w=44, bgr=True, max_bytes=5 * per)
    assert torch.equal(bgr, got.flip(-1))
    bare = _write(tmp_path / "bare.avi", ac.plain_avi([ac.strip_dht(f) for f in files], 100, 48))
    assert torch.equal(frontend.read_video(bare, gpu_device, max_w=44)[0], got)
    foreign, expected = ac.foreign_avi(files, 100, 48)
    odd, _ = frontend.read_video(_write(tmp_path / "foreign.avi", foreign), gpu_device, max_w=0, max_h=0)   # no resize: the decode alone
    assert np.array_equal(odd.cpu().numpy(), np.stack([decoded[files.index(f)] for f in expected]))


def test_read_video_names_a_damaged_or_refused_frame_by_its_index(gpu_device, clip, tmp_path):
    files, _, _ = clip
    per = 48 * 100 * 3 + jpeg.workspace_bytes(1, 48, 100)
    broken = list(files)
    broken[7] = files[7][:len(files[7]) // 2]
    path = _write(tmp_path / "broken.avi", ac.plain_avi(broken, 100, 48))
    for max_bytes in (16 << 30, 5 * per):
        with pytest.raises(RuntimeError, match=r"broken\.avi.*frame 7 cannot be decoded"):
            frontend.read_video(path, gpu_device, max_w=44, max_bytes=max_bytes)
    other = list(files)
    other[5] = ac.pillow_jpeg(ac.clip_pixels(1, 40, 100)[0])                   # another size: the first frame of the second chunk
    path = _write(tmp_path / "other.avi", ac.plain_avi(other, 100, 48))
    for max_bytes in (16 << 30, 5 * per):
        with pytest.raises(RuntimeError, match=r"other\.avi.*frame 5 cannot be decoded.*size"):
            frontend.read_video(path, gpu_device, max_w=44, max_bytes=max_bytes)
    progressive = io.BytesIO()
    Image.fromarray(ac.clip_pixels(1)[0]).save(progressive, "JPEG", progressive=True)
    path = _write(tmp_path / "prog.avi", ac.plain_avi([progressive.getvalue()] + files[:2], 100, 48))
    with pytest.raises(RuntimeError, match=r"prog\.avi.*frame 0 cannot be decoded.*progressive"):
        frontend.read_video(path, gpu_device)
    with pytest.raises(ValueError, match="not a RIFF AVI"):
        frontend.read_video(_write(tmp_path / "x.avi", b"\0" * 64), gpu_device)


def test_the_packages_own_avi_output_reads_back_as_decode_files_gives_it(gpu_device, clip, tmp_path):
    _, decoded, _ = clip
    frames = torch.from_numpy(decoded).to(gpu_device)
    buf, nbytes, status = jpeg.encode_frames(frames, quality=90)
    assert not bool(status.any())
    files = jpeg.download_files(buf, nbytes)
    with mjpeg.AviWriter(str(tmp_path / "own.avi"), 100, 48, 30.0, split_bytes=8192) as w:
        for f in files:
            w.write(f)
    assert len(w.paths) > 1
    got, fps = frontend.read_video(str(tmp_path / "own.avi"), gpu_device)
    want, st = jpeg.decode_files(files, gpu_device)
    assert not bool(st.any()) and fps == 30.0 and got.shape == (12, 48, 100, 3) and torch.equal(got, want)


# ---- the Predictor on a Motion-JPEG AVI ---------------------------------------------------------------------------------------
N_FRAMES = 9
TRACK_FRAMES = [1, 2, 3, 4, 5, 6, 8]
SCALE = 640 / 800                       # cfg.DATASET.front_max_w = 640 in these tests: 800x450 -> 640x360, the bilinear passes
REPORTS = ("reba_result.txt", "rula_result.txt", os.path.join("debug", "REBA_score_log.csv"), os.path.join("debug", "RULA_score_log.csv"))


def _track():
    return {8: {'bbox': np.stack([np.array([380 + 9 * i, 225 - 4 * i, 170, 330], np.float32) * SCALE for i in range(len(TRACK_FRAMES))]),
                'frames': np.array(TRACK_FRAMES)}}


def _same(out, want):
    for k in ("result", "joint_cam", "frames"):
        assert np.array_equal(np.asarray(out[k]), np.asarray(want[k])), k
    for t in ("reba", "rula"):
        np.testing.assert_array_equal(np.asarray(out[t][0], np.float64), np.asarray(want[t][0], np.float64), err_msg=t)   # NaN == NaN
        for part in (1, 2):
            assert np.array_equal(np.asarray(out[t][part]), np.asarray(want[t][part])), (t, part)


@pytest.fixture(scope="module")
def video(gpu_device, tmp_path_factory):
    """clip.avi: nine 800x450 frames from the four golden streams; the frames the front end must make of them (Pillow's decode
    is libjpeg's, resize_ref the downscale to 640x360); a Predictor."""
    d = tmp_path_factory.mktemp("avi")
    streams = [s for _, s, *_ in jc.frames_800x450()]
    order = [streams[(i * 3) % 4] for i in range(N_FRAMES)]
    _write(d / "clip.avi", ac.plain_avi(order, 800, 450, rate=24, scale=1))
    decoded = {id(s): np.asarray(Image.open(io.BytesIO(s)).convert("RGB")) for s in streams}
    frames = rr.resize(np.stack([decoded[id(s)] for s in order]), 360, 640)
    (d / "info.json").write_text(json.dumps(synth.EXAMPLE_INFO))
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=gpu_device)
    args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=True, debug_joints="L_Hip,Neck", debug_frame=-1)
    return d, frames, base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=4)


@pytest.fixture()
def knobs(monkeypatch):
    assert cfg.DATASET.front_max_w == 800 and cfg.DATASET.front_max_h == 450
    monkeypatch.setitem(cfg.DATASET, "front_max_w", 640)
    monkeypatch.setitem(sys.modules, "cv2", None)                              # not importable, whatever the machine has
    monkeypatch.setitem(sys.modules, "multi_person_tracker", None)


def test_predictor_on_an_avi_with_a_tracking_sidecar(gpu_device, video, knobs, tmp_path):
    d, frames, pred = video
    clip_path, info = str(d / "clip.avi"), str(d / "info.json")
    sidecar = d / "clip.tracking.pkl"
    # neither sidecar nor tracker: the error names the sidecar and the prepare command
    with pytest.raises(RuntimeError, match=r"clip\.tracking\.pkl.*frontend prepare .*clip\.avi") as e:
        pred(clip_path, info, str(tmp_path / "none"))
    assert "9 frames of 640 x 360" in str(e.value)
    try:
        with open(sidecar, "wb") as f:
            pickle.dump(_track(), f)
        out = pred(clip_path, info, str(tmp_path / "out"))
    finally:
        if sidecar.exists():
            sidecar.unlink()
    assert out["frames"].tolist() == TRACK_FRAMES and out["fps"] == 24.0
    want = pred.score_frames(frames, _track(), synth.EXAMPLE_INFO)
    _same(out, want)
    for name in REPORTS:
        assert (tmp_path / "out" / name).stat().st_size > 0, name
    # tracking handed to __call__ with frames=None: taken for an AVI, the same reports
    given = pred(clip_path, info, str(tmp_path / "given"), tracking_results=_track())
    _same(given, want)
    for name in REPORTS:
        assert (tmp_path / "given" / name).read_bytes() == (tmp_path / "out" / name).read_bytes(), name
    # a file that is no RIFF AVI goes on to the reference's front end, which is not importable here: today's message
    with open(clip_path, "rb") as f:
        mp4 = _write(tmp_path / "clip.mp4", b"\0\0\0\x18ftypmp42" + f.read()[12:])
    with pytest.raises(RuntimeError, match=r"clip\.mp4' is neither a directory with frames\.npy \+ tracking\.pkl nor one with JPEG frames .* "
                                         r"then call Predictor\.score_frames\(frames, tracking_results, info\)$"):
        pred(mp4, info, str(tmp_path / "mp4"))


def test_predictor_on_an_avi_with_a_tracker_and_on_the_prepared_folder(gpu_device, video, knobs, monkeypatch, tmp_path):
    d, frames, pred = video
    clip_path, info = str(d / "clip.avi"), str(d / "info.json")
    seen = {}

    class MPT:
        def __init__(self, **kw):
            seen["args"] = kw

        def __call__(self, folder):
            names = sorted(os.listdir(folder))
            seen["folder"], seen["names"] = folder, names
            seen["pixels"] = np.stack([np.asarray(Image.open(os.path.join(folder, n)).convert("RGB")) for n in names])
            seen["bytes"] = [open(os.path.join(folder, n), "rb").read() for n in names]
            return _track()
    mpt = types.ModuleType("multi_person_tracker")
    mpt.MPT = MPT
    monkeypatch.setitem(sys.modules, "multi_person_tracker", mpt)
    out = pred(clip_path, info, str(tmp_path / "out"))
    assert seen["names"] == ["{0:09d}.jpg".format(i) for i in range(N_FRAMES)] and seen["folder"] == str(tmp_path / "out" / "tmp")
    assert seen["args"] == dict(device=pred.device, batch_size=8, display=False, detection_threshold=0.1, detector_type='yolo',
                                output_format='dict', yolo_img_size=416)
    assert not os.path.exists(seen["folder"])                                  # removed afterwards
    # the tracker saw the downscaled frames as libjpeg writes them at quality 95, 4:2:0, a restart marker per MCU row: the
    # encoder is byte-exact with it (include/poserisk_hip.h, section j2), so Pillow's files of the reference frames are the files
    assert seen["bytes"] == [ac.pillow_jpeg(f, 95, "4:2:0", 1) for f in frames]
    assert seen["pixels"].shape == frames.shape
    # ... and the scores are those of the pixels decoded back from those files
    want = pred.score_frames(seen["pixels"], _track(), synth.EXAMPLE_INFO)
    _same(out, want)
    assert out["fps"] == 24.0
    # prepare writes that folder; with tracking.pkl added it is an input of its own, with the same scores
    folder = str(tmp_path / "prepared")
    n, size, fps = frontend.prepare(clip_path, folder, device=gpu_device, max_w=640)
    assert (n, size, fps) == (N_FRAMES, (640, 360), 24.0)
    assert sorted(os.listdir(folder)) == seen["names"] + ["fps.txt"]
    assert [open(os.path.join(folder, k), "rb").read() for k in seen["names"]] == seen["bytes"]
    with open(os.path.join(folder, "tracking.pkl"), "wb") as f:
        pickle.dump(_track(), f)
    again = pred(folder, info, str(tmp_path / "again"))
    _same(again, out)
    assert again["fps"] == 24.0
    for name in REPORTS:
        assert (tmp_path / "again" / name).read_bytes() == (tmp_path / "out" / name).read_bytes(), name


def test_prepare_from_the_command_line(gpu_device, clip, tmp_path):
    """`python -m poserisk_release_amd.frontend prepare` in a process of its own: the files are libjpeg's of the downscaled frames."""
    import subprocess
    from conftest import REPO
    files, _, want = clip
    path = _write(tmp_path / "clip.avi", ac.plain_avi(files, 100, 48))
    r = subprocess.run([sys.executable, "-m", "poserisk_release_amd.frontend", "prepare", path, str(tmp_path / "frames"), "--max-w", "44"],
                       cwd=REPO, capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-2000:]
    assert "12 frames of 44 x 21 at 25 frames/s" in r.stdout
    names = sorted(os.listdir(tmp_path / "frames"))
    assert names == ["{0:09d}.jpg".format(i) for i in range(12)] + ["fps.txt"] and float((tmp_path / "frames" / "fps.txt").read_text()) == 25.0
    for i, n in enumerate(names[:12]):
        assert (tmp_path / "frames" / n).read_bytes() == ac.pillow_jpeg(want[i], 95, "4:2:0", 1), n
