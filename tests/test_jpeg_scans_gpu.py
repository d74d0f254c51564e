"""Progressive and multi-scan JPEG on the GPU (include/poserisk_hip.h, section j1b): every byte against libjpeg's pixels
(tests/golden/jpeg_progressive.npz: Pillow's progressive files; tests/jpeg_scans_cases.py: baseline golden cases transcoded
under other scan scripts), progressive and baseline frames mixed in one call, damaged streams beside good ones and the entry
inside guard bands, a Motion-JPEG AVI of progressive frames, the Predictor on a folder of them, and the entry in a captured
graph."""
import hashlib
import io
import json
import pickle
import types

import numpy as np
import pytest
import torch

import avi_cases as ac
import guard_band as gb
import jpeg_cases as jc
import jpeg_scans_cases as sc
from poserisk_release_amd import _lib, dropin, frontend, jpeg, synth

dropin.install()
from core import base  # noqa: E402
from core.config import cfg  # noqa: E402
from models import hmr  # noqa: E402
from smpl import SMPL  # noqa: E402

pytestmark = pytest.mark.gpu


def _first_difference(got, want):
    bad = np.argwhere(got != want)
    return f"{len(bad)} bytes differ, first (frame, row, col, channel) {bad[0].tolist()}: {got[tuple(bad[0])]} for {want[tuple(bad[0])]}"


@pytest.mark.parametrize("bgr", [False, True])
def test_every_small_fixture_and_transcoded_stream_is_byte_exact(gpu_device, bgr):
    groups = {}
    for name, stream, px in sc.all_small():
        groups.setdefault(px.shape[:2], []).append((name, stream, px))
    assert len(groups) == 5 and sum(map(len, groups.values())) == 35 + len(sc.TRANSCODED)
    for (H, W), cases in groups.items():
        frames, status = jpeg.decode_files([s for _, s, _ in cases], gpu_device, bgr=bgr, progressive=True)      # one call per size
        assert tuple(frames.shape) == (len(cases), H, W, 3) and frames.dtype == torch.uint8 and frames.is_cuda
        assert status.cpu().tolist() == [0] * len(cases), (H, W, status.cpu().tolist())
        want = np.stack([px[..., ::-1] if bgr else px for _, _, px in cases])
        got = frames.cpu().numpy()
        assert np.array_equal(got, want), f"{W}x{H} {[n for n, _, _ in cases]}: " + _first_difference(got, want)


def test_a_batch_of_64_frames_mixes_progressive_and_baseline_streams(gpu_device):
    """Frames are the unit of parallelism and the levels the launch structure: 64 frames of 800x450, three levels."""
    streams = sc.frames_800x450() + [s for s in jc.frames_800x450() if s[0] == "420_q95"]
    assert [n for n, *_ in streams] == ["progressive_420_q95", "progressive_420_q95_rstrow", "420_q95"]
    order = np.random.default_rng(64).integers(0, 3, 64)
    order[:3] = np.random.default_rng(65).permutation(3)                     # every stream at least once
    frames, status, stats = jpeg.decode_files([streams[i][1] for i in order], gpu_device, chunk=64, progressive=True, stats=True)
    assert tuple(frames.shape) == (64, 450, 800, 3)
    assert status.cpu().tolist() == [0] * 64 and not stats.any()             # the chunk took the multi-scan entry
    got = frames.cpu().numpy()
    first = {}
    for pos, i in enumerate(order):
        name, _, sha, spos, sval = streams[i]
        flat = got[pos].reshape(-1)
        if hashlib.sha256(flat.tobytes()).hexdigest() != sha:
            off = np.nonzero(flat[spos] != sval)[0]
            where = [(int(spos[o]) // 2400, int(spos[o]) % 2400 // 3, int(spos[o]) % 3, int(flat[spos[o]]), int(sval[o])) for o in off[:5]]
            pytest.fail(f"position {pos} ({name}): SHA-256 differs; {len(off)} of 4096 samples differ, (row, col, channel, got, "
                        f"want) {where}")
        assert np.array_equal(got[pos], got[first.setdefault(i, pos)]), f"{name} differs between positions {first[i]} and {pos}"
    for i in range(3):                                                        # and alone
        one, st = jpeg.decode_files([streams[i][1]], gpu_device, progressive=True)
        assert st.cpu().tolist() == [0] and np.array_equal(one.cpu().numpy()[0], got[first[i]]), streams[i][0]


def test_a_chunk_without_multi_scan_frames_takes_the_single_scan_path(gpu_device):
    cases = [(s, px) for n, s, px in jc.small_cases() if n.startswith("33x17")]
    free = [s for n, s, _ in jc.small_cases() if n.startswith("33x17") and "rst" not in n]
    frames, status, stats = jpeg.decode_files([s for s, _ in cases], gpu_device, progressive=True, stats=True)
    assert not status.any() and np.array_equal(frames.cpu().numpy(), np.stack([px for _, px in cases]))
    assert (stats[:, 0] >= 1).all()                                           # entropy="auto": the sub-sequence decoder ran
    want = jpeg.decode_files(free, gpu_device, stats=True)
    got = jpeg.decode_files(free, gpu_device, stats=True, progressive=True)
    assert all(torch.equal(a, b) for a, b in zip(want, got))
    # the default still refuses, by name
    prog = sc.fuzz_base()
    frames, status = jpeg.decode_files([free[0], prog], gpu_device)
    assert status.cpu().tolist()[0] == 0 and status.cpu().tolist()[1] & jpeg.ST_REFUSED
    assert "progressive" in jpeg.bad_frames([free[0], prog], status)[0][1]


def _packed(streams):
    """The one buffer decode_files uploads for a multi-scan chunk and where its parts lie."""
    frames, segs, huff, pst, H, W, offsets, scans, seg_scan, levels, multi = jpeg.parse_scans(streams)
    assert not pst.any() and multi > 0
    parts, at, pos = [np.frombuffer(b"".join(streams), np.uint8), frames, segs, seg_scan, scans, huff], [], 0
    for a in parts:
        at.append(pos)
        pos = (pos + a.nbytes + 255) // 256 * 256
    buf = np.zeros(pos, np.uint8)
    for a, o in zip(parts, at):
        buf[o:o + a.nbytes] = a.view(np.uint8).reshape(-1)
    return buf, dict(total=int(offsets[-1]), at=at, n_segs=len(segs), n_huff=len(huff), n_scans=len(scans), levels=levels, H=H, W=W,
                     F=len(streams))


def _decode_scans(dev_buf, m, out, status, ws, bgr=False):
    p = dev_buf.data_ptr()
    data, fr, seg, ss, scn, huff = (p + o for o in m["at"])
    args = _lib.JpegScansArgs(_lib.JpegArgs(data, fr, seg, huff, out.data_ptr(), status.data_ptr(), m["total"], m["F"], m["H"], m["W"],
                                            m["n_segs"], m["n_huff"], int(bgr)), scn, ss, m["n_scans"], m["levels"])
    stream = torch.cuda.current_stream(out.device).cuda_stream
    _lib.check(_lib.load().pr_jpeg_decode_scans(args, ws.data_ptr(), ws.numel(), stream), "pr_jpeg_decode_scans")


def test_bad_streams_in_a_good_batch_get_a_status_and_touch_nothing_else(gpu_device):
    """Six damaged progressive streams the CPU suite has proven on the host under sanitizers (tests/test_jpeg_scans_native.py,
    the same bytes by the same rule), each run once; then the entry once between canaries."""
    good = [(s, px) for n, s, px in sc.all_small() if px.shape[:2] == (17, 33)]
    bad = sc.gpu_bad_streams()
    assert len(bad) == 6 and len(good) >= 7
    batch, want = [], []
    for k in range(18):
        if k % 3 == 1:
            batch.append(bad[k // 3][1])
            want.append(None)
        else:
            s, px = good[(k - k // 3) % len(good)]
            batch.append(s)
            want.append(px)
    guard = torch.full((20, 17, 33, 3), 0x5A, dtype=torch.uint8, device=gpu_device)
    frames, status = jpeg.decode_files(batch, gpu_device, out=guard[1:19], progressive=True)
    torch.cuda.synchronize()
    st, got = status.cpu().tolist(), frames.cpu().numpy()
    for k, px in enumerate(want):
        if px is None:
            assert st[k] != 0, f"damaged stream at position {k} came back with status 0"
        else:
            assert st[k] == 0 and np.array_equal(got[k], px), f"good frame at position {k}: status {st[k]}"
    assert (guard[0] == 0x5A).all() and (guard[19] == 0x5A).all()          # nothing outside the call's frames was written
    words = jpeg.bad_frames(batch, status, progressive=True)
    assert [i for i, _ in words] == [k for k, px in enumerate(want) if px is None] and all(w for _, w in words)
    # the good frames of that batch through the entry itself, out, status and workspace between canaries
    streams = [s for s, px in zip(batch, want) if px is not None]
    buf, m = _packed(streams)
    F = len(streams)
    outs = gb.run_guarded(lambda ins, o: _decode_scans(ins["data"], m, o["out"], o["status"], o["workspace"]),
                          {"data": torch.from_numpy(buf)},
                          {"out": ((F, 17, 33, 3), torch.uint8), "status": ((F,), torch.int32),
                           "workspace": ((jpeg.workspace_bytes(F, 17, 33),), torch.uint8)},
                          device=gpu_device, may_hold_canary=("out", "workspace"))
    assert outs["status"].cpu().tolist() == [0] * F
    assert np.array_equal(outs["out"].cpu().numpy(), np.stack([px for px in want if px is not None]))


def test_a_motion_jpeg_avi_of_progressive_frames(gpu_device, tmp_path):
    from PIL import Image
    px = ac.clip_pixels(18)

    def progressive(p):
        b = io.BytesIO()
        Image.fromarray(p).save(b, "JPEG", quality=90, subsampling=2, progressive=True)
        return b.getvalue()
    (tmp_path / "prog.avi").write_bytes(ac.plain_avi([progressive(p) for p in px], 100, 48))
    (tmp_path / "base.avi").write_bytes(ac.plain_avi([ac.pillow_jpeg(p, 90, "4:2:0") for p in px], 100, 48))
    want, fps = frontend.read_video(str(tmp_path / "base.avi"), gpu_device)
    got, fps_p = frontend.read_video(str(tmp_path / "prog.avi"), gpu_device, progressive=True)
    assert tuple(got.shape) == (18, 48, 100, 3) and fps == fps_p
    assert torch.equal(got, want), _first_difference(got.cpu().numpy(), want.cpu().numpy())
    with pytest.raises(RuntimeError, match=r"prog\.avi.*frame 0 cannot be decoded.*progressive"):
        frontend.read_video(str(tmp_path / "prog.avi"), gpu_device)


N_FRAMES = 8
TRACK_FRAMES = [1, 2, 3, 4, 5, 6, 7]


def _track():
    return {8: {'bbox': np.stack([np.array([380 + 9 * i, 225 - 4 * i, 170, 330], np.float32) for i in range(len(TRACK_FRAMES))]),
                'frames': np.array(TRACK_FRAMES)}}


def test_predictor_on_a_folder_of_progressive_frames_equals_the_baseline_folder(gpu_device, tmp_path, monkeypatch):
    baseline = {n: s for n, s, *_ in jc.frames_800x450()}
    pairs = [(s, baseline[n[len("progressive_"):]]) for n, s, *_ in sc.frames_800x450()]
    for kind in (0, 1):
        folder = tmp_path / ("prog", "base")[kind]
        folder.mkdir()
        for i in range(N_FRAMES):
            (folder / "{0:09d}.jpg".format(i)).write_bytes(pairs[i % 2][kind])
        with open(folder / "tracking.pkl", "wb") as f:
            pickle.dump(_track(), f)
        (folder / "fps.txt").write_text("24.0")
    info = tmp_path / "info.json"
    info.write_text(json.dumps(synth.EXAMPLE_INFO))
    model = hmr()
    model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
    smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=gpu_device)
    args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=True, debug_joints="L_Hip,Neck", debug_frame=-1)
    pred = base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=4)
    assert cfg.DATASET.jpeg_progressive is True
    a = pred(str(tmp_path / "prog"), str(info), str(tmp_path / "out_prog"))
    b = pred(str(tmp_path / "base"), str(info), str(tmp_path / "out_base"))
    assert a["frames"].tolist() == TRACK_FRAMES
    for k in ("result", "joint_cam", "frames"):
        assert np.array_equal(np.asarray(a[k]), np.asarray(b[k])), k
    for t in ("reba", "rula"):
        np.testing.assert_array_equal(np.asarray(a[t][0], np.float64), np.asarray(b[t][0], np.float64), err_msg=t)
        for part in (1, 2):
            assert np.array_equal(np.asarray(a[t][part]), np.asarray(b[t][part])), (t, part)
    monkeypatch.setitem(cfg.DATASET, "jpeg_progressive", False)             # the knob restores the refusal
    with pytest.raises(RuntimeError, match=r"frame 0.*progressive"):       # every frame of the folder is refused
        pred(str(tmp_path / "prog"), str(info), str(tmp_path / "out_refused"))


def test_the_entry_captured_into_a_graph_replays_over_new_bytes(gpu_device):
    """Captures (so it neither allocates nor synchronises), replays, and gives the eager bytes."""
    cases = [(s, px) for n, s, px in sc.pillow_cases() if n.startswith("160x120") and "rst" not in n and "gray" not in n][:4]
    first, second = cases, cases[::-1]
    buf_a, m = _packed([s for s, _ in first])
    buf_b, m_b = _packed([s for s, _ in second])
    assert m == m_b and buf_a.shape == buf_b.shape and not np.array_equal(buf_a, buf_b) and m["levels"] == 3
    F, H, W = m["F"], m["H"], m["W"]
    dev = torch.zeros(len(buf_a), dtype=torch.uint8, device=gpu_device)
    out = torch.zeros((F, H, W, 3), dtype=torch.uint8, device=gpu_device)
    status = torch.zeros(F, dtype=torch.int32, device=gpu_device)
    ws = torch.zeros(jpeg.workspace_bytes(F, H, W), dtype=torch.uint8, device=gpu_device)
    dev.copy_(torch.from_numpy(buf_a))
    _decode_scans(dev, m, out, status, ws)
    torch.cuda.synchronize()
    eager = out.clone()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph):                                   # one chain of launches on one stream: no parallel branches
        _decode_scans(dev, m, out, status, ws)
    for buf, want in ((buf_a, first), (buf_b, second)):
        dev.copy_(torch.from_numpy(buf))
        out.fill_(0x5A)
        graph.replay()
        torch.cuda.synchronize()
        assert status.cpu().tolist() == [0] * F
        assert np.array_equal(out.cpu().numpy(), np.stack([px for _, px in want]))
        if buf is buf_a:
            assert torch.equal(out, eager)
