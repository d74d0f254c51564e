"""The YUV4MPEG2 writer without a GPU: the forward matrix's integers through _lib against tests/yuv_enc_ref.py, the contract's two
accuracy statements over all 2^24 colours, the reader's parser on what the writer's reference makes, y4m.write's bytes as they
were, the new symbols, and y4m.Writer's sinks and child failures driven through its host-only put_stream_bytes."""
import io
import os
import re
import sys

import numpy as np
import pytest

import yuv_enc_ref as er
import yuv_ref
from conftest import REPO
from poserisk_release_amd import _lib, dropin, y4m

dropin.install()
from core.config import cfg  # noqa: E402

COMBOS = [(m, f) for m in ("601", "709") for f in (False, True)]
COMBO_IDS = [f"{m}-{'full' if f else 'limited'}" for m, f in COMBOS]


# ---- the plan -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("matrix,full", COMBOS, ids=COMBO_IDS)
def test_the_plan_equals_the_reference_and_its_rows_sum_exactly(matrix, full):
    kyr, kyg, kyb, kc, kur, kug, kvb, kvg, yo = plan = y4m.yuv_enc_plan(matrix, full)
    assert plan == er.plan(matrix, full)
    sy, sc, want_yo = er.scales(full)
    assert kyr + kyg + kyb == int(np.rint(sy * 65536)) and kc == int(np.rint(sc * 32768)) and yo == want_yo
    assert kc - kur - kug == 0 and kc - kvg - kvb == 0
    assert min(plan[:8]) > 0
    if (matrix, full) == ("601", False):
        assert plan == (16829, 33039, 6416, 28784, 9714, 19070, 4681, 24103, 16)
    grey = np.broadcast_to(np.arange(256, dtype=np.uint8)[:, None, None, None], (256, 3, 3, 3))      # 256 flat frames
    for chroma in ("444", "420jpeg", "420mpeg2", "422"):
        Y, U, V = er.planes(grey, chroma, matrix, full, out_size=(4, 4))
        assert (U == 128).all() and (V == 128).all()
    assert (Y[0, 0, 0], Y[255, 3, 3]) == ((0, 255) if full else (16, 235))


def test_plan_refusals_by_name():
    lib = _lib.load()
    plan = _lib.YuvEncCoeffs()
    import ctypes as C
    for args, word in (((2, 0, C.byref(plan)), "matrix = 2"), ((0, 2, C.byref(plan)), "full_range = 2"), ((0, 0, None), "null plan_host")):
        assert lib.pr_yuv_enc_plan(*args) != 0
        assert word in lib.pr_last_error().decode()
    with pytest.raises(ValueError, match="'601' or '709'"):
        y4m.yuv_enc_plan("2020", False)


# ---- the two accuracy statements, over all 2^24 colours -------------------------------------------------------------------------
def _all_colours():
    """Yields u8[1, 1024, 1024, 3]: sixteen values of R a time with every G and B."""
    g, b = np.meshgrid(np.arange(256, dtype=np.uint8), np.arange(256, dtype=np.uint8), indexing="ij")
    for r0 in range(0, 256, 16):
        block = np.empty((16, 256, 256, 3), np.uint8)
        block[..., 0] = np.arange(r0, r0 + 16, dtype=np.uint8)[:, None, None]
        block[..., 1], block[..., 2] = g, b
        yield block.reshape(1, 1024, 1024, 3)


@pytest.mark.parametrize("matrix,full", COMBOS, ids=COMBO_IDS)
def test_every_colour_within_051_of_float64_and_the_444_round_trip_bound(matrix, full):
    """Every sample within 0.51 of the float64 evaluation; through j6's integer conversion (yuv_ref.convert, same matrix and
    range) every colour comes back within 1 level in full range, in limited range within 1 for R and G and within 2 for B."""
    worst_sample, worst_back = 0.0, np.zeros(3, np.int64)
    for rgb in _all_colours():
        Y, U, V = er.planes(rgb, "444", matrix, full)
        for got, exact in zip((Y, U, V), er.planes_f64(rgb, "444", matrix, full)):
            worst_sample = max(worst_sample, float(np.abs(got - exact).max()))
        back = yuv_ref.convert(Y, U, V, "444", matrix, full).astype(np.int64)
        worst_back = np.maximum(worst_back, np.abs(back - rgb).reshape(-1, 3).max(axis=0))
    print(f"{matrix} full={full}: worst sample error {worst_sample:.4f}, worst round trip (R, G, B) {worst_back.tolist()}")
    assert worst_sample <= 0.51
    assert all(w <= bound for w, bound in zip(worst_back.tolist(), (1, 1, 1) if full else (1, 1, 2)))


@pytest.mark.parametrize("chroma", ("420jpeg", "420mpeg2", "422"))
def test_subsampled_taps_stay_within_051_of_float64_too(chroma):
    rgb = np.random.default_rng(4).integers(0, 256, (2, 13, 17, 3), dtype=np.uint8)
    for matrix, full in COMBOS:
        for out in ((13, 17), (14, 18)):
            got, exact = er.planes(rgb, chroma, matrix, full, out_size=out), er.planes_f64(rgb, chroma, matrix, full, out_size=out)
            assert max(float(np.abs(g - e).max()) for g, e in zip(got, exact)) <= 0.51


# ---- the stream: the reader's parser on the writer's bytes ---------------------------------------------------------------------
@pytest.mark.parametrize("chroma", er.CHROMAS)
@pytest.mark.parametrize("full", (False, True, None), ids=("limited", "full", "unsaid"))
def test_the_readers_parser_reads_back_the_header_and_the_frames(chroma, full):
    W, H, F = 7, 5, 3
    rgb = np.random.default_rng(1).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    for out_H, out_W in ((H, W), (H + 1, W + 1)):
        head = y4m.stream_header(out_W, out_H, (24, 1), chroma, full)
        body = er.encode(rgb, chroma, "601", bool(full), out_size=(out_H, out_W))
        info = y4m.parse_header(head + body)
        fb = er.frame_bytes(out_W, out_H, chroma)
        assert (info.width, info.height, info.chroma, info.full_range, info.fps) == (out_W, out_H, chroma, full, 24.0)
        assert info.header_bytes == len(head) and info.frame_bytes == fb and len(body) == F * (6 + fb)
        offsets, used = y4m.index(body, info)
        assert offsets.tolist() == [k * (6 + fb) + 6 for k in range(F)] and used == len(body)
        assert y4m.encoded_size(W, H, chroma, pad_even=(out_H, out_W) != (H, W)) == (out_W, out_H, 6 + fb)
        ref = yuv_ref.parse_header(head + body)
        assert (ref["width"], ref["height"], ref["chroma"], ref["full_range"]) == (out_W, out_H, chroma, full)


def test_y4m_write_gives_the_bytes_it_gave_before():
    """The header line built by hand here, as y4m.write made it before stream_header was factored out of it."""
    rng = np.random.default_rng(3)
    Y, U, V = (rng.integers(0, 256, s, dtype=np.uint8) for s in ((2, 5, 7), (2, 3, 4), (2, 3, 4)))
    for fps, field in ((30.0, b"F30:1"), ((24, 1), b"F24:1"), (29.97, b"F2997:100"), (30000 / 1001, b"F30000:1001")):
        for full, tail in ((None, b""), (True, b" XCOLORRANGE=FULL"), (False, b" XCOLORRANGE=LIMITED")):
            want = b"YUV4MPEG2 W7 H5 " + field + b" Ip A1:1 C420mpeg2" + tail + b"\n"
            for k in range(2):
                want += b"FRAME Xq\n" + Y[k].tobytes() + U[k].tobytes() + V[k].tobytes()
            got = io.BytesIO()
            y4m.write(got, Y, U, V, fps=fps, chroma="420mpeg2", full_range=full, frame_fields=b" Xq")
            assert got.getvalue() == want
    got = io.BytesIO()
    y4m.write(got, Y, chroma="mono")
    assert got.getvalue() == b"YUV4MPEG2 W7 H5 F30:1 Ip A1:1 Cmono\n" + b"".join(b"FRAME\n" + Y[k].tobytes() for k in range(2))
    with pytest.raises(ValueError, match="is not one of"):
        y4m.stream_header(4, 4, 30.0, "411")


def test_the_new_symbols_are_declared_and_bound():
    with open(os.path.join(REPO, "include", "poserisk_hip.h")) as f:
        header = f.read()
    assert re.search(r"int pr_yuv_enc_plan\(int matrix, int full_range, pr_yuv_enc_coeffs\* plan_host\);", header)
    assert re.search(r"int pr_yuv_encode\(const pr_yuv_enc_args\* args, void\* stream\);", header)
    assert "/* j7 " in header and _lib.ABI_VERSION == 16                      # functions and structs were added: no bump
    lib = _lib.load()
    assert lib.pr_abi_version() == _lib.ABI_VERSION
    for name in ("pr_yuv_enc_plan", "pr_yuv_encode"):
        assert name in _lib.SIGNATURES and getattr(lib, name).argtypes is not None
    fields = re.search(r"typedef struct pr_yuv_enc_coeffs \{[^}]*\}", header).group(0)
    assert [n for n, _ in _lib.YuvEncCoeffs._fields_] == re.findall(r"\b(k\w+|yo)\b(?=[,;])", fields)
    args = re.search(r"typedef struct pr_yuv_enc_args \{[^}]*\}", header).group(0)
    assert [n for n, _ in _lib.YuvEncArgs._fields_] == re.findall(r"\b(\w+)(?=[,;])", args)
    import ctypes as C
    assert C.sizeof(_lib.YuvEncCoeffs) == 36 and C.sizeof(_lib.YuvEncArgs) == 16 + 36 + 7 * 4


def test_encode_frames_runs_on_the_gpu_only():
    import torch
    with pytest.raises(_lib.PoseRiskHipError, match="GPU only"):
        y4m.encode_frames(torch.zeros((1, 2, 2, 3), dtype=torch.uint8))


# ---- the Writer, driven on the host ---------------------------------------------------------------------------------------------
COPY = "import sys, shutil; shutil.copyfileobj(sys.stdin.buffer, open(sys.argv[1], 'wb'))"


def _body(W=7, H=5, F=3, chroma="420mpeg2", out=(6, 8)):
    rgb = np.random.default_rng(2).integers(0, 256, (F, H, W, 3), dtype=np.uint8)
    return er.encode(rgb, chroma, out_size=out)


def test_writer_to_a_file_an_object_and_a_child_gives_the_same_bytes(tmp_path):
    body = _body()
    want = y4m.stream_header(8, 6, 25.0, "420mpeg2", False) + body
    how = dict(width=7, height=5, fps=25.0, pad_even=True)
    mem = io.BytesIO()
    sinks = [(y4m.Writer(str(tmp_path / "a.y4m"), **how), lambda: (tmp_path / "a.y4m").read_bytes()),
             (y4m.Writer(mem, **how), mem.getvalue),
             (y4m.Writer(command=[sys.executable, "-c", COPY, str(tmp_path / "b.y4m")], **how), lambda: (tmp_path / "b.y4m").read_bytes())]
    for w, read in sinks:
        assert (w.out_width, w.out_height, w.frame_size) == (8, 6, 6 + 48 + 24)
        w.put_stream_bytes(body[:78], frames=1)
        w.put_stream_bytes(np.frombuffer(body[78:], np.uint8), frames=2)
        w.close()
        w.close()                                             # a second close is nothing
        assert w.frames_written == 3 and read() == want
        with pytest.raises(ValueError, match="closed"):
            w.put_stream_bytes(b"")
    assert not mem.closed                                     # an object given stays the caller's
    info = y4m.parse_header(want)
    assert (info.width, info.height, info.chroma, info.full_range) == (8, 6, "420mpeg2", False)
    with pytest.raises(ValueError, match="either dst"):
        y4m.Writer(width=4, height=4)
    with pytest.raises(ValueError, match="either dst"):
        y4m.Writer(mem, 4, 4, command=[sys.executable])


def test_writer_child_failures_raise_by_name():
    body = _body()
    w = y4m.Writer(command=[sys.executable, "-c", "import sys; sys.stdin.buffer.read(); sys.stderr.write('no such codec'); sys.exit(3)"],
                   width=7, height=5, pad_even=True)
    w.put_stream_bytes(body, frames=3)
    with pytest.raises(RuntimeError, match=r"(?s)video encoder `.*sys\.exit\(3\)'` failed with exit status 3.*standard error ends: no such codec"):
        w.close()
    # a child that ends before it reads: more bytes than a pipe holds, so the write meets the broken pipe
    w = y4m.Writer(command=[sys.executable, "-c", "import sys; sys.stderr.write('bye'); sys.exit(0)"], width=7, height=5)
    with pytest.raises(RuntimeError, match=r"(?s)video encoder `.*` failed with exit status 0: it closed its standard input.*ends: bye"):
        w.put_stream_bytes(bytes(4 << 20))
        w.close()
    assert w._child.poll() == 0                               # reaped
    with pytest.raises(RuntimeError, match=r"video encoder `/no/such/encoder -i -` could not be started"):
        y4m.Writer(command=["/no/such/encoder", "-i", "-"], width=7, height=5)
    # an exception of the caller's inside `with` stands, and the child is reaped all the same
    with pytest.raises(KeyError):
        with y4m.Writer(command=[sys.executable, "-c", "import sys; sys.stdin.buffer.read(); sys.exit(5)"], width=7, height=5) as w:
            raise KeyError("the caller's")
    assert w._child.poll() == 5


# ---- the knobs' defaults ------------------------------------------------------------------------------------------------------
def test_config_defaults_of_the_new_knobs():
    assert cfg.DATASET.video_encoder == "" and cfg.DATASET.video_encoder_ext == ".mp4" and cfg.DATASET.video_chroma == "420mpeg2"
    assert cfg.DATASET.gpu_video_codec == ""
