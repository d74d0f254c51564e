"""The frame sinks and the child-process helper without a GPU: a child that does not end is killed within its limit, the shared
write loop closes on success and aborts exactly once on an error, the cv2 sink releases its writer either way and orders the
channels, the Pillow sink names files by the numbers given, and the opener picks the sink and its file name for every codec."""
import sys
import time
import types

import numpy as np
import pytest
import torch

from poserisk_release_amd import _child, sinks

COPY = "import sys, shutil; shutil.copyfileobj(sys.stdin.buffer, open(sys.argv[1], 'wb'))"


def test_a_child_that_does_not_end_is_killed_within_the_limit():
    t0 = time.monotonic()
    child = _child.Child([sys.executable, "-c", "import time; time.sleep(30)"], "the video encoder", feed=True)
    child.pipe.close()
    with pytest.raises(RuntimeError, match=r"the video encoder `.*time\.sleep\(30\)'` failed with exit status -9: it did not end "
                                         r"after its standard input was closed$"):
        child.finish(0.5)
    assert child.poll() is not None
    assert time.monotonic() - t0 < 5


def test_a_child_that_cannot_be_started_and_one_that_is_read_from():
    with pytest.raises(RuntimeError, match=r"^'in.mkv': the video decoder `/no/such/decoder 'a b'` could not be started: "):
        _child.Child(["/no/such/decoder", "a b"], "'in.mkv': the video decoder", feed=False)
    child = _child.Child([sys.executable, "-c", "import sys; print('out'); sys.stderr.write('x' * 3000 + 'end'); sys.exit(4)"],
                         "the reader's", feed=False)
    assert child.pipe.read() == b"out\n"
    child.pipe.close()
    assert child.finish(5, raising=False) == 4                    # an abort: the status is returned, nothing is raised
    child = _child.Child([sys.executable, "-c", "import sys; sys.stderr.write('x' * 3000 + 'end'); sys.exit(4)"], "the reader's", feed=False)
    child.pipe.close()
    with pytest.raises(RuntimeError, match=r"failed with exit status 4: the caller's words; its standard error ends: x{1997}end$"):
        child.finish(5, "the caller's words")


class Recorder:
    """A sink that records what is done to it."""

    def __init__(self):
        self.calls = []

    def put(self, numbers, images):
        self.calls.append(("put", list(numbers), images))

    def close(self):
        self.calls.append(("close",))
        return "the path"

    def abort(self):
        self.calls.append(("abort",))


def test_the_write_loop_closes_on_success_and_aborts_once_on_an_error():
    def batches(fail):
        yield [0, 1], "a"
        if fail:
            raise KeyError("the iterator's own")
        yield [2], "b"
    sink = Recorder()
    assert sinks.write_all(sink, batches(False)) == "the path"
    assert sink.calls == [("put", [0, 1], "a"), ("put", [2], "b"), ("close",)]
    sink = Recorder()
    with pytest.raises(KeyError, match="the iterator's own"):
        sinks.write_all(sink, batches(True))
    assert sink.calls == [("put", [0, 1], "a"), ("abort",)]


class FakeWriter:
    made = []

    def __init__(self, path, fourcc, fps, size):
        self.args, self.frames, self.released = (path, fourcc, fps, size), [], 0
        FakeWriter.made.append(self)

    def write(self, frame):
        assert frame.flags["C_CONTIGUOUS"]
        self.frames.append(frame.copy())

    def release(self):
        self.released += 1


@pytest.fixture()
def fake_cv2(monkeypatch):
    FakeWriter.made = []
    monkeypatch.setitem(sys.modules, "cv2", types.SimpleNamespace(VideoWriter=FakeWriter))
    return FakeWriter.made


def test_the_cv2_sink_releases_on_close_and_on_abort_and_orders_the_channels(fake_cv2, tmp_path):
    images = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (2, 4, 6, 3), dtype=np.uint8))
    for bgr in (False, True):
        sink = sinks.open_sink("", str(tmp_path / "REBA_video"), 6, 4, 25, bgr)
        vw = fake_cv2[-1]
        assert isinstance(sink, sinks.Cv2Sink) and vw.args == (str(tmp_path / "REBA_video.mp4"), 0x7634706d, 25.0, (6, 4))
        assert vw.args[1] == sum(ord(c) << 8 * i for i, c in enumerate("mp4v"))
        sink.put([0, 1], images)
        want = images.numpy() if bgr else images.numpy()[..., ::-1]
        assert len(vw.frames) == 2 and all(np.array_equal(f, w) for f, w in zip(vw.frames, want))
        assert vw.released == 0
        assert sink.close() == str(tmp_path / "REBA_video.mp4") and vw.released == 1
    sink = sinks.open_sink("", str(tmp_path / "REBA_mesh"), 6, 4, 25, False)
    sink.put([0, 1], images)
    sink.abort()
    assert fake_cv2[-1].released == 1 and len(fake_cv2) == 3


def test_the_pillow_sink_names_its_files_by_the_numbers_given(tmp_path, monkeypatch):
    Image = pytest.importorskip("PIL.Image")
    monkeypatch.setitem(sys.modules, "cv2", None)
    images = np.random.default_rng(1).integers(0, 256, (3, 4, 6, 3), dtype=np.uint8)
    for bgr in (False, True):
        sink = sinks.open_sink("", str(tmp_path / f"mesh{bgr}"), 6, 4, 30.0, bgr)
        assert isinstance(sink, sinks.PillowSink)
        sink.put(np.array([7, 2, 40]), torch.from_numpy(images))
        assert sink.close() == str(tmp_path / f"mesh{bgr}")
        assert sorted(p.name for p in (tmp_path / f"mesh{bgr}").iterdir()) == ["000000002.png", "000000007.png", "000000040.png"]
        for number, im in zip((7, 2, 40), images):
            got = np.asarray(Image.open(tmp_path / f"mesh{bgr}" / f"{number:09d}.png").convert("RGB"))
            assert np.array_equal(got, im[..., ::-1] if bgr else im)
        sink.abort()                                              # nothing is held: nothing happens


@pytest.mark.parametrize("with_cv2", (True, False), ids=("cv2", "no-cv2"))
def test_the_opener_picks_the_sink_and_the_file_name(with_cv2, fake_cv2, tmp_path, monkeypatch):
    if not with_cv2:
        monkeypatch.setitem(sys.modules, "cv2", None)
    # no sink is put to: that this passes on a machine without a GPU is the proof that opening touches none
    stem = str(tmp_path / "REBA_video")
    encoder = f"{sys.executable} -c \"{COPY}\" {{output}}"
    cases = (("mjpeg", {}, sinks.AviSink, stem + ".avi"),
             ("png", {}, sinks.PngSink, stem),
             ("y4m", {}, sinks.Y4mSink, stem + ".y4m"),
             ("y4m", dict(encoder=encoder), sinks.Y4mSink, stem + ".mp4"),
             ("y4m", dict(encoder=encoder, encoder_ext=".mkv", chroma="444", matrix="auto"), sinks.Y4mSink, stem + ".mkv"),
             ("", {}, sinks.Cv2Sink if with_cv2 else sinks.PillowSink, stem + ".mp4" if with_cv2 else stem))
    for codec, knobs, kind, path in cases:
        sink = sinks.open_sink(codec, stem, 7, 5, 30.0, False, **knobs)
        assert type(sink) is kind and sink.path == path, (codec, knobs)
        sink.abort()
    assert {c for c, *_ in cases} == set(sinks.CODECS)
    assert len(fake_cv2) == (1 if with_cv2 else 0)                # only '' asks for cv2
    # what the y4m sink hands its writer: odd sides padded for a subsampled layout only, 'auto' resolved at 576 rows
    w = sinks.open_sink("y4m", stem, 7, 5, 30.0, True)._writer
    assert (w.out_width, w.out_height, w.chroma, w.matrix, w.full_range, w.bgr) == (8, 6, "420mpeg2", "601", False, True)
    w.abort()
    for height, matrix in ((576, "601"), (577, "709")):
        w = sinks.open_sink("y4m", stem, 7, height, 30.0, False, chroma="444", matrix="auto")._writer
        assert (w.out_width, w.out_height, w.matrix) == (7, height, matrix)
        w.abort()
    with pytest.raises(ValueError, match="codec 'h264' is not known"):
        sinks.open_sink("h264", stem, 7, 5, 30.0, False)
