"""The frame sinks on the GPU: the overflow retry (encode into the first slot, encode again alone what overflowed it) gives the
files the full bound gives, for JPEG and for PNG, and a Motion-JPEG sink that is aborted leaves a file that holds what was put."""
import numpy as np
import pytest
import torch

import riff_reader
from poserisk_release_amd import _media, jpeg, png, sinks

pytestmark = pytest.mark.gpu
NOISY = (1, 3)


def _frames():
    """Five frames of 64 x 64: three smooth ones (ramps) and, at positions 1 and 3, uniform noise."""
    rng = np.random.default_rng(11)
    y, x = np.mgrid[0:64, 0:64]
    frames = np.stack([np.stack([(2 * x + 30 * k) % 256, (3 * y + 2 * k) % 256, (x + y + 7 * k) % 256], axis=-1) for k in range(5)])
    for k in NOISY:
        frames[k] = rng.integers(0, 256, (64, 64, 3))
    return frames.astype(np.uint8)


ENCODERS = {"jpeg": (lambda images, capacity: jpeg.encode_frames(images, quality=90, capacity=capacity), lambda: jpeg.encode_bound(64, 64),
                     jpeg.ENC_ST_OVERFLOW),
            "png": (lambda images, capacity: png.encode_frames(images, capacity=capacity), lambda: png.encode_bound(64, 64),
                    png.ENC_ST_OVERFLOW)}


@pytest.mark.parametrize("kind", sorted(ENCODERS))
def test_the_overflow_retry_gives_the_files_of_the_full_bound(gpu_device, kind):
    encode, bound, overflow = ENCODERS[kind]
    images = torch.from_numpy(_frames()).to(gpu_device)
    buf, nbytes, status = encode(images, bound())
    assert status.cpu().tolist() == [0] * 5
    want = _media.download_files(buf, nbytes)
    sizes = [len(f) for f in want]
    smooth, noise = max(s for k, s in enumerate(sizes) if k not in NOISY), min(sizes[k] for k in NOISY)
    print(f"{kind}: file sizes {sizes}, bound {bound()}")
    assert smooth + 1 < noise, "the noise frames must come out larger than every smooth one: choose other frames"
    first = (smooth + noise) // 2
    assert smooth < first < noise
    _, nbytes1, status1 = encode(images, first)
    assert status1.cpu().tolist() == [overflow if k in NOISY else 0 for k in range(5)]      # the retry has something to do
    assert nbytes1.cpu().tolist() == [0 if k in NOISY else sizes[k] for k in range(5)]
    got = _media.encode_files(encode, images, first, bound(), kind)
    assert got == want
    with pytest.raises(RuntimeError, match=f"^{kind}: status {overflow} for a frame with the largest slot$"):
        _media.encode_files(encode, images, first, noise - 1, kind)     # a 'bound' below frame 1's size: it still does not fit


def test_an_aborted_avi_sink_holds_the_frames_that_were_put(gpu_device, tmp_path):
    images = torch.from_numpy(_frames()).to(gpu_device)
    buf, nbytes, status = jpeg.encode_frames(images, quality=80, capacity=jpeg.encode_bound(64, 64))
    want = jpeg.download_files(buf, nbytes)
    assert status.cpu().tolist() == [0] * 5 and all(want)
    sink = sinks.open_sink("mjpeg", str(tmp_path / "REBA_video"), 64, 64, 25.0, False, quality=80)
    sink.put(range(0, 3), images[:3])
    sink.put(range(3, 5), images[3:])
    sink.abort()
    avi = riff_reader.read_avi(tmp_path / "REBA_video.avi")
    assert avi["frames"] == want
    assert (avi["count"], avi["stream_count"], len(avi["index"])) == (5, 5, 5) and avi["has_index"]
    assert (avi["width"], avi["height"], avi["fps"], avi["compression"]) == (64, 64, 25.0, b"MJPG")
    assert avi["index"] == list(zip(avi["offsets"], map(len, want)))
