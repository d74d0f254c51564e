"""Writes tests/golden/jpeg_progressive.npz: progressive JPEG streams encoded by Pillow (libjpeg-turbo, libjpeg's default scan
script) from the very images of make_jpeg_golden.py, with the pixels Pillow decodes from them, two 800x450 progressive frames
(SHA-256 of the decoded pixels and 4096 samples, as jpeg_frames.npz), and the SHA-256 of every transcoded stream of
tests/jpeg_scans_cases.py AFTER Pillow has decoded it to its source case's golden pixels.  Seeded; needs Pillow, the tests do
not.    python tests/golden/make_jpeg_progressive_golden.py

names, streams, offsets, px_<i>      the small cases, as jpeg_cases.npz
frame_names, frame_streams, frame_offsets, frame_sha256, frame_sample_pos int64[2,4096], frame_sample_val u8[2,4096]
transcoded_names, transcoded_sha256  per entry of jpeg_scans_cases.TRANSCODED"""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image, ImageFile

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_cases as jc  # noqa: E402
import jpeg_scans_cases as sc  # noqa: E402
from make_jpeg_golden import content, encode, pack  # noqa: E402

ImageFile.MAXBLOCK = 1 << 24        # a progressive file is written in one piece: "Suspension not allowed here" otherwise


def main():
    rng = np.random.default_rng(20240607)                                    # make_jpeg_golden.py's images, in its order
    golden = {n: px for n, _, px in jc.small_cases()}
    names, streams, pixels = [], [], []

    def add(name, img, same_as=None, **kw):
        s, px = encode(img, progressive=True, **kw)
        assert b"\xff\xc2" in s.tobytes()
        if same_as:                                                          # the baseline encoding's pixels, to the byte
            assert np.array_equal(px, golden[same_as]), name
        names.append(name)
        streams.append(s)
        pixels.append(px)

    for H, W in [(16, 17), (17, 33), (29, 37), (32, 48), (120, 160)]:
        smooth, noise = content("smooth", H, W, rng), content("noise", H, W, rng)
        tag = f"{W}x{H}"
        add(f"{tag}_420_q75", smooth, same_as=f"{tag}_420_q75", quality=75, subsampling=2)
        add(f"{tag}_422_q90", smooth, same_as=f"{tag}_422_q90_opt", quality=90, subsampling=1)
        add(f"{tag}_444_q30", smooth, same_as=f"{tag}_444_q30", quality=30, subsampling=0)
        add(f"{tag}_gray_q85", smooth, same_as=f"{tag}_gray_q85", gray=True, quality=85)
        add(f"{tag}_420_q95_rstrow", smooth, same_as=f"{tag}_420_q95_rstrow", quality=95, subsampling=2, restart_marker_rows=1)
        add(f"{tag}_422_q60_rst3", noise, same_as=f"{tag}_422_q60_rst3", quality=60, subsampling=1, restart_marker_blocks=3)
        add(f"{tag}_420_q100_noise", noise, same_as=f"{tag}_420_q100_noise", quality=100, subsampling=2)
    data, offsets = pack(streams)

    H, W = 450, 800
    frame = content("smooth", H, W, rng, sigma=3.0)
    yy, xx = np.mgrid[0:H, 0:W]
    frame[((yy - 225) ** 2 + (xx - 380) ** 2) < 90 ** 2] //= 2
    baseline = {n: sha for n, _, sha, *_ in jc.frames_800x450()}
    pos_rng = np.random.default_rng(20251019)
    fnames, fstreams, sha, spos, sval = [], [], [], [], []
    for i, (name, kw) in enumerate([("420_q95", dict(quality=95, subsampling=2)),
                                    ("420_q95_rstrow", dict(quality=95, subsampling=2, restart_marker_rows=1))]):
        s, px = encode(np.roll(frame, 11 * i, axis=1), progressive=True, **kw)
        flat = px.reshape(-1)
        sha.append(hashlib.sha256(flat.tobytes()).hexdigest())
        assert sha[-1] == baseline[name], name                               # the baseline frame of jpeg_frames.npz, to the byte
        fnames.append("progressive_" + name)
        fstreams.append(s)
        pos = np.sort(pos_rng.choice(flat.size, 4096, replace=False)).astype(np.int64)
        spos.append(pos)
        sval.append(flat[pos])
    fdata, foffsets = pack(fstreams)

    tnames, tsha = [], []
    for name, stream, want in sc.transcoded_cases.__wrapped__(check=False):
        got = np.asarray(Image.open(io.BytesIO(stream)).convert("RGB"))
        assert np.array_equal(got, want), f"{name}: Pillow does not decode the transcoded stream to its source's pixels"
        tnames.append(name)
        tsha.append(hashlib.sha256(stream).hexdigest())

    out = os.path.join(HERE, "jpeg_progressive.npz")
    np.savez_compressed(out, names=np.array(names), streams=data, offsets=offsets, **{f"px_{i}": p for i, p in enumerate(pixels)},
                        frame_names=np.array(fnames), frame_streams=fdata, frame_offsets=foffsets, frame_sha256=np.array(sha),
                        frame_sample_pos=np.stack(spos), frame_sample_val=np.stack(sval),
                        transcoded_names=np.array(tnames), transcoded_sha256=np.array(tsha))
    print("jpeg_progressive.npz", os.path.getsize(out), "bytes;", len(names), "small,", len(fnames), "frames,", len(tnames), "transcoded;",
          "frame bytes", [len(s) for s in fstreams])


if __name__ == "__main__":
    main()
