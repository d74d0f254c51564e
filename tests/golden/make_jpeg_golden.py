"""Writes tests/golden/jpeg_cases.npz and tests/golden/jpeg_frames.npz: baseline JPEG streams encoded by Pillow (libjpeg-turbo)
with the pixels Pillow decodes from them -- libjpeg's default path (islow IDCT, fancy upsampling), which is what cv2.imread runs.
Seeded; needs Pillow, the tests do not.    python tests/golden/make_jpeg_golden.py

jpeg_cases.npz   names (U), streams (one u8 array, `offsets` cuts it), and per case `px_<i>` u8[H,W,3] (RGB; gray replicated).
jpeg_frames.npz  four 800x450 streams (names, streams, offsets), sha256 of each one's decoded RGB pixels (hex), and 4096 sampled
                 (flat byte position, value) pairs per stream for diagnosis: sample_pos int64[4,4096], sample_val u8[4,4096]."""
import hashlib
import io
import os

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))


def content(kind, H, W, rng, sigma=6.0):
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, 3), dtype=np.uint8)
    img = np.stack([127 + 120 * np.sin(xx / (3.0 + W / 9) + c) * np.cos(yy / (2.0 + H / 7) - c) for c in range(3)], -1)
    img += 40 * ((xx // 7 + yy // 5) % 2)[..., None] * np.array([1, -1, 0.5])       # hard edges: chroma that upsampling must place
    img += rng.normal(0, sigma, img.shape)
    return np.clip(img, 0, 255).astype(np.uint8)


def encode(img, gray=False, **kw):
    im = Image.fromarray(img)
    if gray:
        im = im.convert("L")
    buf = io.BytesIO()
    im.save(buf, "JPEG", **kw)
    data = buf.getvalue()
    px = np.asarray(Image.open(io.BytesIO(data)).convert("RGB"))
    return np.frombuffer(data, np.uint8), px


def pack(streams):
    return np.concatenate(streams), np.cumsum([0] + [len(s) for s in streams]).astype(np.int64)


def main():
    rng = np.random.default_rng(20240607)
    names, streams, pixels = [], [], []

    def add(name, img, **kw):
        s, px = encode(img, **kw)
        names.append(name)
        streams.append(s)
        pixels.append(px)

    sizes = [(16, 17), (17, 33), (29, 37), (32, 48), (120, 160)]            # (H, W); 29x37 and 17x33: both odd
    for H, W in sizes:
        smooth, noise = content("smooth", H, W, rng), content("noise", H, W, rng)
        tag = f"{W}x{H}"
        add(f"{tag}_420_q75", smooth, quality=75, subsampling=2)
        add(f"{tag}_422_q90_opt", smooth, quality=90, subsampling=1, optimize=True)
        add(f"{tag}_444_q30", smooth, quality=30, subsampling=0)
        add(f"{tag}_gray_q85", smooth, gray=True, quality=85)
        add(f"{tag}_420_q95_rstrow", smooth, quality=95, subsampling=2, restart_marker_rows=1)
        add(f"{tag}_422_q60_rst3", noise, quality=60, subsampling=1, restart_marker_blocks=3)
        add(f"{tag}_420_q100_noise", noise, quality=100, subsampling=2)
        if H <= 32:
            add(f"{tag}_444_q100_noise_opt_rst3", noise, quality=100, subsampling=0, optimize=True, restart_marker_blocks=3)
            add(f"{tag}_gray_q50_noise_rstrow", noise, gray=True, quality=50, restart_marker_rows=1)
    data, offsets = pack(streams)
    np.savez_compressed(os.path.join(HERE, "jpeg_cases.npz"), names=np.array(names), streams=data, offsets=offsets,
                        **{f"px_{i}": p for i, p in enumerate(pixels)})

    H, W = 450, 800
    frame = content("smooth", H, W, rng, sigma=3.0)                        # keeps the four streams under 1 MiB together
    yy, xx = np.mgrid[0:H, 0:W]
    frame[((yy - 225) ** 2 + (xx - 380) ** 2) < 90 ** 2] //= 2               # a dark disc: something to crop
    opts = [("420_q95", dict(quality=95, subsampling=2)), ("420_q95_rstrow", dict(quality=95, subsampling=2, restart_marker_rows=1)),
            ("420_q95_opt", dict(quality=95, subsampling=2, optimize=True)), ("444_q95", dict(quality=95, subsampling=0))]
    fnames, fstreams, sha, spos, sval = [], [], [], [], []
    for i, (name, kw) in enumerate(opts):
        s, px = encode(np.roll(frame, 11 * i, axis=1), **kw)
        fnames.append(name)
        fstreams.append(s)
        flat = px.reshape(-1)
        sha.append(hashlib.sha256(flat.tobytes()).hexdigest())
        pos = np.sort(rng.choice(flat.size, 4096, replace=False)).astype(np.int64)
        spos.append(pos)
        sval.append(flat[pos])
    data, offsets = pack(fstreams)
    np.savez_compressed(os.path.join(HERE, "jpeg_frames.npz"), names=np.array(fnames), streams=data, offsets=offsets,
                        sha256=np.array(sha), sample_pos=np.stack(spos), sample_val=np.stack(sval))
    for f in ("jpeg_cases.npz", "jpeg_frames.npz"):
        print(f, os.path.getsize(os.path.join(HERE, f)), "bytes")


if __name__ == "__main__":
    main()
