"""Writes tests/golden/jpeg_encode.npz: source pixels and the complete baseline JPEG files Pillow (libjpeg-turbo) writes from
them with optimize=False -- what pr_jpeg_encode has to reproduce byte for byte.  Seeded; needs Pillow, the tests do not.
    python tests/golden/make_jpeg_encode_golden.py

names (U) `<W>x<H>_<content>_<sampling>_q<quality>_<restart>`, streams (one u8 array, `offsets` cuts it) and one
`src_<W>x<H>_<content>` u8[H,W,3] per source; px_sha256 (U) is the sha256 of the RGB pixels Pillow decodes from each file.  The 450x1000 canvas case stores no source: tests/jpeg_enc_cases.py makes it from
integer arithmetic.  A pruned cross product: every quality x sampling pair with both odd-sized images, content and restart
setting cycling through them; a Latin selection at the other sizes."""
import hashlib
import io
import os
import sys

import numpy as np
from PIL import Image

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
import jpeg_enc_cases as ec   # noqa: E402
from make_jpeg_golden import content   # noqa: E402

SUB = {"444": 0, "422": 1, "420": 2}
RST = {"none": {}, "row": dict(restart_marker_rows=1), "b3": dict(restart_marker_blocks=3)}
QUALITIES, CONTENTS = (1, 30, 75, 90, 100), ("smooth", "noise")


def save(img, samp, q, rst):
    buf = io.BytesIO()
    Image.fromarray(img).save(buf, "JPEG", quality=q, subsampling=SUB[samp], optimize=False, **RST[rst])
    return np.frombuffer(buf.getvalue(), np.uint8)


def decoded_sha(stream):
    return hashlib.sha256(np.asarray(Image.open(io.BytesIO(stream.tobytes())).convert("RGB")).tobytes()).hexdigest()


def main():
    rng = np.random.default_rng(20250311)
    names, streams, sources = [], [], {}
    for H, W in [(16, 17), (17, 33), (29, 37), (32, 48), (120, 160), (50, 1000)]:
        src = {c: content(c, H, W, rng) for c in CONTENTS}
        odd = H % 2 and W % 2
        picks, n = [], 0
        for qi, q in enumerate(QUALITIES):
            for si, samp in enumerate(SUB):
                if odd or (qi + si) % 3 == (H // 8) % 3:
                    picks.append((CONTENTS[n % 2], samp, q, list(RST)[(qi + si) % 3 if odd else qi % 3]))
                    n += 1
        if (H, W) == (120, 160):
            picks.append(("noise", "420", 100, "none"))      # even, not a multiple of 16: the last chroma block row
        if (H, W) == (50, 1000):
            picks = [p for p in picks if not (p[0] == "noise" and p[2] > 75)] + [("noise", "420", 30, "row"), ("smooth", "420", 90, "row")]
        for c, samp, q, rst in dict.fromkeys(picks):
            names.append(f"{W}x{H}_{c}_{samp}_q{q}_{rst}")
            streams.append(save(src[c], samp, q, rst))
            sources[f"src_{W}x{H}_{c}"] = src[c]
    names.append(ec.CANVAS_NAME)
    streams.append(save(ec.canvas_source(), "420", 90, "row"))
    for H, W in ((17, 33), (29, 37)):                        # every value of every axis with both odd-sized images
        mine = [n.split("_") for n in names if n.startswith(f"{W}x{H}_")]
        assert {m[1] for m in mine} == set(CONTENTS) and {m[2] for m in mine} == set(SUB) and {m[4] for m in mine} == set(RST)
        assert {m[3] for m in mine} == {f"q{q}" for q in QUALITIES}
    path = os.path.join(HERE, "jpeg_encode.npz")
    np.savez_compressed(path, names=np.array(names), streams=np.concatenate(streams), px_sha256=np.array([decoded_sha(s) for s in streams]),
                        offsets=np.cumsum([0] + [len(s) for s in streams]).astype(np.int64), **sources)
    print(len(names), "cases,", os.path.getsize(path), "bytes; canvas", len(streams[-1]))


if __name__ == "__main__":
    main()
