"""The encoder's golden cases (tests/golden/jpeg_encode.npz, written by tests/golden/make_jpeg_encode_golden.py) for the CPU,
native and GPU suites: source pixels and the complete files Pillow (libjpeg-turbo, optimize=False) wrote from them."""
import functools
import os

import numpy as np

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
RESTART = {"none": 0, "row": -1, "b3": 3}      # a case's restart tag -> the restart_interval the encoder is given
CANVAS_NAME = "1000x450_canvas_420_q90_row"


def canvas_source():
    """u8[450, 1000, 3], shaped like a composed score canvas (a picture beside a flat panel with thin strokes), from integer
    arithmetic only, so that it is the same array everywhere."""
    y, x = np.mgrid[0:450, 0:1000].astype(np.int64)
    h = ((x * 73856093) ^ (y * 19349663) ^ ((x * y) * 83492791)) >> 5
    img = np.stack([(x * 255 // 999 + (h & 7)) & 255, (y * 255 // 449 + ((h >> 3) & 7)) & 255,
                    ((x + 2 * y) * 255 // 1897 + ((h >> 6) & 7)) & 255], -1)
    disc = (x - 380) ** 2 + (y - 225) ** 2 < 120 ** 2
    img[disc] = img[disc] // 3 + 20
    box = (np.abs(x - 300) < 3) & (np.abs(y - 200) < 150) | (np.abs(y - 200) < 3) & (np.abs(x - 300) < 150)
    img[box] = (0, 255, 0)
    panel = x >= 800
    img[panel] = 32
    strokes = panel & (y % 18 < 11) & (((x * 7 + y // 18 * 13) % 11) < 4) & (x % 200 > 12) & (x % 200 < 188)
    img[strokes] = (255, 255, 255)
    return img.astype(np.uint8)


@functools.lru_cache(maxsize=None)
def _pack():
    z = np.load(os.path.join(GOLDEN, "jpeg_encode.npz"))
    return {k: z[k] for k in z.files}


def _case(i):
    z = _pack()
    name = str(z["names"][i])
    size, content, samp, q, rst = name.split("_")
    src = canvas_source() if content == "canvas" else z[f"src_{size}_{content}"]
    data = z["streams"][z["offsets"][i]:z["offsets"][i + 1]].tobytes()
    return dict(name=name, src=src, data=data, quality=int(q[1:]), subsampling=f"{samp[0]}:{samp[1]}:{samp[2]}",
                restart_interval=RESTART[rst], px_sha256=str(z["px_sha256"][i]))


def small_cases():
    """Every golden case but the 450x1000 canvas."""
    return [_case(i) for i, n in enumerate(_pack()["names"]) if str(n) != CANVAS_NAME]


def canvas_case():
    return _case(list(_pack()["names"]).index(CANVAS_NAME))
