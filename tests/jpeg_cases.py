"""What the JPEG tests share (not a test module): the golden streams, the seeded damaged streams of the robustness tests and
the choice of the six that also run on the GPU.  tests/test_jpeg_native.py proves every damaged stream on the host under
sanitizers; tests/test_jpeg_gpu.py runs `gpu_bad_streams()` only -- the same bytes, chosen by the same rule."""
import os

import numpy as np

import jpeg_ref as jr

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
FUZZ_CASE = "33x17_422_q60_rst3"      # small, with a restart interval: the parser's whole path
FUZZ_SEED, FUZZ_N = 77, 2000


def small_cases():
    """[(name, stream bytes, pixels u8[H,W,3] RGB as Pillow decoded them)]"""
    z = np.load(os.path.join(GOLDEN, "jpeg_cases.npz"))
    off, s = z["offsets"], z["streams"]
    return [(str(n), s[off[i]:off[i + 1]].tobytes(), z[f"px_{i}"]) for i, n in enumerate(z["names"])]


def frames_800x450():
    """[(name, stream bytes, sha256 hex of the RGB pixels, sample positions, sample values)]"""
    z = np.load(os.path.join(GOLDEN, "jpeg_frames.npz"))
    off, s = z["offsets"], z["streams"]
    return [(str(n), s[off[i]:off[i + 1]].tobytes(), str(z["sha256"][i]), z["sample_pos"][i], z["sample_val"][i])
            for i, n in enumerate(z["names"])]


def fuzz_base():
    return next(s for n, s, _ in small_cases() if n == FUZZ_CASE)


def truncations(stream):
    return [stream[:n] for n in range(len(stream))]


def corruptions(stream, n=FUZZ_N, seed=FUZZ_SEED):
    """n copies of the stream with one byte each set to another value (seeded)."""
    rng = np.random.default_rng(seed)
    out = []
    for _ in range(n):
        pos = int(rng.integers(0, len(stream)))
        val = (stream[pos] + int(rng.integers(1, 256))) & 255
        out.append(stream[:pos] + bytes([val]) + stream[pos + 1:])
    return out


def reference_verdict(stream):
    """'refused', 'bad' (the parser's rules accept it, decoding by the contract fails) or the decoded pixels."""
    try:
        p = jr.parse(stream)
    except jr.Refused:
        return "refused"
    try:
        return jr.decode_strict(stream, p)
    except jr.BadStream:
        return "bad"


def gpu_bad_streams(count=6):
    """The first `count` corruptions of the fuzz stream that the parser accepts at the original size and that cannot be decoded
    (the reference fails): the device must give each a non-zero status.  [(index among the corruptions, bytes)]"""
    base = fuzz_base()
    size = jr.parse(base)
    out = []
    for i, s in enumerate(corruptions(base)):
        try:
            p = jr.parse(s)
        except jr.Refused:
            continue
        if (p["width"], p["height"]) != (size["width"], size["height"]):
            continue
        if isinstance(reference_verdict(s), str):
            out.append((i, s))
            if len(out) == count:
                break
    return out
