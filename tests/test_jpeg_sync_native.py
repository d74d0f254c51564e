"""pr_jpeg_decode_sync -- entropy decoding by self-synchronising sub-sequences, csrc/jpeg_sync.hip -- on the CPU, under
ASan + UBSan.

The kernels index by thread only, so tests/native/host_shim.h turns a launch into nested loops and g++ builds
csrc/jpeg_host.cc, csrc/jpeg.hip and csrc/jpeg_sync.hip into one stand-alone driver, tests/native/jpeg_sync_native.cc, which
decodes every stream on its own, in exact-size heap blocks, by pr_jpeg_decode AND by pr_jpeg_decode_sync.  Checked here, without
a GPU: every golden case byte for byte at four (sub-sequence bytes, rounds) settings with its statistics, that the defaults
synchronise everything but saturating noise, that the iteration, blocks spanning three sub-sequences and cuts inside a stuffed
FF 00 pair are really exercised, the header's contract against pr_jpeg_decode and the numpy reference on one stream cut at
every byte and corrupted 2000 times, and every argument error."""
import functools

import numpy as np
import pytest

import host_build
import jpeg_cases as jc
import jpeg_ref as jr

DEFAULT_S, DEFAULT_R = 128, 16        # include/poserisk_hip.h: the build's defaults
SETTINGS = [(0, 0), (16, 64), (64, 8), (128, 1)]


@pytest.fixture(scope="module")
def native(tmp_path_factory):
    d = tmp_path_factory.mktemp("jpeg_sync_native")
    exe = host_build.build(d, "jpeg_sync_native", "jpeg_sync_native.cc", stage=("jpeg.hip", "jpeg_sync.hip", "jpeg_host.cc"), shim=True)
    cache = {}

    def each(key, streams, S, R, bgr=0):
        """-> per stream dict(parse_status, serial, sync, stats = (n_subseq, rounds, fell_back), serial_px, sync_px)"""
        if (key, S, R, bgr) in cache:
            return cache[key, S, R, bgr]
        exe.run("each", host_build.pack_streams(d / "pack.bin", streams), d / "out.bin", S, R, bgr)
        raw, pos, out = np.fromfile(d / "out.bin", np.uint8), 0, []
        for _ in streams:
            head = raw[pos:pos + 44].view(np.int32)
            pos += 44
            rec = dict(parse_status=int(head[0]), serial=int(head[5]), sync=int(head[6]), stats=tuple(int(v) for v in head[7:10]))
            if rec["parse_status"] == 0:
                H, W = int(head[3]), int(head[4])
                for k in ("serial_px", "sync_px"):
                    rec[k] = raw[pos:pos + H * W * 3].reshape(H, W, 3)
                    pos += H * W * 3
            out.append(rec)
        assert pos == raw.size
        cache[key, S, R, bgr] = out
        return out

    def args(stream):
        return exe.run("args", host_build.pack_streams(d / "args.bin", [stream])).stdout
    return each, args


def _subseq(stream, S):
    """(sum over the segments of ceil(length / S), the largest of them) from the reference's parse."""
    n = [-(-(end - begin) // S) for begin, end, _ in jr.parse(stream)["segments"]]
    return sum(n), max(n)


@pytest.mark.parametrize("S,R", SETTINGS)
def test_every_golden_case_is_byte_exact_with_its_statistics(native, S, R):
    each, _ = native
    cases = jc.small_cases()
    assert len(cases) >= 36
    for bgr in (0, 1):
        got = each("small", [s for _, s, _ in cases], S, R, bgr)
        for (name, stream, want), rec in zip(cases, got):
            assert rec["parse_status"] == 0 and rec["sync"] == 0 and rec["serial"] == 0, (name, rec["parse_status"], rec["sync"])
            bad = np.argwhere(rec["sync_px"] != (want[..., ::-1] if bgr else want))
            assert bad.size == 0, f"{name} S={S} R={R} bgr={bgr}: {len(bad)} bytes differ, first (row, col, channel) {bad[0].tolist()}"
            total, most = _subseq(stream, S or DEFAULT_S)
            n_subseq, rounds, fell_back = rec["stats"]
            assert n_subseq == total and 1 <= rounds <= (R or DEFAULT_R) and fell_back in (0, 1), (name, rec["stats"], total)
            assert fell_back == 0 or rounds == (R or DEFAULT_R), (name, rec["stats"])
            if (S, R) == (128, 1) and most > 2:
                assert fell_back == 1, f"{name}: {most} sub-sequences in a segment cannot be proven in one round"


def test_the_defaults_synchronise_everything_but_saturating_noise_and_really_iterate(native):
    each, _ = native
    cases = jc.small_cases()
    got = each("small", [s for _, s, _ in cases], 0, 0)
    iterated = corrected = 0
    for (name, stream, _), rec in zip(cases, got):
        n_subseq, rounds, fell_back = rec["stats"]
        if "noise" not in name:
            assert fell_back == 0, f"{name} fell back at the defaults after {rounds} rounds over {n_subseq} sub-sequences"
        iterated += _subseq(stream, DEFAULT_S)[1] >= 4 and rounds >= 2 and not fell_back
        # Round 1 counts every lane from a segment's third on as changed, so rounds >= 2 holds by construction there.  A frame
        # that converges at round 3 or later had a lane whose exit really differed in round 2: a guess was corrected.
        corrected += rounds >= 3 and not fell_back
    assert iterated >= 5, iterated
    assert corrected >= 3, corrected


def _block_byte_ranges(stream):
    """[(first raw byte, last raw byte)] of every block's bits, by the reference's decoder (tests/jpeg_ref.py)."""
    p = jr.parse(stream)
    tabs = {k: jr._codes(*v) for k, v in p["huff"].items()}
    mx, my, _ = jr.geometry(p)
    out = []
    for begin, end, first in p["segments"]:
        raw = stream[begin:end]
        keep = [i for i in range(len(raw)) if not (raw[i] == 0 and i and raw[i - 1] == 0xFF)]   # unstuffed index -> raw index
        b = jr._Bits(raw.replace(b"\xff\x00", b"\xff"))
        n = min(p["restart"], mx * my - first) if p["restart"] else mx * my
        for _ in range(n):
            for c in range(p["ncomp"]):
                for _ in range(p["hs"] * p["vs"] if c == 0 else 1):
                    start = b.pos
                    s = b.symbol(tabs[(0, p["dc_sel"][c])])
                    if s:
                        b.extend(s)
                    k = 1
                    while k < 64:
                        rs = b.symbol(tabs[(1, p["ac_sel"][c])])
                        if rs & 15 == 0:
                            if rs >> 4 != 15:
                                break
                            k += 16
                            continue
                        k += rs >> 4
                        b.extend(rs & 15)
                        k += 1
                    out.append((begin + keep[start >> 3], begin + keep[(b.pos - 1) >> 3], begin))
    return out


def test_at_16_bytes_a_block_spans_three_sub_sequences(native):
    each, _ = native
    cases = jc.small_cases()
    name, stream, want = next(c for c in cases if c[0] == "17x16_420_q100_noise")
    spans = [(last - begin) // 16 - (first - begin) // 16 for first, last, begin in _block_byte_ranges(stream)]
    assert max(spans) >= 2, "no block of the case reaches into a third 16-byte sub-sequence"
    rec = each("small", [s for _, s, _ in cases], 16, 64)[[c[0] for c in cases].index(name)]
    assert rec["sync"] == 0 and np.array_equal(rec["sync_px"], want)


def _cuts_inside_a_pair(stream, S):
    return [begin + i for begin, end, _ in jr.parse(stream)["segments"] for i in range(S, end - begin, S)
            if stream[begin + i] == 0 and stream[begin + i - 1] == 0xFF]


def test_a_cut_on_the_00_of_a_stuffed_pair_decodes_exactly(native):
    each, _ = native
    cases = jc.small_cases()
    found = [(S, name) for S in (16, 20, 24, 28, 32, 36, 40, 48) for name, stream, _ in cases if _cuts_inside_a_pair(stream, S)]
    assert found, "no golden stream has a stuffed pair across a cut at these sizes"
    for S in sorted({S for S, _ in found}):
        got = each("small", [s for _, s, _ in cases], S, 64)
        for (name, stream, want), rec in zip(cases, got):
            assert rec["sync"] == 0 and np.array_equal(rec["sync_px"], want), (S, name, _cuts_inside_a_pair(stream, S))


def test_bytes_behind_the_last_mcu_are_not_looked_at(native):
    """Non-FF bytes between the last MCU and EOI (encoders pad, cameras append): pr_jpeg_decode stops at the segment's block
    count and so must the sub-sequence decoder, whatever those bytes decode to -- a whole extra sub-sequence of them at 16."""
    each, _ = native
    rng = np.random.default_rng(5)
    cases = [c for c in jc.small_cases() if c[0].startswith(("48x32", "160x120")) and "rst" not in c[0]]
    assert len(cases) >= 8
    tails = [bytes(rng.integers(0, 255, n, dtype=np.uint8)) for n in (1, 3, 40, 200)]          # 0 .. 254: no 0xFF among them
    padded = [(name, stream[:-2] + tails[i % 4] + stream[-2:], px) for i, (name, stream, px) in enumerate(cases)]
    assert all(s[-2:] == b"\xff\xd9" for _, s, _ in padded)
    for S, R in ((0, 0), (16, 64)):
        for (name, stream, want), rec in zip(padded, each("padded", [s for _, s, _ in padded], S, R)):
            assert rec["parse_status"] == 0 and rec["serial"] == 0 and rec["sync"] == 0, (name, S, rec["serial"], rec["sync"])
            assert np.array_equal(rec["serial_px"], want) and np.array_equal(rec["sync_px"], want), (name, S)


@functools.lru_cache(maxsize=None)
def _damaged():
    base = jc.fuzz_base()
    cut, hit = jc.truncations(base), jc.corruptions(base)
    return cut, hit, [jc.reference_verdict(s) for s in hit]


@pytest.mark.parametrize("S,R", [(0, 0), (16, 64)])
def test_truncated_and_corrupted_streams_keep_the_contract(native, S, R):
    """Accepted streams only (which refusal damaged bytes get is the parser's business, tested in test_jpeg_native.py): where
    pr_jpeg_decode ends with status 0 the sub-sequence decoder gives the same pixels and status 0, where it does not, a
    non-zero status -- and the same against the numpy reference's verdict.  The driver runs under the sanitizers."""
    each, _ = native
    cut, hit, verdicts = _damaged()
    assert len(hit) == 2000
    got = each("damaged", cut + hit, S, R)
    assert all(r["parse_status"] != 0 for r in got[:len(cut)]), "a stream without its EOI was accepted"
    accepted = bad = 0
    for i, (want, rec) in enumerate(zip(verdicts, got[len(cut):])):
        if rec["parse_status"] != 0:
            continue
        accepted += 1
        if rec["serial"] == 0:
            assert rec["sync"] == 0, f"corruption {i}: status {rec['sync']} where pr_jpeg_decode has 0"
            np.testing.assert_array_equal(rec["sync_px"], rec["serial_px"], err_msg=f"corruption {i}")
        else:
            assert rec["sync"] != 0, f"corruption {i}: status 0 where pr_jpeg_decode has {rec['serial']}"
        assert not (isinstance(want, str) and want == "refused"), f"corruption {i}: the reference's parser refuses what the library accepts"
        if isinstance(want, str):
            bad += 1
            assert rec["sync"] != 0, f"corruption {i} cannot be decoded but came back with status 0"
        else:
            assert rec["sync"] == 0, f"corruption {i} is a valid stream but came back with status {rec['sync']}"
            np.testing.assert_array_equal(rec["sync_px"], want, err_msg=f"corruption {i}")
    assert accepted >= 200 and bad >= 50, (accepted, bad)


def test_argument_errors_return_invalid_and_write_nothing(native):
    """Null pointers, subseq_bytes 12 / 18 / 8192, max_rounds 0 / 65, a workspace one byte short or misaligned: the driver
    fails unless each returns PR_ERR_INVALID with pixels, status, statistics and workspace untouched."""
    _, args = native
    out = args(jc.fuzz_base())
    assert "0 wrong" in out and int(out.split(":")[1].split()[0]) >= 15, out
