"""A frame's bits at EVERY batch size: the encoder's kernels choose their launch geometry from the batch (quarter-tile tails,
ragged last tiles, the runs of the persistent kernels, the bf16 routing, the sub-batch split), DESIGN.md 3.1 / 3.1b state
"a frame's bits do not depend on its batch", and sharding across GPUs relies on it -- so the criterion needs no tolerance:
torch.equal with the batches tests/test_encoder_blocks.py verifies against fp64 (fp32: 64 frames, also frame by frame; bf16:
256 frames).

  * dense sweeps: every B in 1 .. 256 as the prefix x[:B] and as the suffix x[256 - B:] of the same 256 crops (the suffix puts
    a frame at another row offset inside its tiles), for fp32 in the default and the direct conv form and for bf16; bf16 up to
    600 frames across the 0.85 x 512 threshold of layer3's frame-per-workgroup kernel and the 512-frame cap of a sub-batch;
    two and three sub-batch streams.  rotmat, betas, cam, the pooled features and pose6d of every frame are compared; a sweep
    does not stop at its first failure but reports every failing B together -- the pattern names the rule.
  * per-block taps (pr_hmr_encode_until) at geometry_classes.COVER_BATCHES, the sizes tests/test_launch_geometry.py shows to
    run every launch-geometry class: bit-equal pooled features cannot quite exclude an early difference that a ReLU masks, and a
    failure above needs a place -- the message names the first differing block, frame, pixel and channel range."""
import time

import pytest
import torch

import geometry_classes as gc
from conftest import measured
from poserisk_release_amd import synth
from poserisk_release_amd.hmr import HMR

pytestmark = pytest.mark.gpu

N = 256
NAMES = ("rotmat", "betas", "cam", "features", "pose6d")
_CACHE = {}


def _crops(dev, n=N):
    if ("x", n) not in _CACHE:
        _CACHE[("x", n)] = torch.rand((n, 3, 224, 224), device=dev, generator=torch.Generator(device=dev).manual_seed(20 + n))
    return _CACHE[("x", n)]


def _model(dev, config, max_batch=N, lanes=1):
    assert torch.cuda.get_device_properties(dev).multi_processor_count == 256      # the geometry classes depend on it
    precision, _, form = gc.CONFIGS[config]
    m = HMR(max_batch=max_batch, precision=("fp32", "bf16")[precision], conv_form=form).to(dev)
    m.load_state_dict(synth.hmr_state_dict(seed=1))
    if lanes > 1:
        m.set_streams(lanes)
        m.set_concurrency(lanes)
    return m


def _forward(m, x):
    with torch.no_grad():
        return [t.reshape(t.shape[0], -1) for t in m(x, return_features=True)]


def _anchor(dev, config):
    """The five outputs of the 256 crops from the batches the fp64 block tests verify: fp32 in four batches of 64, which must
    equal frame-by-frame runs (every 8th frame); bf16 as one batch of 256."""
    if ("anchor", config) in _CACHE:
        return _CACHE[("anchor", config)]
    x = _crops(dev)
    m = _model(dev, config)
    if config == "bf16":
        want = _forward(m, x)
    else:
        parts = [_forward(m, x[i:i + 64]) for i in range(0, N, 64)]
        want = [torch.cat(p) for p in zip(*parts)]
        bad = []
        for i in range(0, N, 8):
            one = _forward(m, x[i:i + 1])
            bad += [(i, name) for name, a, b in zip(NAMES, one, want) if not torch.equal(a[0], b[i])]
        assert not bad, f"{config}: frames alone differ from the same frames in their batch of 64: {bad}"
    assert all(bool(torch.isfinite(t).all()) for t in want) and float(want[3].abs().max()) > 0
    _CACHE[("anchor", config)] = want
    return want


def _sweep(m, x, want, batches, tag):
    """Runs x[:B] and x[n - B:] for every B and returns the failures, all of them: (B, "prefix" | "suffix", outputs that differ,
    first differing frame of the batch)."""
    n = x.shape[0]
    bad = []
    t0 = time.perf_counter()
    for B in batches:
        for side, lo in (("prefix", 0), ("suffix", n - B)):
            got = _forward(m, x[lo:lo + B])
            diff = [(name, int((g != w[lo:lo + B]).any(dim=1).nonzero()[0])) for name, g, w in zip(NAMES, got, want)
                    if not torch.equal(g, w[lo:lo + B])]
            if diff:
                bad.append((B, side, [d[0] for d in diff], min(d[1] for d in diff)))
    measured(f"batch sweep {tag}: wall time of {2 * len(batches)} forwards", time.perf_counter() - t0, None, "s")
    measured(f"batch sweep {tag}: batches with a differing frame", len(bad), 0)
    return bad


def _report(tag, bad):
    sizes = sorted({b[0] for b in bad})
    return f"{tag}: {len(sizes)} batch sizes give a frame other bits than its verified batch: B = {sizes}; first entries {bad[:12]}"


@pytest.mark.parametrize("config", list(gc.CONFIGS))
def test_every_batch_size_up_to_256_gives_the_verified_bits(gpu_device, config):
    want = _anchor(gpu_device, config)
    m = _model(gpu_device, config)
    bad = _sweep(m, _crops(gpu_device), want, range(1, N + 1), config)
    assert not bad, _report(config, bad)


# 257 .. 600 in steps of 8 plus both sides of 0.85 x 512 = 435.2 (hmr_fused3_pays for two rounds of CUs) and of the 512-frame cap
BF16_BIG = sorted(set(range(257, 601, 8)) | {434, 435, 436, 511, 512, 513, 600})


def test_bf16_batches_up_to_600_give_the_verified_bits(gpu_device):
    x = _crops(gpu_device, 600)
    m256 = _model(gpu_device, "bf16")
    a, b, c = _forward(m256, x[:256]), _forward(m256, x[256:512]), _forward(m256, x[344:])
    for name, tb, tc in zip(NAMES, b, c):
        assert torch.equal(tb[88:], tc[:168]), f"{name}: frames 344 .. 511 differ between two batches of 256"
    want = [torch.cat([ta, tb, tc[168:]]) for ta, tb, tc in zip(a, b, c)]
    del m256
    m = _model(gpu_device, "bf16", max_batch=600)
    assert m.plan_counts(435) == (37, 0) and m.plan_counts(436) == (27, 0) and m.plan_counts(600) == (64, 0)   # as tests/test_encoder_blocks.py derives them
    bad = _sweep(m, x, want, BF16_BIG, "bf16 257..600")
    assert not bad, _report("bf16, 257 .. 600 frames", bad)


# every B up to 16 (fewer frames than streams, shares of 0 / 1 / 2 frames, unequal shares), then every 7th
STREAM_BATCHES = list(range(1, 17)) + list(range(23, N + 1, 7))


@pytest.mark.parametrize("lanes", [2, 3])
@pytest.mark.parametrize("config", ["fp32_default", "bf16"])
def test_sub_batch_streams_give_the_verified_bits(gpu_device, config, lanes):
    want = _anchor(gpu_device, config)
    m = _model(gpu_device, config, lanes=lanes)
    bad = _sweep(m, _crops(gpu_device), want, STREAM_BATCHES, f"{config} {lanes} streams")
    assert not bad, _report(f"{config}, {lanes} sub-batch streams", bad)


def _locate(tap, want):
    """First differing element of two NHWC taps -> frame, pixel, the channel range that differs at that pixel, and how many
    elements differ in all."""
    ne = tap != want
    f, y, x_, _ = (int(v) for v in ne.nonzero()[0])
    ch = ne[f, y, x_].nonzero().flatten()
    return f"frame {f}, pixel ({y}, {x_}), channels {int(ch[0])} .. {int(ch[-1])} ({int(ne.sum())} elements differ)"


@pytest.mark.parametrize("config", list(gc.CONFIGS))
def test_block_taps_at_the_class_covering_batch_sizes(gpu_device, config):
    x = _crops(gpu_device)
    m = _model(gpu_device, config)
    bad = {}      # (B, side) -> its first differing block
    t0 = time.perf_counter()
    with torch.no_grad():
        for k in range(17):
            if config == "bf16":
                want = m.encode_until(x, k)
            else:
                want = torch.cat([m.encode_until(x[i:i + 64], k) for i in range(0, N, 64)])
            for B in gc.COVER_BATCHES:
                for side, lo in (("prefix", 0), ("suffix", N - B)):
                    if (B, side) in bad:
                        continue
                    tap = m.encode_until(x[lo:lo + B], k)
                    if not torch.equal(tap, want[lo:lo + B]):
                        bad[(B, side)] = f"block {k}: {_locate(tap, want[lo:lo + B])}"
            del want
    measured(f"block taps {config}: wall time", time.perf_counter() - t0, None, "s")
    assert not bad, f"{config}: first differing block per batch: {bad}"
