"""The handles' and the stand-alone entries' OWN device buffers between guards (POSERISK_FENCE; csrc/fence.h, DESIGN.md "The
internal fence"), head- and tail-aligned.

tests/test_guard_band_gpu.py fences the tensors a caller hands in.  The kernels that matter most run in workspaces the
library allocates itself: the encoder's activation buffers, sized for the largest map times the handle's capacity whatever
the layer and the batch, so that megabytes of finite stale data lie behind every tensor; the Winograd V / M array and the
split-K slab, sized as maxima likewise; packed weights, biases and regressor / SMPL workspaces, exact-size with unknown
neighbours.  A ragged last tile's rows >= M, a halo lane below the last frame's last row, the stride-2 second source's last
pixel or a persistent kernel's last unit that leaves its tensor there goes unnoticed by every value test.

With the switch set each of those allocations is guard | payload | guard, all 0xFF bytes (NaN as fp32 and bf16) before use; in
mode 2 every tensor in a buffer that is sized as a maximum ENDS on the payload's last byte, so the guard behind it is sharp for
every layer at every B, in mode 1 it starts on the first and the guard in front is.  Every test here: set the switch, create
the handle, run, pr_fence_check() == 0 after each call (a failure prints the report: buffer, side, byte range), outputs finite
and bit for bit those of a handle created with the switch unset -- placement must not change arithmetic, and a wrong tail
offset fails here rather than silently testing nothing.  No tolerance anywhere: every comparison is exact.

Out of reach still: a read whose value is discarded, an access further away than a guard, and the split-K tickets, which stay
head-aligned in both modes (guard_band.py's docstring)."""
import ctypes as C
import time

import numpy as np
import pytest
import torch

import geometry_classes as gc
import kernel_refs as kr
import test_guard_band_gpu as tg
from conftest import measured
from poserisk_release_amd import _lib, ops, synth
from poserisk_release_amd.hmr import HMR
from poserisk_release_amd.pipeline import FramePipeline
from poserisk_release_amd.smpl_layer import SMPLLayer

pytestmark = pytest.mark.gpu

F32, BF16 = torch.float32, torch.bfloat16
MODES = {"head": "1", "tail": "2"}
HMR_NAMES = ("rotmat", "betas", "cam", "xf", "pose6d")
_CACHE = {}


def fence_check():
    """-> (damaged guard regions, report) of pr_fence_check."""
    buf = C.create_string_buffer(1 << 16)
    n = _lib.load().pr_fence_check(buf, len(buf))
    return n, buf.value.decode("utf-8", "replace")


def fence_names():
    """-> {name: (payload bytes, guard bytes)} of the live fenced allocations (pr_fence_list)."""
    buf = C.create_string_buffer(1 << 18)
    n = _lib.load().pr_fence_list(buf, len(buf))
    rows = [line.split("\t") for line in buf.value.decode().splitlines()]
    assert len(rows) == n
    return {r[0]: (int(r[1]), int(r[2])) for r in rows}


def assert_fence_intact(what):
    n, report = fence_check()
    assert n == 0, f"{what}: {n} guard regions of the library's own buffers were written\n{report}"


def _set_mode(mp, mode):
    if mode is None:
        mp.delenv("POSERISK_FENCE", raising=False)
    else:
        mp.setenv("POSERISK_FENCE", MODES[mode])


def _hmr(dev, mp, mode, precision, form="default", max_batch=4, streams=0):
    """A handle created (now, not at its first forward) with the switch at `mode` (None = unset)."""
    _set_mode(mp, mode)
    m = HMR(max_batch=max_batch, precision=precision, conv_form=form).to(dev)
    m.load_state_dict(_sd())
    if streams:
        m.set_streams(streams)
    m._ensure(max_batch)
    if mode is not None:
        names = fence_names()
        assert "act[0][0]" in names and "act[0][5]" in names and "xf" in names and "conv 0 weights" in names, sorted(names)[:20]
        assert all(g >= 65536 and g % 4096 == 0 for _, g in names.values())
        assert not [n for n in names if n.startswith("plan ")], "a plan constant kept its placeholder name"
    return m


def _sd():
    if "sd" not in _CACHE:
        _CACHE["sd"] = synth.hmr_state_dict(seed=1)
    return _CACHE["sd"]


def _crops(dev, n):
    if ("x", n) not in _CACHE:
        _CACHE[("x", n)] = torch.rand((n, 3, 224, 224), device=dev, generator=torch.Generator(device=dev).manual_seed(20 + n))
    return _CACHE[("x", n)]


def _forward(m, x):
    with torch.no_grad():
        return [t.reshape(t.shape[0], -1) for t in m(x, return_features=True)]


def _assert_same(got, want, what):
    for name, g, w in zip(HMR_NAMES, got, want):
        assert bool(torch.isfinite(g).all()), f"{what}: {name} is not finite under the fence (a value from a 0xFF guard or from stale 0xFF slack took part)"
        assert torch.equal(g, w), f"{what}: {name} differs from the unfenced handle's ({int((g != w).any(dim=1).sum())} frames)"


def _unfenced(dev, key, make, batches, x):
    """The outputs of an unfenced handle at every B of `batches`, computed once per `key`."""
    if key not in _CACHE:
        with pytest.MonkeyPatch.context() as mp:
            before = fence_names()
            m = make(mp)
            assert fence_names() == before, "the unfenced handle recorded allocations"
            _CACHE[key] = {B: _forward(m, x[:B]) for B in batches}
            del m
    return _CACHE[key]


def _timed(tag, t0):
    measured(f"internal fence {tag}: wall time", time.perf_counter() - t0, None, "s")


# ------------------------------------------------------------------------------------------------
# the fence itself
# ------------------------------------------------------------------------------------------------
def test_fence_selftest_and_nothing_recorded_with_the_switch_off(gpu_device, monkeypatch):
    lib = _lib.load()
    assert lib.pr_fence_selftest() == 0, lib.pr_last_error()
    assert fence_check() == (0, "")
    before = fence_names()
    m = _hmr(gpu_device, monkeypatch, None, "fp32")
    out = _forward(m, _crops(gpu_device, 3))
    assert all(bool(torch.isfinite(t).all()) for t in out)
    assert fence_names() == before and fence_check() == (0, "")
    del m


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
@pytest.mark.parametrize("mode", list(MODES))
def test_the_modes_place_the_tensors_where_they_say(gpu_device, monkeypatch, mode, precision):
    """One frame through a handle for four: no tensor is larger than one frame of the largest map, so in tail mode all but the
    last frame's worth of every activation buffer is never written (still 0xFF) counted from its START, in head mode from its
    END -- a tail offset that was not applied, or applied in head mode, shows here rather than testing nothing above."""
    m = _hmr(gpu_device, monkeypatch, mode, precision)
    _forward(m, _crops(gpu_device, 3)[:1])
    lib, names = _lib.load(), fence_names()
    es = 2 if precision == "bf16" else 4
    assert names["act[0][1]"][0] == 4 * 112 * 112 * 64 * es and names["act[0][0]"][0] == 4 * 224 * 224 * 16
    used = 0
    for name in [f"act[0][{i}]" for i in range(6)] + (["wino_work[0]"] if precision == "fp32" else []):
        lead, trail = C.c_size_t(0), C.c_size_t(0)
        _lib.check(lib.pr_fence_payload_fill(name.encode(), C.byref(lead), C.byref(trail)), "pr_fence_payload_fill")
        cap = names[name][0]
        untouched, other = (lead.value, trail.value) if mode == "tail" else (trail.value, lead.value)
        assert cap % 4 == 0 and untouched >= cap - cap // 4, f"{name} ({mode}): {untouched} of {cap} bytes untouched at the far end"
        if untouched < cap:      # (a buffer no launch of this plan uses stays 0xFF throughout: act[0][1] behind the fused stem)
            assert other < cap // 4, f"{name} ({mode}): {other} bytes untouched at the near end"
            used += 1
    assert used >= 5
    assert_fence_intact(f"{precision} {mode} one frame of four")
    del m


# ------------------------------------------------------------------------------------------------
# the encoder as routed: every launch-geometry class up to 256 frames, both alignments
# ------------------------------------------------------------------------------------------------
SWEEP = tuple(sorted(gc.ANCHORED + gc.COVER_BATCHES))


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("config", list(gc.CONFIGS))
def test_encoder_as_routed(gpu_device, monkeypatch, config, mode):
    t0 = time.perf_counter()
    precision, _, form = gc.CONFIGS[config]
    prec = ("fp32", "bf16")[precision]
    x = _crops(gpu_device, 256)
    want = _unfenced(gpu_device, ("sweep", config), lambda mp: _hmr(gpu_device, mp, None, prec, form, 256), SWEEP, x)
    m = _hmr(gpu_device, monkeypatch, mode, prec, form, 256)
    for B in SWEEP:
        got = _forward(m, x[:B])
        assert_fence_intact(f"{config} {mode} B={B}")
        _assert_same(got, want[B], f"{config} {mode} B={B}")
    del m
    assert_fence_intact(f"{config} {mode} after the handle was destroyed")
    _timed(f"encoder {config} {mode}", t0)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("form", ["winograd2", "winograd4"])
def test_other_winograd_forms(gpu_device, monkeypatch, form, mode):
    """F(2x2) and F(4x4) on Lavin & Gray's points: other tile counts, other ragged edges on the 7x7 and 14x14 maps."""
    t0 = time.perf_counter()
    x = _crops(gpu_device, 256)
    want = _unfenced(gpu_device, ("form", form), lambda mp: _hmr(gpu_device, mp, None, "fp32", form, 37), (1, 37), x)
    m = _hmr(gpu_device, monkeypatch, mode, "fp32", form, 37)
    assert "wino_work[0]" in fence_names()
    for B in (1, 37):
        got = _forward(m, x[:B])
        assert_fence_intact(f"{form} {mode} B={B}")
        _assert_same(got, want[B], f"{form} {mode} B={B}")
    del m
    _timed(f"{form} {mode}", t0)


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_sub_batch_streams(gpu_device, monkeypatch, precision, mode):
    """pr_hmr_set_streams(3): every chunk has its own buffers, allocated by set_chunks after the handle was created."""
    t0 = time.perf_counter()
    x = _crops(gpu_device, 256)
    want = _unfenced(gpu_device, ("streams", precision), lambda mp: _hmr(gpu_device, mp, None, precision, "default", 37), (5, 37), x)
    m = _hmr(gpu_device, monkeypatch, mode, precision, "default", 37, streams=3)
    names = fence_names()
    assert all(f"act[{c}][{i}]" in names for c in range(3) for i in range(6)) and "act[3][0]" not in names
    for B in (37, 5):
        got = _forward(m, x[:B])
        assert_fence_intact(f"{precision} 3 streams {mode} B={B}")
        _assert_same(got, want[B], f"{precision} 3 streams {mode} B={B}")
    del m
    _timed(f"streams {precision} {mode}", t0)


@pytest.mark.parametrize("B", [1, 3, 37])
@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_batch_sized_buffers_are_exact(gpu_device, monkeypatch, precision, B):
    """Pooled features, regressor state and fc workspaces are sized by max_batch and not tail-aligned: max_batch == B makes
    them exact-size, so their guards are sharp (head mode; the activation buffers are exact at the largest map only)."""
    t0 = time.perf_counter()
    x = _crops(gpu_device, 256)
    want = _unfenced(gpu_device, ("exact", precision, B), lambda mp: _hmr(gpu_device, mp, None, precision, "default", B), (B,), x)
    m = _hmr(gpu_device, monkeypatch, "head", precision, "default", B)
    names = fence_names()
    assert names["xf"][0] == max(B * 2048, 4) * 4 and names["state"][0] == max(B * 192, 4) * 4 and names["h1"][0] == B * 1024 * 4
    got = _forward(m, x[:B])
    assert_fence_intact(f"{precision} max_batch = B = {B}")
    _assert_same(got, want[B], f"{precision} max_batch = B = {B}")
    del m
    _timed(f"exact {precision} B={B}", t0)


@pytest.mark.parametrize("precision", ["fp32", "bf16"])
def test_encode_until_reads_the_tail_aligned_tap(gpu_device, monkeypatch, precision):
    t0 = time.perf_counter()
    x = _crops(gpu_device, 256)[:3]
    with pytest.MonkeyPatch.context() as mp:
        plain = _hmr(gpu_device, mp, None, precision)
        want = {k: plain.encode_until(x, k) for k in tg.ENCODER_BLOCKS}
        del plain
    m = _hmr(gpu_device, monkeypatch, "tail", precision)
    for k in tg.ENCODER_BLOCKS:
        tap = m.encode_until(x, k)
        assert_fence_intact(f"{precision} tap of block {k}")
        assert bool(torch.isfinite(tap.float()).all()) and torch.equal(tap, want[k]), f"{precision}: the tap of block {k} differs from the unfenced handle's"
    del m
    _timed(f"encode_until {precision}", t0)


# ------------------------------------------------------------------------------------------------
# SMPL and the whole per-batch driver
# ------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def smpl97():
    return synth.smpl_model(V=97, seed=2)


def _smpl_run(layer, dev, B):
    pose, betas = synth.poses(B, seed=40 + B), synth.betas(B, seed=41 + B)
    trans = (np.random.default_rng(B).standard_normal((B, 3)) * 0.2).astype(np.float32)
    v, j = layer(*(torch.from_numpy(a).to(dev) for a in (pose, betas, trans)))
    jc, v2 = layer.joint_cam(torch.from_numpy(pose.reshape(B, 24, 3).copy()).to(dev), return_verts=True)
    return {"verts": v, "joints": j, "joint_cam": jc, "joint_cam verts": v2}


@pytest.mark.parametrize("variant,B", [(v, B) for v in ("skin_tile", "skin_split_waves") for B in (1, 5, 17)] +
                         [("skin_rows", B) for B in (129, 256)])      # pr_smpl_create: max_batch > 128 selects the rows kernel
@pytest.mark.parametrize("mode", list(MODES))
def test_smpl(gpu_device, smpl97, monkeypatch, mode, variant, B):
    _, tile = tg.SMPL_VARIANTS[variant]
    if tile is None:
        monkeypatch.delenv("POSERISK_SMPL_TILE", raising=False)
    else:
        monkeypatch.setenv("POSERISK_SMPL_TILE", tile)
    outs = {}
    for fenced in (None, mode):
        _set_mode(monkeypatch, fenced)
        layer = SMPLLayer(smpl97, device=gpu_device, max_batch=B)      # max_batch == B: the workspaces are as small as they get
        layer._ensure()
        names = fence_names()
        assert ("smpl posedirs_T" in names and "smpl A" in names) == (fenced is not None), sorted(names)
        outs[fenced] = _smpl_run(layer, gpu_device, B)
        if fenced:
            assert_fence_intact(f"SMPL {variant} {mode} B={B}")
        del layer
    for k, t in outs[mode].items():
        assert bool(torch.isfinite(t).all()) and torch.equal(t, outs[None][k]), f"SMPL {variant} {mode} B={B}: {k} differs from the unfenced handle's"
    assert_fence_intact(f"SMPL {variant} {mode} B={B} after the handle was destroyed")


def test_frames_forward(gpu_device, smpl97, monkeypatch):
    """pr_frames_forward through FramePipeline at B = 3, both handles fenced in tail mode."""
    x = _crops(gpu_device, 256)[:3]
    outs = {}
    for fenced in (None, "tail"):
        hmr = _hmr(gpu_device, monkeypatch, fenced, "fp32")
        layer = SMPLLayer(smpl97, device=gpu_device, max_batch=32)
        layer._ensure()
        pipe = FramePipeline(hmr, layer, synth.EXAMPLE_INFO, with_verts=True)
        outs[fenced] = {k: v.clone() for k, v in pipe(x).items() if k != "crop_status"}      # (the one buffer the call does not write)
        torch.cuda.synchronize()
        if fenced:
            names = fence_names()
            assert "act[0][1]" in names and "smpl A" in names
            assert_fence_intact("pr_frames_forward")
        del pipe, hmr, layer
    assert set(outs["tail"]) >= {"rotmat", "betas", "cam", "axis_angle", "euler", "joint_cam", "status", "reba", "rula", "verts"}
    for k, t in outs["tail"].items():
        assert (not t.dtype.is_floating_point or bool(torch.isfinite(t).all())) and torch.equal(t, outs[None][k]), f"pr_frames_forward: {k} differs"
    assert_fence_intact("pr_frames_forward after the handles were destroyed")


# ------------------------------------------------------------------------------------------------
# the stand-alone entries' own copies: packed weights, biases, Winograd work, split-K slab and tickets
# ------------------------------------------------------------------------------------------------
def _conv(cfg, shape, with_res, bf):
    def make(dev):
        x, w, bias, res, _, _ = tg._conv_data(shape, bf)
        dt = BF16 if bf else F32
        xd, rd = x.to(dev, dt), res.to(dev, dt) if with_res else None
        return lambda: ops.conv2d_nhwc(xd, w, bias, rd, stride=shape[6], pad=shape[7], relu=True, tile_cfg=cfg, precision="bf16" if bf else "fp32")[0]
    return make


def _dual(dev):
    B, Ho, C1, C2, N = 1, 5, 64, 128, 64
    rng = np.random.default_rng(7)
    t = torch.from_numpy(rng.standard_normal((B, Ho, Ho, C1)).astype(np.float32)).to(dev)
    x = torch.from_numpy(rng.standard_normal((B, 2 * Ho - 1, 2 * Ho - 1, C2)).astype(np.float32)).to(dev)
    w1 = (rng.standard_normal((N, C1)) / np.sqrt(C1)).astype(np.float32)
    w2 = (rng.standard_normal((N, C2)) / np.sqrt(C2)).astype(np.float32)
    bias = rng.standard_normal(N).astype(np.float32)
    return lambda: ops.conv1x1_dual_nhwc(t, w1, x, w2, bias, stride2=2, relu=True, tile_cfg=8, precision="fp32")


def _fused(dev):
    B, H, Cin, N3 = 1, 5, 32, 64
    rng = np.random.default_rng(8)
    x = torch.from_numpy(rng.standard_normal((B, H, H, Cin)).astype(np.float32)).to(dev)
    w2 = (rng.standard_normal((64, Cin, 3, 3)) / np.sqrt(Cin * 9)).astype(np.float32)
    w3 = (rng.standard_normal((N3, 64)) / 8).astype(np.float32)
    b2, b3 = rng.standard_normal(64).astype(np.float32), rng.standard_normal(N3).astype(np.float32)
    res = torch.from_numpy(rng.standard_normal((B, H, H, N3)).astype(np.float32)).to(dev)
    return lambda: ops.conv3x3_conv1x1_nhwc(x, w2, b2, w3, b3, res, relu=True, precision="fp32")


def _wino64(dev):
    x, w2, b2, w3, b3, res = kr.wino64_layer((2, 5, 5))
    xd, rd = torch.from_numpy(x).to(dev), torch.from_numpy(res).to(dev)
    return lambda: ops.conv3x3_wino64_nhwc(xd, w2, b2, w3, b3, rd, form=5)


def _bottleneck(mid, case, first=False):
    def make(dev):
        x, w1, w2, w3, wd, b = kr.bottleneck_inputs(mid, case, first)
        fn = {64: ops.bottleneck_nhwc, 128: ops.bottleneck128_nhwc, 256: ops.bottleneck256_nhwc}[mid]
        extra = dict(wd=wd.numpy(), bd=b[3]) if first else {}
        xd = x.to(dev, BF16)
        return lambda: fn(xd, w1.numpy(), b[0], w2.numpy(), b[1], w3.numpy(), b[2], **extra)[0]
    return make


def _stem_bf16(dev):
    x, w, bias, _ = kr.stem_pool_bf16_case((5, 2))
    xd = x.to(dev, BF16)
    return lambda: ops.stem_pool_nhwc(xd, w.numpy(), bias)[0]


def _stem_f32(dev):
    x, w, bias, _, _ = kr.stem_pool_f32_case(2)
    xd = torch.from_numpy(x).to(dev)
    return lambda: ops.stem_pool_f32_nhwc(xd, w, bias)[0]


# one case per family, each the smallest shape of its list in tests/test_guard_band_gpu.py
STANDALONE = {
    "tile_f32": _conv(8, (1, 9, 64, 64, 64, 3, 1, 1), True, False),
    "tile_bf16": _conv(13, (1, 9, 64, 64, 64, 3, 1, 1), True, True),
    "split_k": _conv(202, (1, 5, 96, 96, 64, 1, 1, 0), True, False),
    "register_weights": _conv(400, (1, 5, 128, 128, 256, 1, 1, 0), True, False),
    "winograd2": _conv(-2, (2, 9, 64, 64, 192, 3, 1, 1), False, False),
    "winograd4": _conv(-4, (2, 9, 64, 64, 192, 3, 1, 1), False, False),
    "winograd5": _conv(-5, (2, 9, 64, 64, 192, 3, 1, 1), False, False),
    "wino64": _wino64,
    "dual_source": _dual,
    "conv3x3_conv1x1": _fused,
    "bottleneck64": _bottleneck(64, (7, 1, 1)),
    "bottleneck64_first": _bottleneck(64, (7, 1, 1), True),
    "bottleneck128": _bottleneck(128, (7, 1, 1)),
    "bottleneck256": _bottleneck(256, (5, 1, 1)),
    "stem_pool_bf16": _stem_bf16,
    "stem_pool_f32": _stem_f32,
}


@pytest.mark.parametrize("entry", list(STANDALONE))
def test_standalone_entries_own_copies(gpu_device, monkeypatch, entry):
    """The entry frees its copies before it returns: the frees read the guards, pr_fence_check picks up what they found."""
    call = STANDALONE[entry](gpu_device)
    _set_mode(monkeypatch, None)
    want = call()
    assert fence_check() == (0, "")
    _set_mode(monkeypatch, "head")
    got = call()
    assert_fence_intact(f"stand-alone {entry}")
    assert not [n for n in fence_names() if n.startswith("standalone")], "a stand-alone entry left a fenced allocation behind"
    assert bool(torch.isfinite(got.float()).all()) and got.dtype == want.dtype and torch.equal(got, want), f"{entry}: the fenced call's bits differ"
