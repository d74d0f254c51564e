"""Every block of the encoder as the production plan routes it, at production batch sizes, against an fp64 reference
computed from that block's own GPU input (tests/encoder_ref.py): the tap pr_hmr_encode_until gives block k's output with the
forward's sub-batch split, lanes and routing; block k's reference starts from the GPU's tap k - 1, so errors do not
compound and the criterion is elementwise -- |gpu - ref| <= E on every element of every frame -- plus a tile criterion
(no 32-pixel x 32-channel tile's RMS of (gpu - ref) / E above encoder_ref.RHO times its block's)."""
import pytest
import torch

import encoder_ref as er
from conftest import measured
from poserisk_release_amd import synth
from poserisk_release_amd.hmr import HMR

pytestmark = pytest.mark.gpu

CHUNK = 16   # frames per fp64 reference step (a few hundred MB of im2col at layer1)

# (precision, B, max_batch, streams / concurrency, conv_form) -> expected plan_counts(B) on 256 CUs.  bf16: 37 launches
# per sub-batch, 27 where the five plain layer3 blocks take bottleneck256_bf16 (hmr_fused3_pays: b >= 0.85 of whole CU
# rounds; 217 frames miss it, 218 take it; 3 x 85 frames miss it; 600 frames = 512 (two rounds, taken) + 88 (missed) under
# the 512-frame cap).  fp32: 47 launches, 10 of them Winograd layers in the default form, none in "direct".
CONFIGS = {
    "bf16_B256": ("bf16", 256, 256, 1, "default", (27, 0)),
    "bf16_B256_lanes3": ("bf16", 256, 256, 3, "default", (111, 0)),
    "bf16_B217": ("bf16", 217, 217, 1, "default", (37, 0)),
    "bf16_B218": ("bf16", 218, 218, 1, "default", (27, 0)),
    "bf16_B3": ("bf16", 3, 3, 1, "default", (37, 0)),
    "bf16_B600": ("bf16", 600, 600, 1, "default", (64, 0)),
    "fp32_B64_wino": ("fp32", 64, 64, 1, "default", (47, 10)),
    "fp32_B64_direct": ("fp32", 64, 64, 1, "direct", (47, 0)),
    "fp32_B1": ("fp32", 1, 1, 1, "default", (47, 10)),
    # one sub-batch each (fp32 has no batch-dependent routing: 47 launches, 10 Winograd layers): 37 frames = whole rounds + a
    # quarter tail + a ragged last tile in layer2.0's and layer3.0's conv3 + downsample, layer3.0's conv1 and layer4's Winograd GEMMs
    # (tests/test_launch_geometry.py); 256 = the configs[3] slice
    "fp32_B37": ("fp32", 37, 37, 1, "default", (47, 10)),
    "fp32_B256": ("fp32", 256, 256, 1, "default", (47, 10)),
}

_REFS = {}


def _reference(precision, dev):
    if precision not in _REFS:
        _REFS[precision] = er.Reference(synth.hmr_state_dict(seed=1), precision, dev)
    return _REFS[precision]


def _nchw(t):
    return t.permute(0, 3, 1, 2).double()


@pytest.mark.parametrize("name", list(CONFIGS))
def test_encoder_blocks_match_fp64_reference(gpu_device, name):
    precision, B, cap, lanes, form, counts = CONFIGS[name]
    assert torch.cuda.get_device_properties(gpu_device).multi_processor_count == 256   # the routing thresholds above
    m = HMR(max_batch=cap, precision=precision, conv_form=form).to(gpu_device)
    m.load_state_dict(synth.hmr_state_dict(seed=1))
    if lanes > 1:
        m.set_streams(lanes)
        m.set_concurrency(lanes)
    assert m.plan_counts(B) == counts
    wino = m.conv_form_resolved() if precision == "fp32" else 0
    assert (wino != 0) == (form == "default" and precision == "fp32")
    ref = _reference(precision, gpu_device)
    x = torch.rand((B, 3, 224, 224), device=gpu_device, generator=torch.Generator(device=gpu_device).manual_seed(7))
    with torch.no_grad():
        prev = None
        for k in range(17):
            tap = m.encode_until(x, k)
            assert torch.equal(tap, m.encode_until(x, k)), f"block {k}: two runs differ"
            assert tap.dtype == (torch.bfloat16 if precision == "bf16" else torch.float32)
            assert tap.shape == (B,) + (HMR.BLOCK_SHAPES[k][0],) * 2 + (HMR.BLOCK_SHAPES[k][1],)
            st = er.Stats()
            for f0 in range(0, B, CHUNK):
                if k == 0:
                    y, E = ref.block0(x[f0:f0 + CHUNK])
                else:
                    y, E = ref.block(k, _nchw(prev[f0:f0 + CHUNK]), wino)
                st.add(_nchw(tap[f0:f0 + CHUNK]), y, E)
            measured(f"{name} block {k}: max |gpu - ref| / E", st.max_r, 1.0)
            measured(f"{name} block {k}: max tile RMS of r / block RMS", st.tile_ratio, er.RHO)
            assert st.max_r <= 1.0, (k, st.max_r)
            assert st.tile_ratio <= er.RHO, (k, st.tile_ratio)
            prev = tap
        xf = m(x, return_features=True)[3]
        ref_f, E_f = er.pool_ref(_nchw(prev))
        rf = float(er.ratios(xf.double(), ref_f, E_f).max())
        measured(f"{name} pooled features: max |gpu - ref| / E", rf, 1.0)
        assert rf <= 1.0, rf


# 218: the smallest batch at which layer3's plain blocks take the whole-block alternate on 256 CUs (CONFIGS above)
@pytest.mark.parametrize("precision,B", [("fp32", 1), ("bf16", 3), ("bf16", 218)])
def test_profile_brackets_every_launch_once(gpu_device, precision, B):
    """Profile mode: one event bracket per launch of the plan -- the ordinary entries and layer3's alternate alike -- summed
    per layer by profile_read, which also clears them; the forward computes the same bits with the brackets around it."""
    assert torch.cuda.get_device_properties(gpu_device).multi_processor_count == 256
    m = HMR(max_batch=B, precision=precision).to(gpu_device)
    m.load_state_dict(synth.hmr_state_dict(seed=1))
    x = torch.rand((B, 3, 224, 224), device=gpu_device, generator=torch.Generator(device=gpu_device).manual_seed(7))
    with torch.no_grad():
        plain = m(x, return_features=True)
        m.profile_enable(True)
        profiled = m(x, return_features=True)
    ms, launches, _ = m.profile_read()
    assert int(launches.sum()) == m.plan_counts(B)[0]
    assert (ms[launches > 0] > 0).all() and not ms[launches == 0].any()
    again_ms, again_launches, _ = m.profile_read()
    assert not again_ms.any() and not again_launches.any()
    m.profile_enable(False)
    assert len(plain) == len(profiled) == 5 and all(torch.equal(a, b) for a, b in zip(plain, profiled))
