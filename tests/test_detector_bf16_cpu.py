"""The bf16 detector without a GPU (include/poserisk_hip.h, section j8, paragraph "bf16"): the shipped library's fold + pack bit
for bit against numpy on the full table and on truncated ones, its refusals by name, the new symbols, the knob's plumbing, and
the GPU tests' checker (tests/det_bf16_ref.py) proving itself on the emulation's own tensors."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import det_bf16_ref as br
import det_cases as dc
import det_ref
from conftest import REPO
from poserisk_release_amd import _lib, detector
from test_detector_bf16_native import special_body

NEW_SYMBOLS = ("pr_det_packed_bytes_bf16", "pr_det_fold_pack_bf16", "pr_det_create_p", "pr_det_precision", "pr_det_elem_bytes",
               "pr_det_conv_nhwc_bf16")


def test_rounding_rules_of_the_reference_itself():
    f = lambda *bits: np.array(bits, np.uint32).view(np.float32)
    assert br.bf16_bits(f(0x3f808000, 0x3f818000, 0x3f808001, 0x7f7fffff, 0x7f800001, 0x80000000)).tolist() == \
        [0x3f80, 0x3f82, 0x3f81, 0x7f80, 0x7fc0, 0x8000]
    # float64 straight to bf16: a value a hair above a tie that float32 would first round ONTO the tie goes up, not to even
    tie = float(f(0x3f808000)[0])
    assert br.bf16_round_f64(np.array([tie, tie + 2.0 ** -40, tie - 2.0 ** -40])).tolist() == [1.0, 1.0078125, 1.0]
    assert br.ulp_step(np.array([1.0, -1.0, 0.0], np.float32), 1).tolist() == [1.0078125, -0.99609375, float(f(0x00010000)[0])]


@pytest.mark.parametrize("n_layers", (1, 2, 5, 83, 107))
def test_the_shipped_library_folds_and_packs_bf16_like_numpy(n_layers):
    """Ties in both directions, a NaN and an overflow to infinity sit in the last convolution's weights (at 83 and 107 a head
    convolution, which has no BatchNorm: the ties reach the rounding as they are)."""
    layers = detector.yolo_layers()[:n_layers]
    body = special_body(layers, 20 + n_layers)
    got = detector.fold_pack_bf16(body, n_layers)
    want, used = br.numpy_fold_pack_bf16(body, layers, 1e-5)
    assert used == body.size and got.size == want.size == _lib.load().pr_det_packed_bytes_bf16(n_layers)
    assert np.array_equal(got, want), f"{int((got != want).sum())} of {got.size} packed bytes differ"
    if n_layers in (83, 107):      # the specials came through un-scaled: tie down, tie up, ..., NaN, +inf, -inf
        cin = layers[-2]["cin"]                     # the head convolution is 1 x 1: kpad = cin; its last real row is 254 of 256
        w = got[-(256 * cin * 2):].view(np.uint16).reshape(256, cin)
        assert w[254, cin - 9:].tolist() == [0x3f80, 0x3f82, 0x3f81, 0x3f81, 0xbf80, 0xbf82, 0x7fc0, 0x7f80, 0xff80]
        assert not w[255].any()


def test_the_bf16_pack_refuses_by_name():
    lib = _lib.load()
    body = np.zeros(lib.pr_det_weight_floats(2), np.float32)
    out = np.zeros(lib.pr_det_packed_bytes_bf16(2), np.uint8)
    call = lambda n, w, nw, eps, o, no: lib.pr_det_fold_pack_bf16(n, w, nw, eps, o, no)
    cases = (((0, body.ctypes.data, body.size, 1e-5, out.ctypes.data, out.size), "n_layers = 0"),
             ((108, body.ctypes.data, body.size, 1e-5, out.ctypes.data, out.size), "n_layers = 108"),
             ((2, None, body.size, 1e-5, out.ctypes.data, out.size), "null weights_host"),
             ((2, body.ctypes.data, body.size, 1e-5, None, out.size), "null packed_host"),
             ((2, body.ctypes.data, body.size - 1, 1e-5, out.ctypes.data, out.size), "n_floats = "),
             ((2, body.ctypes.data, body.size, 1e-5, out.ctypes.data, out.size - 2), "packed_bytes = "),
             ((2, body.ctypes.data, body.size, 0.0, out.ctypes.data, out.size), "bn_eps = 0"))
    for args, name in cases:
        with pytest.raises(_lib.PoseRiskHipError, match=re.escape("pr_det_fold_pack_bf16: " + name)):
            _lib.check(call(*args), "pr_det_fold_pack_bf16")
    assert lib.pr_det_packed_bytes_bf16(0) == 0 and lib.pr_det_packed_bytes_bf16(108) == 0
    assert lib.pr_det_precision(None) == -1 and lib.pr_det_elem_bytes(None, 0) == 0


def test_new_symbols_are_declared_bound_and_exported():
    hdr = open(os.path.join(REPO, "include", "poserisk_hip.h")).read()
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert re.search(r"\b" + name + r"\s*\(", hdr) and name in _lib.SIGNATURES and hasattr(lib, name), name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1]
    assert lib.pr_abi_version() == _lib.ABI_VERSION      # functions were added: no ABI bump


def test_the_knob_is_plumbed_and_refuses_other_values(tmp_path):
    import subprocess
    import sys
    assert detector.check_precision("fp32") == 0 and detector.check_precision("bf16") == 1
    with pytest.raises(ValueError, match="'fp16' unknown: one of 'fp32', 'bf16'"):
        detector.check_precision("fp16")
    from poserisk_release_amd import frontend
    with pytest.raises(ValueError, match="one of 'fp32', 'bf16'"):
        frontend.track(str(tmp_path / "none.y4m"), "none.weights", precision="fp16")
    (tmp_path / "bf16.yaml").write_text("TRACKER: {precision: bf16}\n")
    code = ("from poserisk_release_amd import dropin; dropin.install(); from core.config import cfg; "
            "print('PRECISION', cfg.TRACKER.precision, cfg.TRACKER.batch)")
    env = {k: v for k, v in os.environ.items() if k != "POSERISK_CFG"}
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, env=env, cwd=REPO)
    assert r.returncode == 0 and "PRECISION fp32 8" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=300, cwd=REPO,
                       env=dict(env, POSERISK_CFG=str(tmp_path / "bf16.yaml")))
    assert r.returncode == 0 and "PRECISION bf16 8" in r.stdout, (r.stdout[-500:], r.stderr[-2000:])


# ---- the checker proves itself ------------------------------------------------------------------------------------------------------
SIZE = (32, 64)
CHECKED = (0, 1, 4, 81, 82, 85, 86, 87)


@pytest.fixture(scope="module")
def emulation():
    x = det_ref.letterbox(dc.frames(7, 1, SIZE[0] - 9, SIZE[1] + 11), *SIZE)
    outs = br.forward(dc.weights(), x, torch.float32, until=max(CHECKED))
    outs[-1] = x
    return outs


def test_the_checker_passes_the_emulations_own_tensors(emulation):
    for l in CHECKED:
        err, t = br.check_layer(l, emulation[l], emulation)
        assert err <= 0.01 * float(np.abs(emulation[l]).max()) + t, (l, err, t)
    for l in range(max(CHECKED) + 1):      # what is stored holds the contract's formats
        v = emulation[l]
        if l not in br.FP32_LAYERS:
            assert np.array_equal(br.bf16_round(v.astype(np.float32)).astype(np.float64), v), l


@pytest.mark.parametrize("l", (1, 4, 87))
def test_the_checker_names_an_element_one_ulp_beyond_the_band(emulation, l):
    want = br.layer_from_inputs(l, emulation, accumulate=torch.float64)
    t = 4 * float(np.abs(br.layer_from_inputs(l, emulation, accumulate=torch.float32) - want).max())
    i = tuple(np.array(want.shape) // 2)
    for edge, step in ((br.bf16_round_f64(want + t), 1), (br.bf16_round_f64(want - t), -1)):
        moved = emulation[l].copy()
        moved[i] = edge[i]                                   # on the band's edge: still inside
        br.check_layer(l, moved, emulation)
        moved[i] = float(br.ulp_step(np.array([edge[i]], np.float32), step)[0])
        with pytest.raises(AssertionError, match=re.escape(f"first {list(i)}")):
            br.check_layer(l, moved, emulation)


def test_the_checker_fails_a_route_with_its_halves_swapped(emulation):
    got = emulation[86]
    ca = emulation[85].shape[-1]
    swapped = np.concatenate([got[..., ca:], got[..., :ca]], axis=-1)
    assert swapped.shape == got.shape
    with pytest.raises(AssertionError, match="layer 86: .* not the bits of the sources"):
        br.check_layer(86, swapped, emulation)
    up = emulation[85].copy()
    up[0, 0, 1] = up[0, 1, 0] + 1.0
    with pytest.raises(AssertionError, match="layer 85"):
        br.check_layer(85, up, emulation)
