"""Routing of layer1's 3x3 convolutions to the one-launch Winograd kernel and the executed multiply-adds they report, on
the CPU: tests/native/wino_layer1_plan.cc builds the fp32 plan from the synthetic blob under a given environment.

Pinned: a routed conv2 at 56x56 executes 14 tile rows x 16 B columns (14 tiles + 2 idle) = 224 tiles x 36 products x
64 x 64 multiply-adds per frame (+ conv3's 56 x 56 x 256 x 64 where it rides behind); an unrouted one its direct count
56 x 56 x 64 x 576.  POSERISK_WINO_LAYER1 routes by BLOCK (1 = layer1.0 only, also when conv3 is not fused), never by what
happens to be a launch of its own."""
import pytest

import host_build
from poserisk_release_amd import synth, weights

WINO = 224 * 36 * 64 * 64
DIRECT = 56 * 56 * 64 * 576
CONV3 = 56 * 56 * 256 * 64


@pytest.fixture(scope="module")
def plan_exe(tmp_path_factory):
    d = tmp_path_factory.mktemp("wino_layer1_plan")
    exe = host_build.build(d, "wino_layer1_plan", "wino_layer1_plan.cc", sources=("host_plan.cc",), strict=True, sanitize=False,
                           without_compiler="skip")
    weights.flatten_state_dict(synth.hmr_state_dict(seed=1)).tofile(str(d / "blob.f32"))
    return exe, str(d / "blob.f32")


def _plan(plan_exe, form=-1, **env):
    exe, blob = plan_exe
    r = exe.run(blob, form, env=env)          # the child's only POSERISK_* switches are the ones given here
    lines = r.stdout.strip().splitlines()
    convs = [tuple(int(v) for v in l.split()) for l in lines[:-1]]      # (layer, routed, N3, executed MACs)
    return convs, tuple(int(v) for v in lines[-1].split()[1:])


def test_default_routes_layer1_0_and_counts_224_tiles(plan_exe):
    convs, counts = _plan(plan_exe)
    assert counts == (47, 10)
    assert [(c[1], c[2]) for c in convs] == [(1, 0), (0, 256), (0, 256)]
    assert convs[0][3] == WINO                                   # 14 x 16 tiles, not 14 x 14 and not 14 x 29
    assert convs[1][3] == convs[2][3] == DIRECT + CONV3
    assert _plan(plan_exe, POSERISK_WINO_LAYER1="1") == (convs, counts)


def test_switch_values_and_forms(plan_exe):
    convs, counts = _plan(plan_exe, POSERISK_WINO_LAYER1="2")
    assert counts == (47, 10)
    assert [c[1] for c in convs] == [1, 1, 1]
    assert [c[3] for c in convs] == [WINO, WINO + CONV3, WINO + CONV3]
    convs, counts = _plan(plan_exe, POSERISK_WINO_LAYER1="0")
    assert counts == (47, 10) and [c[1] for c in convs] == [0, 0, 0] and convs[0][3] == DIRECT
    for form, want in [(0, [0, 0, 0]), (244, [0, 0, 0]), (4, [1, 0, 0]), (455, [1, 0, 0]), (505, [1, 0, 0]), (2, [0, 0, 0])]:
        convs, _ = _plan(plan_exe, form=form)
        assert [c[1] for c in convs] == want, form


def test_switch_routes_by_block_not_by_launch(plan_exe):
    """With conv3 not fused, layer1.1's and layer1.2's conv2 are launches of their own: value 1 still leaves them direct."""
    convs, counts = _plan(plan_exe, POSERISK_FUSE_CONV3="0")
    assert counts == (49, 10)
    assert [(c[1], c[2]) for c in convs] == [(1, 0), (0, 0), (0, 0)]
    assert [c[3] for c in convs] == [WINO, DIRECT, DIRECT]
    convs, _ = _plan(plan_exe, POSERISK_FUSE_CONV3="0", POSERISK_WINO_LAYER1="2")
    assert [(c[1], c[3]) for c in convs] == [(1, WINO)] * 3
