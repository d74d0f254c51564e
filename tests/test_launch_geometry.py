"""Which launch-geometry classes the encoder runs at which batch size, on the CPU, from the launchers' own rules.

The fp32 kernels choose their launch geometry from the batch: conv_dma_launch cuts the tiles beyond the last whole round of
256 CUs into quarter blocks (conv_tail_split), conv1x1_regw_f32 deals its units to persistent workgroups as contiguous runs
that may cross a channel block (conv_regw_geometry), the row-panel form splits its columns by the panel count
(conv_panel_nsplit).  The bf16 encoder chooses the KERNEL from the batch: the tile index goes by the rows of the launch
(conv_pick_tile_cfg), the evenly dealt kernel takes a layer whose pixel runs are long enough (conv_bal_bf16_pays) and layer3's
plain blocks take a frame-per-workgroup kernel when the frames fill whole rounds of CUs (hmr_fused3_pays).  All of these are
pure functions of csrc/host_plan.h, the kernel choice behind hmr_route, which the forward executes;
tests/native/launch_geometry.cc walks the real plan with hmr_route and prints one class per launch and batch size (its
header describes the classes).

Held here: geometry_classes.COVER_BATCHES together with the fp64-verified sizes 1 and 64 runs EVERY class that occurs for
B = 1 .. 256, per configuration, and the number of classes is pinned -- a new routing rule, or a changed threshold, fails
this test until the list (which tests/test_encoder_batch_sweep.py taps block by block on the GPU) covers it again.

Not modelled: the persistent bf16 kernels that have no rule in host_plan.h (the whole-Bottleneck kernels, expand_res_bf16)
size their grids inside their own launchers.  The dense sweep of tests/test_encoder_batch_sweep.py, which leaves no batch
size out, is what covers them."""
import pytest

import geometry_classes as gc

# distinct "<layer family> | <geometry class>" strings over B = 1 .. 256 (the sub-batch split's class included)
CLASS_COUNTS = {"fp32_default": 136, "fp32_direct": 145, "bf16": 49}


@pytest.fixture(scope="module")
def prog(tmp_path_factory):
    p = gc.build(tmp_path_factory.mktemp("launch_geometry"))
    if p is None:
        pytest.skip("no g++")
    return p


@pytest.mark.parametrize("config", list(gc.CONFIGS))
def test_committed_batches_cover_every_class(prog, config):
    by_b = gc.classes(prog, config, 1, 256)
    assert sorted(by_b) == list(range(1, 257))
    every = set().union(*by_b.values())
    covered = set().union(*(by_b[b] for b in gc.ANCHORED + gc.COVER_BATCHES))
    missing = sorted(every - covered)
    first = {c: min(b for b in by_b if c in by_b[b]) for c in missing}
    assert not missing, f"{config}: classes no committed batch size runs (first B that does): {first}"
    assert len(every) == CLASS_COUNTS[config]
    assert len(set(gc.COVER_BATCHES)) == len(gc.COVER_BATCHES) and all(1 <= b <= 256 for b in gc.COVER_BATCHES)


def test_what_the_two_anchored_sizes_leave_out(prog):
    """At 64 frames no tile launch has a ragged last tile, at one frame no tile launch has whole rounds: "whole rounds +
    quarter tail + ragged last tile" first appears at other sizes, 37 among them."""
    by_b = gc.classes(prog, "fp32_direct", 1, 256)
    tile = lambda b: [c for c in by_b[b] if "| tile " in c]
    assert tile(64) and all(c.endswith("ragged=none") for c in tile(64))
    # (all but layer2.0's conv3 + downsample: 13 x 8 = 104 tiles, one short round of whole tiles)
    assert tile(1) and all("| tile quarters" in c or "| tile whole:one-round" in c for c in tile(1))
    want = "k1 s1 512->256 @28 | tile whole+tail ragged=quarter"        # 37 x 784 rows: 454 x 4 tiles = 7 rounds + 24, 29 008 % 64 = 16
    assert want in by_b[37] and want not in by_b[1] | by_b[64]
    # a Winograd layer's 36 GEMMs on the register-resident-weights kernel: runs that cross channel blocks and GEMMs, partly filled
    # units; layer4's on the tile kernel: each GEMM's ragged tiles land in whole tiles and in the quarter tail
    wino = [c for c in gc.classes(prog, "fp32_default", 37, 37)[37] if "winograd5" in c]
    assert any("regw" in c for c in wino) and all("crosses-block crosses-group ragged=1" in c for c in wino if "regw" in c)
    assert "k3 s1 512->512 @7 | winograd5 xform-ragged=0,0 P%64=1 | tile whole+tail ragged=both" in wino


def test_sub_batch_split_classes(prog):
    assert "split serial 1 equal" in gc.classes(prog, "bf16", 256, 256)[256]
    by_b = gc.classes(prog, "bf16", 1, 16, max_batch=256, streams=3, concurrency=3)
    assert "split serial 1 equal" in by_b[1]                    # one frame: one sub-batch
    assert "split concurrent 2 equal" in by_b[2]
    assert "split concurrent 3 equal" in by_b[6] and "split concurrent 3 unequal" in by_b[7]
    # beyond the 512-frame cap of a sub-batch: serial passes, the last one shorter; layer3's plain blocks go by the pass
    big = gc.classes(prog, "bf16", 600, 600, max_batch=600)[600]
    assert "split serial 2 unequal" in big
    assert "block 1024 @14 | bottleneck256 frame-per-workgroup rounds" in big and "k1 s1 1024->256 @14 | tile cfg12 ragged=1" in big
