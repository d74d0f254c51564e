"""The batch sizes that, together with the fp64-verified 1 and 64, run every launch-geometry class of the encoder that occurs
up to 256 frames, and the CPU program that derives those classes from the launchers' own rules
(tests/native/launch_geometry.cc over csrc/host_plan.h).  Shared by tests/test_launch_geometry.py, which holds the list to
the rules, and tests/test_encoder_batch_sweep.py, which taps every encoder block at these sizes on the GPU."""
import os

import host_build

ANCHORED = (1, 64)      # checked against fp64 block by block (tests/test_encoder_blocks.py)
# A greedy cover of the classes of the three configurations below over B = 1 .. 256, plus 37 (a "whole rounds + quarter tail +
# ragged last tile" size that tests/test_encoder_blocks.py also checks against fp64), plus 251 (the first size at which layer3.0's
# 3x3 / stride-2 conv runs on the bf16 balanced kernel, with a ragged last 32-row tile).
COVER_BATCHES = (2, 4, 16, 17, 32, 37, 94, 115, 146, 192, 208, 218, 251, 256)

# name -> (precision, conv_form of pr_hmr_create, HMR's conv_form name)
CONFIGS = {"fp32_default": (0, -1, "default"), "fp32_direct": (0, 0, "direct"), "bf16": (1, -1, "default")}


def build(tmp_dir):
    """-> (program, blob file) or None where there is no g++."""
    from poserisk_release_amd import synth, weights
    exe = host_build.build(tmp_dir, "launch_geometry", "launch_geometry.cc", sources=("host_plan.cc",), strict=True, sanitize=False,
                           without_compiler="none")
    if exe is None:
        return None
    blob = os.path.join(str(tmp_dir), "blob.f32")
    weights.flatten_state_dict(synth.hmr_state_dict(seed=1)).tofile(blob)
    return exe, blob


def classes(prog, config, b_first, b_last, max_batch=256, streams=1, concurrency=1):
    """-> {B: set of "<layer family> | <geometry class>" strings} in a clean environment (no POSERISK_* switch)."""
    exe, blob = prog
    precision, form, _ = CONFIGS[config]
    r = exe.run(blob, precision, form, max_batch, streams, concurrency, b_first, b_last)
    out = {}
    for line in r.stdout.splitlines():
        head, rest = line.split(" | ", 1)
        out.setdefault(int(head.split()[1]), set()).add(rest)
    return out
