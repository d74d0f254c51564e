"""One of two ranks sharing one GPU (tests/test_smooth_gpu.py starts two of these): score_frames with the smoothing knobs on,
first alone, then as a rank of a gloo group of two; the two results must be the same bits.
usage: smooth_ranks_child.py <repository> <port> <rank>"""
import sys
import types

sys.path.insert(0, sys.argv[1])
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from poserisk_release_amd import dropin, synth  # noqa: E402

dropin.install()
from core import base  # noqa: E402
from models import hmr  # noqa: E402
from smpl import SMPL  # noqa: E402

rank = int(sys.argv[3])
dev = torch.device("cuda", 0)                      # rehearsal: both ranks share the one GPU of the box
model = hmr()
model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=dev)
args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1, lanes=2,
                             smooth_median_radius=1, smooth_sigma=1.0)
pred = base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=2)
rng = np.random.default_rng(9)
frames = rng.integers(0, 256, (9, 240, 320, 3), dtype=np.uint8)
tr = {8: {'bbox': np.stack([np.array([160 + 3 * i, 120 - 2 * i, 90, 180], np.float32) for i in range(7)]),
          'frames': np.array([1, 2, 3, 4, 5, 6, 8])}}
whole = pred.score_frames(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True)      # no process group yet: all 7 frames here
plain = base.Predictor(types.SimpleNamespace(**dict(vars(args), smooth_median_radius=0, smooth_sigma=0.0)), spin_model=model,
                       smpl_model=smpl, batch_size=2).score_frames(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True)
assert not np.array_equal(whole["rotmat"], plain["rotmat"]) and not np.array_equal(whole["result"], plain["result"])
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + sys.argv[2], rank=rank, world_size=2)
part = pred.score_frames(frames, tr, synth.EXAMPLE_INFO, with_smpl_params=True)       # 3 + 4 frames, one gather, then smoothed
for k in ("result", "joint_cam", "debug_result", "rotmat", "betas", "cam"):
    assert part[k].shape == whole[k].shape and np.array_equal(part[k], whole[k]), k
assert np.array_equal(part["smooth"]["status"], whole["smooth"]["status"]) and np.array_equal(part["smooth"]["replaced"], whole["smooth"]["replaced"])
for k in ("reba", "rula"):
    assert np.array_equal(np.array(part[k][0], float), np.array(whole[k][0], float), equal_nan=True), k   # top-10 % is NaN for N < 10
    assert np.array_equal(part[k][1], whole[k][1]), k
dist.destroy_process_group()
print("ok")
