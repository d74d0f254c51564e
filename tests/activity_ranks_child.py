"""One of two ranks sharing one GPU (tests/test_activity_gpu.py starts two of these): score_frames with the activity knob on,
first alone, then as a rank of a gloo group of two; the two results must be the same bits.
usage: activity_ranks_child.py <repository> <port> <rank>"""
import sys
import types

sys.path.insert(0, sys.argv[1])
import numpy as np  # noqa: E402
import torch  # noqa: E402
import torch.distributed as dist  # noqa: E402

from poserisk_release_amd import dropin, synth  # noqa: E402

dropin.install()
from core import base  # noqa: E402
from core.config import cfg  # noqa: E402
from models import hmr  # noqa: E402
from smpl import SMPL  # noqa: E402

rank = int(sys.argv[3])
dev = torch.device("cuda", 0)                      # rehearsal: both ranks share the one GPU of the box
model = hmr()
model.load_state_dict(synth.hmr_state_dict(seed=1), strict=False)
smpl = SMPL(models={"neutral": synth.smpl_model(V=6890, seed=2)}, device=dev)
cfg.ACTIVITY.update(hold_seconds=0.4, rapid_seconds=0.2, gap_seconds=0.2)        # 4, 2 and 2 frames at 10 fps
args = types.SimpleNamespace(gpu="0", type="REBA,RULA", debug=False, debug_joints="", debug_frame=-1, lanes=2, derive_activity=True)
pred = base.Predictor(args, spin_model=model, smpl_model=smpl, batch_size=2)
rng = np.random.default_rng(9)
frames = rng.integers(0, 256, (9, 240, 320, 3), dtype=np.uint8)
frames[2:9] = frames[2]                            # a still stretch: the same frame under the same box
tr = {8: {'bbox': np.stack([np.array([160, 120, 90, 180], np.float32) for i in range(8)]), 'frames': np.arange(1, 9)}}
whole = pred.score_frames(frames, tr, synth.EXAMPLE_INFO, fps=10.0)      # no process group yet: all 8 frames here
assert whole["activity"]["parameters"]["hold_frames"] == 4 and whole["activity"]["adds"][-1, 0] >= 1
dist.init_process_group("gloo", init_method="tcp://127.0.0.1:" + sys.argv[2], rank=rank, world_size=2)
part = pred.score_frames(frames, tr, synth.EXAMPLE_INFO, fps=10.0)       # 4 + 4 frames, one gather, then one activity call each
for k in ("result", "joint_cam", "debug_result"):
    assert part[k].shape == whole[k].shape and np.array_equal(part[k], whole[k]), k
for k in ("flags", "adds"):
    assert np.array_equal(part["activity"][k], whole["activity"][k]), k
for k in ("reba", "rula"):
    assert np.array_equal(np.array(part[k][0], float), np.array(whole[k][0], float), equal_nan=True), k   # top-10 % is NaN for N < 10
    assert np.array_equal(part[k][1], whole[k][1]), k
dist.destroy_process_group()
print("ok")
