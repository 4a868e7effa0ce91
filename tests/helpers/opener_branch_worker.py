"""Child of tests/test_opener_branch.py: ``PA_F32_DS_FUSE`` is read once per process, so each setting runs in a process of its own.
Traces the exact engine's backbone (``pa_backbone_trace``) around the three blocks that have a 1x1/2 downsample branch -- the
openers (stages 6, 10, 14), the convolutions that add the stored branch (7, 11, 15, with the branch itself) and the features (19)
-- at 1 and 5 crops, where the openers run split K and the branch stays a launch of its own, and at 128 crops, the benchmark's
batch, where the openers of blocks 2 and 3 take the fused kernel. Small batches are saved whole, the large one as SHA-256 digests
of the stored bytes (bit identity is all that is asked of it) plus stages 14 and 15 themselves."""
import hashlib
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from playaid_core_amd import synth
from playaid_core_amd.engine import Engine

STAGES = (6, 7, 10, 11, 14, 15, 19)
BRANCH = (7, 11, 15)
WHOLE_AT_128 = (14, 15)


def main():
    out_path = sys.argv[1]
    res = {}
    eng = Engine(synth.make_state_dict(seed=1234), max_batch_frames=64, max_clip_frames=16, max_frame_height=128, max_frame_width=128,
                 compute_dtype="f32")
    try:
        for n in (1, 5, 128):
            rng = np.random.default_rng(4000 + n)
            x = torch.from_numpy(rng.integers(0, 256, (n, 3, 128, 128)).astype(np.float32) / np.float32(255)).cuda()
            for s in STAGES:
                got = eng.backbone_trace(x, s, aux=True) if s in BRANCH else (eng.backbone_trace(x, s),)
                torch.cuda.synchronize()
                for name, t in zip((f"n{n}_s{s}", f"n{n}_s{s}_aux"), got):
                    a = t.cpu().numpy()
                    if n <= 5 or s in WHOLE_AT_128:
                        res[name] = a
                    res[name + "_sha"] = np.frombuffer(hashlib.sha256(a.tobytes()).digest(), dtype=np.uint8)
                    res[name + "_nonzero"] = np.array(float((a != 0).mean()))
    finally:
        eng.close()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main()
