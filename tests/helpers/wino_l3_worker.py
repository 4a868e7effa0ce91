"""Child of tests/test_wino_l3_engine.py: ``PA_WINO_L3_SHAPE`` is read once per process, so each form of layer 3's launches runs in
a process of its own. An exact engine of 16 crops (``max_batch_frames=8``) on 128 x 128 frames traces layer 3 (``pa_backbone_trace``
stages 10..13: layer3.0.conv1, layer3.0.conv2 with its stored branch, layer3.1.conv1, layer3.1.conv2) and the stage that feeds it (9) at
16 and at 5 crops."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np
import torch

from playaid_core_amd import synth
from playaid_core_amd.engine import Engine


def main():
    out_path = sys.argv[1]
    res = {}
    eng = Engine(synth.make_state_dict(seed=1234), max_batch_frames=8, max_clip_frames=16, max_frame_height=128, max_frame_width=128,
                 compute_dtype="f32")
    try:
        for n in (16, 5):
            rng = np.random.default_rng(7000 + n)
            x = torch.from_numpy(rng.integers(0, 256, (n, 3, 128, 128)).astype(np.float32) / np.float32(255)).cuda()
            for s in (9, 10, 12, 13):
                res[f"n{n}_s{s}"] = eng.backbone_trace(x, s).cpu().numpy()
            o, a = eng.backbone_trace(x, 11, aux=True)
            res[f"n{n}_s11"], res[f"n{n}_aux11"] = o.cpu().numpy(), a.cpu().numpy()
        torch.cuda.synchronize()
    finally:
        eng.close()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main()
