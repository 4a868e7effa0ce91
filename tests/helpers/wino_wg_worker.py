"""Child of tests/test_wino_wg_engine.py: ``PA_WINO_WG`` is read once per process, so each launch width of layers 1 and 2 runs in a
process of its own. An exact engine of 16 crops (``max_batch_frames=8``) on 128 x 128 frames traces every stage of layers 1 and 2
(``pa_backbone_trace`` stages 2..9, stage 7 with its stored branch) and the stage that feeds them (1) at 16 and at 5 crops, and
takes the log-probabilities of two windows of 7 crops through the whole model."""
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
            rng = np.random.default_rng(9000 + n)
            x = torch.from_numpy(rng.integers(0, 256, (n, 3, 128, 128)).astype(np.float32) / np.float32(255)).cuda()
            for s in (1, 2, 3, 4, 5, 6, 8, 9):
                res[f"n{n}_s{s}"] = eng.backbone_trace(x, s).cpu().numpy()
            o, a = eng.backbone_trace(x, 7, aux=True)
            res[f"n{n}_s7"], res[f"n{n}_aux7"] = o.cpu().numpy(), a.cpu().numpy()
            if n >= 2 * eng.S:
                res["logp"] = eng.infer_windows(x[:2 * eng.S].reshape(2, eng.S, 3, 128, 128)).cpu().numpy()
        torch.cuda.synchronize()
    finally:
        eng.close()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main()
