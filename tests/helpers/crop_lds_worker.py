"""Child of tests/test_frame_geometry.py: the fused crop kernel's LDS budget (PA_FUSED_LDS) is an
environment variable read once per process, so each budget runs in a process of its own. Runs the crop case lists of the frame
sizes named on the command line (indices into helpers.frame_geometry.FRAMES) through ``Engine.square_crops``, batch by batch as
the layout there says, and saves crops and status in case order: ``crops_<i>``, ``status_<i>``."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from helpers import frame_geometry as fg
from playaid_core_amd import synth
from playaid_core_amd.engine import Engine


def main():
    out_path = sys.argv[1]
    sizes = [int(a) for a in sys.argv[2:]]
    h = max(fg.FRAMES[fi][0] for fi in sizes)
    w = max(fg.FRAMES[fi][1] for fi in sizes)
    eng = Engine(synth.make_state_dict(seed=1234), max_batch_frames=fg.BATCH_FRAMES, max_clip_frames=64, max_frame_height=h, max_frame_width=w)
    res = {}
    try:
        for fi in sizes:
            cases = fg.crop_cases(fi)
            fr = torch.from_numpy(fg.frames(fi)).to(eng.device)
            crops = np.zeros((len(cases), 128, 128, 3), np.uint8)
            status = np.full(len(cases), -9, np.int64)
            for pad, slots in fg.batches(fi):
                c, s = eng.square_crops(fr, fg.call_boxes(fi, slots), padding=pad)
                sel = slots >= 0
                crops[slots[sel]] = c[sel]
                status[slots[sel]] = s[sel]
            res[f"crops_{fi}"], res[f"status_{fi}"] = crops, status
    finally:
        eng.close()
    np.savez(out_path, **res)


if __name__ == "__main__":
    main()
