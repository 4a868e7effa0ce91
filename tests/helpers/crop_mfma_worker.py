"""Child of tests/test_crop_mfma.py: ``PA_CROP_MFMA`` is read once per process, so each setting runs in a process of its own.
Runs every case of helpers/crop_mfma_cases.py through ``Engine.square_crops`` (two frames, two boxes a frame and call, one
padding a call), twice, and saves ``crops`` / ``status`` and ``crops_again`` / ``status_again`` in case order."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from helpers import crop_mfma_cases as cm
from playaid_core_amd import synth
from playaid_core_amd.engine import Engine


def run_all(eng, fr):
    n = len(cm.CASES)
    crops = np.zeros((n, 128, 128, 3), np.uint8)
    status = np.full(n, -9, np.int64)
    filler = cm.CASES[0][2]
    for pad in cm.PADDINGS:
        mine = [[i for i, c in enumerate(cm.CASES) if c[1] == pad and cm.frame_of(i) == f] for f in range(2)]
        for j in range(0, max(len(m) for m in mine), 2):
            boxes = np.zeros((2, 2, 4), np.float64)
            slots = -np.ones((2, 2), np.int64)
            for f in range(2):
                for s in range(2):
                    i = mine[f][j + s] if j + s < len(mine[f]) else -1
                    slots[f, s] = i
                    boxes[f, s] = cm.CASES[i][2] if i >= 0 else filler
            c, st = eng.square_crops(fr, boxes, padding=pad)
            sel = slots >= 0
            crops[slots[sel]] = c[sel]
            status[slots[sel]] = st[sel]
    return crops, status


def main():
    # (the fallback case's pass is 1280 wide: the engine's tables hold passes up to its largest frame side)
    eng = Engine(synth.make_state_dict(seed=1234), max_batch_frames=2, max_clip_frames=64, max_frame_height=1080, max_frame_width=1920)
    try:
        fr = torch.from_numpy(cm.frames()).to(eng.device)
        crops, status = run_all(eng, fr)
        crops2, status2 = run_all(eng, fr)
    finally:
        eng.close()
    np.savez(sys.argv[1], crops=crops, status=status, crops_again=crops2, status_again=status2)


if __name__ == "__main__":
    main()
