"""Child of tests/test_crop_mfma_h.py: ``PA_CROP_MFMA_H`` / ``PA_CROP_MFMA`` are read once per process, so each setting runs
in a process of its own. One engine runs, in this order: every case of helpers/crop_mfma_h_cases.py twice in a row
(``crops`` / ``crops_again``), every case once more in reverse order (``crops_rev``: a call with small crops behind one with
large crops), the calls of several crop counts (``count_<frames>``), the 12-crop call twenty times (``twenty_equal``), and one
clip longer than the engine's batch through ``infer_clip`` (``clip_rgb``)."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import numpy as np
import torch

from helpers import crop_mfma_h_cases as ch
from playaid_core_amd import synth
from playaid_core_amd.engine import Engine


def run_case(eng, dev_frames, i):
    name, fs, fr, bx = ch.CASES[i]
    n = ch.SETS[fs][2]
    boxes = np.tile(np.asarray(bx, np.float64), (n, 2, 1))
    c, st = eng.square_crops(dev_frames[fs], boxes)
    return c[fr, 0], st[fr, 0]


def main():
    sd = synth.make_state_dict(seed=1234)
    out = {}
    eng = Engine(sd, max_batch_frames=40, max_clip_frames=64, max_frame_height=560, max_frame_width=640)
    try:
        dev = {fs: torch.from_numpy(ch.frames(fs)).to(eng.device) for fs in ch.SETS}
        n = len(ch.CASES)
        for key in ("crops", "crops_again", "crops_rev"):
            out[key] = np.zeros((n, 128, 128, 3), np.uint8)
            out[key.replace("crops", "status")] = np.full(n, -9, np.int64)
        for i in range(n):
            out["crops"][i], out["status"][i] = run_case(eng, dev, i)
            out["crops_again"][i], out["status_again"][i] = run_case(eng, dev, i)
        for i in reversed(range(n)):
            out["crops_rev"][i], out["status_rev"][i] = run_case(eng, dev, i)
        for nf, slots in ch.COUNTS:
            fr = torch.from_numpy(ch.mixed_frames(nf)).to(eng.device)
            bx, _ = ch.mixed_boxes(nf, slots)
            c, st = eng.square_crops(fr, bx)
            out[f"count_{nf}"], out[f"count_status_{nf}"] = c, st.astype(np.int64)
            if nf == 6:
                same = True
                for _ in range(20):
                    c2, st2 = eng.square_crops(fr, bx)
                    same = same and np.array_equal(c2, c) and np.array_equal(st2, st)
                out["twenty_equal"] = np.array(same)
    finally:
        eng.close()
    eng = Engine(sd, max_batch_frames=ch.CLIP_BATCH, max_clip_frames=64, max_frame_height=ch.SETS["main"][0], max_frame_width=ch.SETS["main"][1])
    try:
        bx, _ = ch.mixed_boxes(ch.CLIP_FRAMES, 2)
        out["clip_rgb"] = np.asarray(eng.infer_clip(ch.mixed_frames(ch.CLIP_FRAMES), bx, want_crops=True)["crops_rgb"])
    finally:
        eng.close()
    np.savez(sys.argv[1], **out)


if __name__ == "__main__":
    main()
