"""Shared by tests/test_stem_int.py and its child: ``PA_STEM_INT`` is read once per process, so ``PA_STEM_INT=0`` (the fp32 stem on
k / 255) runs in a process of its own. ``run(eng)`` sends one clip through each producer of the model input -- the crop stage
(16 frames of 360 x 640), the runner-input stage (crop images, 4 frames = 8 crops) and the JPEG round trip (4 frames = 8 crops) -- and
returns logp / action_id / crops per producer; as a program it saves them to the .npz named on the command line."""
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)

import numpy as np

H, W, N_CLIP, N_SMALL = 360, 640, 16, 4


def make_engine(dtype="f32", max_batch_frames=16):
    from playaid_core_amd import synth
    from playaid_core_amd.engine import Engine

    return Engine(synth.make_state_dict(seed=1234), max_batch_frames=max_batch_frames, max_clip_frames=64, max_frame_height=H,
                  max_frame_width=W, compute_dtype=dtype)


def crop_images(n):
    """images[frame][fighter]: BGR crop images of mixed sizes, as the detector leaves them for the runner."""
    rng = np.random.default_rng(77)
    return [[rng.integers(0, 256, (100 + 17 * f + 9 * k, 90 + 23 * k + 5 * f, 3), dtype=np.uint8) for k in range(2)] for f in range(n)]


def run_clip(eng, n=N_CLIP):
    from playaid_core_amd import synth

    r = eng.infer_clip(synth.make_frames(n, H, W, seed=31), synth.make_boxes(n, H, W), want_crops=True)
    return {"logp": r["logp"], "action_id": r["action_id"], "crops": r["crops_rgb"]}


def run_crop_images(eng):
    r = eng.infer_clip_from_crop_images(crop_images(N_SMALL), want_crops=True)
    return {"logp": r["logp"], "action_id": r["action_id"], "crops": r["crops_rgb"]}


def run_jpeg(eng):
    eng.set_crop_jpeg_quality(95)
    try:
        return run_clip(eng, N_SMALL)
    finally:
        eng.set_crop_jpeg_quality(0)


PRODUCERS = {"clip": run_clip, "crop_images": run_crop_images, "jpeg": run_jpeg}


def run(eng):
    return {f"{name}_{k}": v for name, fn in PRODUCERS.items() for k, v in fn(eng).items()}


if __name__ == "__main__":
    eng = make_engine()
    try:
        res = run(eng)
    finally:
        eng.close()
    np.savez(sys.argv[1], **res)
