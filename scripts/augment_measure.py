"""Timings behind profiles/augment.md (needs the GPU): the augment launch for 448 crops (64 windows x 7) into model layout next
to ``pa_backbone_windows`` on the same 448 crops, and a ``fit_head`` epoch at level 0 and at level 2 on one clip.

    python scripts/augment_measure.py [--frames 64] [--reps 50]

Device events around ``reps`` back-to-back launches after a warm-up, five repeats each, median and spread printed; the two
kernels alternate inside one process."""
import argparse
import json
import os
import statistics
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from playaid_core_amd import augment, synth  # noqa: E402
from playaid_core_amd.engine import Engine  # noqa: E402


def timed(fn, reps):
    start, stop = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    start.record()
    for _ in range(reps):
        fn()
    stop.record()
    stop.synchronize()
    return start.elapsed_time(stop) * 1e3 / reps   # microseconds per call


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--epochs", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    out = {}
    n, S = 448, 7
    eng = Engine(synth.make_state_dict(seed=7), max_batch_frames=224, max_clip_frames=256, max_frame_height=128, max_frame_width=128)
    rng = np.random.default_rng(0)
    src = torch.from_numpy(rng.integers(0, 256, (128, 128, 128, 3), dtype=np.uint8)).to(eng.device)
    x = torch.empty((n, 3, 128, 128), dtype=torch.float32, device=eng.device)
    feats = torch.empty((n, 1024), dtype=torch.float32, device=eng.device)
    cases = {
        "identity": augment.identity_params(n, src=rng.integers(0, 128, n)),
        "level1": augment.sample_params(n, 1, rng, src=rng.integers(0, 128, n)),
        "level2": augment.sample_params(n, 2, rng, src=rng.integers(0, 128, n)),
        "everything": augment.sample_params(n, {k: 1.0 for k in augment.AUGMENT_DEFAULTS if k != "hard_mode"}, rng, src=rng.integers(0, 128, n)),
    }
    cases["everything"]["blur_k"] = 3
    dev = {k: torch.from_numpy(v.view(np.uint8).reshape(n, -1)).to(eng.device) for k, v in cases.items()}

    def aug(name, fmt=1, dst=None):
        dst = x if dst is None else dst
        return lambda: eng._check(eng._lib.pa_augment_crops(eng._h, src.data_ptr(), 128, dev[name].data_ptr(), n, fmt, dst.data_ptr(), eng._stream()))

    def backbone():
        eng._check(eng._lib.pa_backbone_windows(eng._h, x.data_ptr(), n, feats.data_ptr(), eng._stream()))

    u8 = torch.empty((n, 128, 128, 3), dtype=torch.uint8, device=eng.device)
    runs = {f"augment_{k}_model": aug(k) for k in cases}
    runs["augment_level2_uint8"] = aug("level2", 0, u8)
    runs["backbone_windows"] = backbone
    for fn in runs.values():   # warm-up
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for _ in range(5):
        for k, fn in runs.items():
            samples[k].append(timed(fn, args.reps))
    for k, v in samples.items():
        out[k + "_us"] = {"median": round(statistics.median(v), 1), "min": round(min(v), 1), "max": round(max(v), 1)}
    # bytes the augment launch needs: each source crop once, each output crop once
    moved = n * 49152 * (1 + 4)
    out["augment_level2_model_GBps"] = round(moved / (out["augment_level2_model_us"]["median"] * 1e-6) / 1e9, 1)
    eng.close()

    # a fit_head epoch at level 0 and level 2 on one clip
    from playaid_core_amd.ai_runner import AIRunner, ClipSource
    from playaid_core_amd.cnn_action_detector import CNNActionDetector

    actions = [f"action{i}" for i in range(63)]
    with tempfile.TemporaryDirectory() as td:
        for level in (0, 2, 0, 2):
            model = CNNActionDetector(actions, sequence_length=S, state_dict=synth.make_state_dict(seed=7), max_batch_frames=16, max_clip_frames=256,
                                      max_frame_height=360, max_frame_width=640, freeze_encoder=True)
            runner = AIRunner(ClipSource.synthetic(args.frames, 360, 640), model=model, output_dir=os.path.join(td, f"o{level}"), crop_mode="square",
                              crop_jpeg_quality=0, num_frames_per_sample=S)
            runner.run_action_recognition()
            gt = [[runner.ai_output_data[f][i].action for i in range(runner.max_frames - 1)] for f in runner.fighters]
            runner.fit_head(actions=gt, epochs=1, batch_size=64, seed=0, synth_difficulty=level)   # warm-up
            # every call runs the clip once and then its epochs, each ending in a read: the epoch's time is the difference
            times = []
            for epochs in (1, 1 + args.epochs):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                hist = runner.fit_head(actions=gt, epochs=epochs, batch_size=64, seed=0, synth_difficulty=level)
                times.append(time.perf_counter() - t0)
            dt = (times[1] - times[0]) / args.epochs
            out.setdefault(f"fit_head_epoch_level{level}_ms", []).append(round(dt * 1e3, 2))
            out["fit_head_windows"] = hist[0]["windows"]
            model.engine.close()
    print(json.dumps(out))


if __name__ == "__main__":
    main()
