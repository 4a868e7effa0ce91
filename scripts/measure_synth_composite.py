"""Timing behind profiles/synth_composite.md (needs the GPU): ONE ``pa_synth_composite`` launch of 64 x 7 frames at dim 128 into
the model layout, from 256 x 256 sprites (the 2 x 2 fast branch) and 1280 x 720 stages.

    python scripts/measure_synth_composite.py [--reps 50] [--out result.json]

Device events around ``reps`` back-to-back launches on one stream after a warm-up of 5, five repeats, median and spread
printed as one JSON line. The bytes are the ones the launch needs, computed from the shapes: every source pixel of every
frame's sprite once (a sprite that several frames use is counted for each, so this is an upper bound on what comes from HBM),
every stage-crop byte once, every output byte once."""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd import synth_dataset as sd  # noqa: E402
from playaid_core_amd.engine import Engine  # noqa: E402

HBM_PEAK_SPEC = 8.0e12       # bytes/s, MI355X_MICROARCH.md
HBM_PEAK_MEASURED = 6.29e12  # float4 copy, same document


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
    ap.add_argument("--reps", type=int, default=50)
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--sprites", type=int, default=128)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    S, D, side = 7, 128, 256
    n = args.windows * S
    eng = Engine(synth.make_state_dict(seed=7), max_batch_frames=4, max_clip_frames=16, max_frame_height=128, max_frame_width=128)
    rng = np.random.default_rng(0)
    frames = [rng.integers(0, 256, (side, side, 4), dtype=np.uint8) for _ in range(args.sprites)]
    sprites = sd.SpriteBank.from_arrays(eng, {"c": {"A": {"c00": {"r": {"90": frames}}}}})
    stages = sd.StageBank.from_arrays(eng, [rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8) for _ in range(4)])
    recs = np.zeros(n, dtype=sd.PARAMS_DTYPE)
    recs["sprite"] = rng.integers(0, args.sprites, n)
    recs["stage"] = np.repeat(rng.integers(0, 4, args.windows), S)          # one stage and origin per window, as get_synth
    recs["stage_x"] = np.repeat(rng.integers(0, 1280 - D, args.windows), S)
    recs["stage_y"] = np.repeat(rng.integers(0, 720 - D, args.windows), S)
    assert sd.check_params(recs, sprites, stages, D)
    pd = torch.from_numpy(recs.view(np.uint8).reshape(n, -1)).to(eng.device)
    outs = {"model": torch.empty((n, 3, D, D), dtype=torch.float32, device=eng.device),
            "uint8": torch.empty((n, D, D, 3), dtype=torch.uint8, device=eng.device)}

    def launch(fmt):
        return lambda: eng._check(eng._lib.pa_synth_composite(eng._h, sprites._h, stages._h, pd.data_ptr(), n, D, sd.FORMATS[fmt],
                                                              outs[fmt].data_ptr(), eng._stream()))

    runs = {fmt: launch(fmt) for fmt in outs}
    for fn in runs.values():
        for _ in range(5):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for _ in range(5):
        for k, fn in runs.items():
            samples[k].append(timed(fn, args.reps))
    out = {"frames": n, "dim": D, "sprite_side": side, "distinct_sprites": args.sprites}
    read = n * (side * side * 4 + D * D * 3) + n * 32
    for fmt, v in samples.items():
        written = n * D * D * 3 * (4 if fmt == "model" else 1)
        us = statistics.median(v)
        out[fmt] = {"us_median": round(us, 1), "us_min": round(min(v), 1), "us_max": round(max(v), 1), "bytes_read": read,
                    "bytes_written": written, "TBps": round((read + written) / (us * 1e-6) / 1e12, 3),
                    "roofline_us_at_8.0TBps": round((read + written) / HBM_PEAK_SPEC * 1e6, 1),
                    "fraction_of_spec_peak": round((read + written) / HBM_PEAK_SPEC / (us * 1e-6), 3),
                    "fraction_of_measured_copy_peak": round((read + written) / HBM_PEAK_MEASURED / (us * 1e-6), 3)}
    sprites.close()
    stages.close()
    eng.close()
    line = json.dumps(out)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
