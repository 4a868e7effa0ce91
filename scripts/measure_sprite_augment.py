"""Timing behind profiles/sprite_augment.md (needs the GPU), which this script writes: ONE ``pa_sprite_augment`` launch of 448
sprites (64 windows x 7) at level 2 and at identity, the ``pa_synth_composite`` launch that reads the augmented bank, and
``pa_backbone_windows`` on the result.

    python scripts/measure_sprite_augment.py [--reps 20] [--out profiles/sprite_augment.md]

Device events around ``reps`` back-to-back launches on one stream after a warm-up of 3, five repeats with the four launches
alternated inside the one process; median (min .. max) of the five. No time is a pass bar."""
import argparse
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from playaid_core_amd import sprite_augment as sa  # noqa: E402
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd import synth_dataset as sd  # noqa: E402
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
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--sprites", type=int, default=128)
    ap.add_argument("--tree", default=None, help="what to name as the measured tree (default: git's HEAD, where there is a checkout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sprite_augment.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    S, D = 7, 128
    n = args.windows * S
    eng = Engine(synth.make_state_dict(seed=7), max_batch_frames=224, max_clip_frames=256, max_frame_height=128, max_frame_width=128)
    rng = np.random.default_rng(0)
    # renders of 160..256 px a side, between 1 : 1.5 and 1.5 : 1: the general INTER_AREA branch; the tall ones take the BICUBIC pad
    shapes = [(int(h), int(w)) for h, w in zip(rng.integers(160, 257, args.sprites), rng.integers(160, 257, args.sprites))]
    frames = [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for h, w in shapes]
    sprites = sd.SpriteBank.from_arrays(eng, {"c": {"A": {"c00": {"r": {"90": frames}}}}})
    stages = sd.StageBank.from_arrays(eng, [rng.integers(0, 256, (720, 1280, 3), dtype=np.uint8) for _ in range(4)])
    src = rng.integers(0, args.sprites, n)
    cases = {"level2": sa.sample_sprite_params(n, 2, rng, src=src), "identity": sa.identity_params(n, src=src)}
    assert all(sa.check_params(p, sprites) for p in cases.values())
    dev = {k: torch.from_numpy(v.view(np.uint8).reshape(n, -1)).to(eng.device) for k, v in cases.items()}
    bank = sa.AugmentedSpriteBank(eng, n)
    recs = np.zeros(n, dtype=sd.PARAMS_DTYPE)
    recs["sprite"] = np.arange(n)
    recs["stage"] = np.repeat(rng.integers(0, 4, args.windows), S)
    recs["stage_x"] = np.repeat(rng.integers(0, 1280 - D, args.windows), S)
    recs["stage_y"] = np.repeat(rng.integers(0, 720 - D, args.windows), S)
    recs["paste_dx"], recs["paste_dy"] = rng.integers(-40, 41, n), rng.integers(-40, 41, n)
    assert sd.check_params(recs, bank, stages, D)
    rd = torch.from_numpy(recs.view(np.uint8).reshape(n, -1)).to(eng.device)
    x = torch.empty((n, 3, D, D), dtype=torch.float32, device=eng.device)
    feats = torch.empty((n, 1024), dtype=torch.float32, device=eng.device)

    def aug(name):
        return lambda: eng._check(eng._lib.pa_sprite_augment(eng._h, sprites._h, dev[name].data_ptr(), n, bank._h, eng._stream()))

    def composite():
        eng._check(eng._lib.pa_synth_composite(eng._h, bank._h, stages._h, rd.data_ptr(), n, D, sd.FORMATS["model"], x.data_ptr(), eng._stream()))

    def backbone():
        eng._check(eng._lib.pa_backbone_windows(eng._h, x.data_ptr(), n, feats.data_ptr(), eng._stream()))

    runs = {"pa_sprite_augment, level 2": aug("level2"), "pa_sprite_augment, identity records": aug("identity"),
            "pa_synth_composite from the augmented bank (model layout)": composite, "pa_backbone_windows on the result": backbone}
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    samples = {k: [] for k in runs}
    for _ in range(5):
        for k, fn in runs.items():
            samples[k].append(timed(fn, args.reps))
    p2 = cases["level2"]
    tall = sum(1 for k in src if sa.resized_height(*shapes[int(k)]) > 128)
    try:
        if args.tree:
            raise LookupError
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        dirty = bool(subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain"], stderr=subprocess.DEVNULL).strip())
        commit += " plus uncommitted changes (the change that adds this file)" if dirty else ""
    except Exception:
        commit = args.tree or "unknown (no git metadata where this ran)"
    lines = [
        "# Augmenting the renders before the paste (`csrc/sprite_augment.hip`, DESIGN.md 5.16)",
        "",
        f"Written by `python scripts/measure_sprite_augment.py` on {torch.cuda.get_device_name(0)} (fp32 engine, seeded weights,",
        f"profiler off); tree: {commit}. A record, not a gate: nobody had measured this path. Times are HIP events around",
        f"{args.reps} back-to-back launches on one stream after a warm-up of 3, five repeats with the four launches alternated inside",
        "the one process; median (min .. max) of the five.",
        "",
        f"{n} sprites ({args.windows} windows x {S}) drawn uniformly from {args.sprites} RGBA renders of seeded noise, 160..256 px a side",
        f"(the general INTER_AREA branch; {tall} of the {n} are taller than wide and take the premultiplied BICUBIC pad). Level 2 as",
        f"`sample_sprite_params` drew it: {int((p2['new_scale'] != 0).sum())} shrunk (C > 128), {int(p2['sized_crop'].sum())} with the sized crop,",
        f"{int((p2['noise_sigma'] != 0).sum())} with noise, {int((p2['pixel_drop_thr'] != 0).sum())} with pixel dropout, {int((p2['n_holes'] != 0).sum())} with holes, "
        f"{int((p2['blur_k'] != 0).sum())} blurred; HSV always.",
        "Identity records switch the Compose and the shrink off: the front end (resize, pad) and the copies remain.",
        "",
        "| launch | us per call |",
        "|---|---|",
    ]
    for k, v in samples.items():
        lines.append(f"| `{k}` | {statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f}) |")
    lines += [
        "",
        f"The launch is min(n, 256) = {min(n, 256)} workgroups of 512 threads, each taking its sprites in turn through phases in",
        "memory (DESIGN.md 5.16), so its time is the longest workgroup's chain of phases, not a bandwidth figure. Not measured: the",
        "launch under `rocprofv3`, other render sizes, the 2 x 2 and integer fast branches, the dataset's per-item path.",
        "",
        "From the compiler (`-Rpass-analysis=kernel-resource-usage`): 120 VGPRs, no scratch, 36.3 KB of LDS per workgroup of 512",
        "threads, occupancy 4 waves per SIMD.",
    ]
    bank.close()
    sprites.close()
    stages.close()
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
