"""Timing behind profiles/detect_composite.md (needs the GPU), which this script writes: the four device stages of one batch of
the detector's synthetic training images -- ``pa_sprite_resize``, ``pa_sprite_augment``, ``pa_scene_composite``,
``pa_jpegenc_encode`` -- for 64 scenes of 1280 x 720 with four sprites each, and a device-to-device copy of the scene
kernel's byte count beside it.

    python scripts/measure_detect_composite.py [--reps 20] [--out profiles/detect_composite.md]

Device events around ``reps`` back-to-back calls on one stream after a warm-up of 3, five repeats with the five alternated inside
the one process; median (min .. max) of the five. No time is a pass bar."""
import argparse
import ctypes as C
import os
import statistics
import subprocess
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from playaid_core_amd import detect_composite as dc  # noqa: E402
from playaid_core_amd import sprite_augment as sa  # noqa: E402
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd import synth_dataset as sd  # noqa: E402
from playaid_core_amd.engine import Engine  # noqa: E402
from playaid_core_amd.jpeg_encode import JpegEncoder, file_bytes_bound  # noqa: E402


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
    ap.add_argument("--scenes", type=int, default=64)
    ap.add_argument("--renders", type=int, default=32)
    ap.add_argument("--tree", default=None, help="what to name as the measured tree (default: git's HEAD, where there is a checkout)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "detect_composite.md"))
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("no GPU: nothing is measured")
    H, W, K = 720, 1280, dc.MAX_NUM_CHAR
    n, m = args.scenes, args.scenes * K
    eng = Engine(synth.make_state_dict(seed=7), max_batch_frames=4, max_clip_frames=16, max_frame_height=128, max_frame_width=128)
    rng = np.random.default_rng(0)
    # renders of 256..640 px a side, no taller than 3 : 1: both passes shrink at widths 50..150
    shapes = []
    while len(shapes) < args.renders:
        h, w = int(rng.integers(256, 641)), int(rng.integers(256, 641))
        if h <= 3 * w:
            shapes.append((h, w))
    sprites = sd.SpriteBank.from_arrays(eng, {"Pikachu": {"Jab": {"c00": {"r": {"0": [rng.integers(0, 256, (h, w, 4), dtype=np.uint8) for h, w in shapes]}}}}})
    # stage pictures: blocks of 16 x 16 with a little noise on top (flat noise is the entropy coder's worst case, not a picture)
    stage_arrays = []
    for _ in range(4):
        coarse = np.kron(rng.integers(0, 256, (H // 16, W // 16, 3)), np.ones((16, 16, 1), dtype=np.int64))
        stage_arrays.append(np.clip(coarse + rng.integers(-3, 4, (H, W, 3)), 0, 255).astype(np.uint8))
    stages = sd.StageBank.from_arrays(eng, stage_arrays)
    src = rng.integers(0, args.renders, m)
    bw = rng.integers(dc.BASEWIDTH_MIN, dc.BASEWIDTH_MAX, m, endpoint=True)
    hs = [int(float(shapes[k][0]) * (int(b) / float(shapes[k][1]))) for k, b in zip(src, bw)]
    resize = dc.resize_params(src, bw, hs)
    aug = sa.sample_sprite_params(m, {}, rng, src=np.arange(m))
    scenes = np.zeros(n, dtype=dc.SCENE_DTYPE)
    scenes["stage"] = rng.integers(0, 4, n)
    scenes["n_sprites"] = K
    scenes["sprites"]["slot"] = np.arange(m).reshape(n, K)
    scenes["sprites"]["x"] = np.clip(rng.normal(W / 2, W / 6, (n, K)), 0, W).astype(np.int64) - 64
    scenes["sprites"]["y"] = np.clip(rng.normal(H / 2, H / 6, (n, K)), 0, H).astype(np.int64) - 64
    resized = dc.ResizedSpriteBank(eng, m, dc.BASEWIDTH_MAX, int(3.5 * dc.BASEWIDTH_MAX))
    augmented = sa.AugmentedSpriteBank(eng, m)
    assert dc.resize_check_status(resize, sprites, resized) == 0 and dc.scene_check_params(scenes, augmented, stages)
    dc.resize_sprites(eng, sprites, resize, out=resized)
    assert sa.check_params(aug, resized)
    _, total = dc.scene_layout(scenes, stages.shapes)
    images = torch.empty(total, dtype=torch.uint8, device=eng.device)
    mirror = torch.empty(total, dtype=torch.uint8, device=eng.device)
    desc = torch.empty((n, 2), dtype=torch.int64, device=eng.device)
    aug_dev = torch.from_numpy(aug.view(np.uint8).reshape(m, -1)).to(eng.device)
    scenes_dev = torch.from_numpy(scenes.view(np.uint8).reshape(n, -1)).to(eng.device)
    enc = JpegEncoder.for_frames(n, H, W, subsampling=2, device=str(eng.device))
    files = torch.empty(n * (file_bytes_bound(H, W, 2) // 2 + 16), dtype=torch.uint8, device=eng.device)
    records = torch.empty((n, 2), dtype=torch.int64, device=eng.device)

    def f_resize():
        eng._check(eng._lib.pa_sprite_resize(eng._h, sprites._h, resize.ctypes.data_as(C.c_void_p), m, resized._h, eng._stream()))

    def f_augment():
        eng._check(eng._lib.pa_sprite_augment(eng._h, resized._h, aug_dev.data_ptr(), m, augmented._h, eng._stream()))

    def f_scene():
        eng._check(eng._lib.pa_scene_composite(eng._h, augmented._h, stages._h, scenes_dev.data_ptr(), n, images.data_ptr(), total,
                                               desc.data_ptr(), eng._stream()))

    def f_encode():
        enc.encode_images(images, desc, H, W, quality=dc.JPEG_QUALITY, subsampling=2, bgr=False, files=files, records=records)

    def f_copy():
        mirror.copy_(images)

    runs = {"pa_sprite_resize": f_resize, "pa_sprite_augment (the function's own defaults)": f_augment,
            "pa_scene_composite (layout + scenes)": f_scene, "pa_jpegenc_encode (quality 95, 4:2:0)": f_encode,
            "device-to-device copy of the scenes' bytes": f_copy}
    for fn in runs.values():
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    assert enc.overflows() == 0
    sizes = JpegEncoder.unpack_files(files, records)
    samples = {k: [] for k in runs}
    for _ in range(5):
        for k, fn in runs.items():
            samples[k].append(timed(fn, args.reps))
    try:
        if args.tree:
            raise LookupError
        commit = subprocess.check_output(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], stderr=subprocess.DEVNULL).decode().strip()
        dirty = bool(subprocess.check_output(["git", "-C", ROOT, "status", "--porcelain"], stderr=subprocess.DEVNULL).strip())
        commit += " plus uncommitted changes (the change that adds this file)" if dirty else ""
    except Exception:
        commit = args.tree or "unknown (no git metadata where this ran)"
    moved = 2 * total + m * 65536   # every scene byte read and written once; every sprite slot read at least once
    t_scene, t_copy = statistics.median(samples["pa_scene_composite (layout + scenes)"]), statistics.median(samples["device-to-device copy of the scenes' bytes"])
    taps = [int(np.ceil(2.0 * max(shapes[k][1] / int(b), 1.0))) * 2 + 1 for k, b in zip(src, bw)]
    lines = [
        "# The detector's synthetic training images on the device (`csrc/sprite_resize.hip`, `csrc/scene_composite.hip`, DESIGN.md 5.17)",
        "",
        f"Written by `python scripts/measure_detect_composite.py` on {torch.cuda.get_device_name(0)} (profiler off); tree: {commit}.",
        f"A record, not a gate: nobody had measured this path. Times are HIP events around {args.reps} back-to-back calls on one stream",
        "after a warm-up of 3, five repeats with the five alternated inside the one process; median (min .. max) of the five.",
        "",
        f"One batch: {n} scenes of {W} x {H} with {K} sprites each ({m} sprites), the stages drawn from 4 pictures (16 x 16 blocks plus",
        f"noise of +-3), the renders from {args.renders} RGBA images of seeded noise, 256..640 px a side, resized to widths 50..150",
        f"({min(taps)}..{max(taps)} taps a row in the horizontal pass), centres Gaussian as the reference draws them. The JPEG files of the",
        f"batch come to {sum(len(f) for f in sizes) / 1e6:.1f} MB.",
        "",
        "| stage | us per call |",
        "|---|---|",
    ]
    for k, v in samples.items():
        lines.append(f"| `{k}` | {statistics.median(v):.1f} ({min(v):.1f} .. {max(v):.1f}) |")
    lines += [
        "",
        f"The scene launch moves {moved / 1e6:.1f} MB ({total / 1e6:.1f} MB of stage bytes read, as many written, {m * 65536 / 1e6:.1f} MB of sprite",
        f"slots read): {moved / t_scene / 1e6:.2f} TB/s over its median time. The copy beside it moves {2 * total / 1e6:.1f} MB:",
        f"{2 * total / t_copy / 1e6:.2f} TB/s. The scenes' time is {t_scene / t_copy:.2f} times the copy's.",
        "",
        "What the scenes' call does beyond the copy: a second, one-workgroup launch ahead of it (the layout), two comparisons per",
        "sprite and 16-byte piece, the row and column of every piece inside a sprite's band of rows, and the blends themselves, in",
        "waves where only the lanes under a sprite work. Both sides move whole aligned 16-byte pieces with consecutive lanes on",
        "consecutive addresses, so the access pattern is the copy's; which of the three accounts for how much was not measured.",
        "The stages of this batch are drawn from 4 pictures (11 MB), which the last-level cache can hold, while the copy reads its",
        "177 MB once: on the read side the comparison favours the scene launch. Not separated.",
        "",
        "From the compiler (`-Rpass-analysis=kernel-resource-usage`): the scene kernel 40 VGPRs, no scratch, 128 bytes of LDS,",
        "occupancy 8 waves per SIMD, four `global_load_dwordx4` and four `global_store_dwordx4` per thread; the resize kernel 84",
        "VGPRs, no scratch, 27.6 KB of LDS per workgroup of 512 threads, occupancy 5.",
        "",
        "Not measured: either launch under `rocprofv3`, other stage sizes, mixed-size batches, the host side of",
        "`generate_stage_char_compositions` (the draws, the one device -> host copy, the file writes).",
    ]
    for b in (resized, augmented, sprites, stages):
        b.close()
    eng.close()
    text = "\n".join(lines) + "\n"
    print(text)
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)


if __name__ == "__main__":
    main()
