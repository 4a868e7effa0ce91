"""Encode rate of pa_jpegenc_encode on one GPU against Pillow (libjpeg-turbo) on one host core of the same machine.
  (a) the 128 detector crops (save_one_box, raw) of the bench's 64-frame 1080p clip, quality 95, 4:4:4 -- the crop cache
  (b) 64 1080p frames, quality 95, 4:2:0 -- a Motion-JPEG clip
HIP events around whole calls after warm-up, median and min-max over --reps calls (images in HBM, files left in HBM; the
device -> host copy of the files is timed apart). The per-stage split of a call comes from the kernel trace:
  rocprofv3 --kernel-trace --stats -- python scripts/jpegenc_rate.py --reps 20 --no-pillow
usage: python scripts/jpegenc_rate.py [--reps 20] [--frames 64] [--no-pillow]"""
import argparse
import io
import os
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd.engine import Engine  # noqa: E402
from playaid_core_amd.jpeg_encode import JpegEncoder, coded_blocks  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--no-pillow", action="store_true")
args = ap.parse_args()
n, h, w = args.frames, 1080, 1920
reps = max(args.reps, 20)


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:.3f} ms (min {ms[0]:.3f}, max {ms[-1]:.3f}, {len(ms)} calls)"


def time_calls(fn):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return out


def pillow_ms(images_rgb, subsampling):
    from PIL import Image

    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        for im in images_rgb:
            Image.fromarray(im).save(io.BytesIO(), format="JPEG", quality=95, subsampling=subsampling)
        t.append((time.perf_counter() - t0) * 1e3)
    return min(t)


frames = synth.make_frames(n, h, w)
fd = torch.from_numpy(frames).cuda()
print(f"device: {torch.cuda.get_device_name(0)}; host threads used by Pillow's encoder: 1 (libjpeg-turbo encodes in the calling "
      f"thread; torch reports {torch.get_num_threads()} intra-op threads, unused here)")

# (a) the detector's crops
boxes = synth.make_boxes(n, h, w)
dets = np.zeros((n, 2, 6), np.float32)
for i in range(n):
    for p in range(2):
        cx, cy, bw, bh = boxes[i, p] * np.array([w, h, w, h])
        x1, y1, x2, y2 = np.rint([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]).clip(0, [w, h, w, h]).astype(np.float32)
        dets[i, p] = [2 + p, (x1 + x2) / 2 / w, (y1 + y2) / 2 / h, (x2 - x1) / w, (y2 - y1) / h, 0.9]
eng = Engine(synth.make_state_dict(seed=1234), max_batch_frames=max(n, 64), max_clip_frames=max(n, 64), max_frame_height=h, max_frame_width=w)
images, desc = eng.save_one_box_crops(fd, torch.from_numpy(dets).cuda(), torch.full((n,), 2, dtype=torch.int32, device="cuda"), jpeg_quality=0)
eng.check_device_errors()
crops = eng.unpack_crop_images(images, desc)
px = sum(c.shape[0] * c.shape[1] for c in crops if c is not None)
mh, mw = max(c.shape[0] for c in crops if c is not None), max(c.shape[1] for c in crops if c is not None)
enc = JpegEncoder(2 * n, sum(coded_blocks(c.shape[0], c.shape[1], 0) for c in crops if c is not None) + 64)
files = torch.empty(px * 3 + 2 * n * 1024, dtype=torch.uint8, device="cuda")
rec = torch.empty((2 * n, 2), dtype=torch.int64, device="cuda")
ms = time_calls(lambda: enc.encode_images(images, desc, mh, mw, quality=95, subsampling=0, bgr=True, files=files, records=rec))
blobs = enc.unpack_files(files, rec)
assert enc.overflows() == 0 and all(b for b in blobs)
nbytes = sum(len(b) for b in blobs)
med = sorted(ms)[len(ms) // 2]
print(f"(a) {len(crops)} detector crops (up to {mh} x {mw}, {px / 1e6:.2f} Mpixel, {nbytes / 1e6:.2f} MB of files), q95 4:4:4: {stats(ms)} "
      f"= {len(crops) / med * 1e3:.0f} crops/s, {px / med / 1e3:.0f} Mpixel/s")
t0 = time.perf_counter()
enc.unpack_files(files, rec)
print(f"    device -> host copy of the files + split: {(time.perf_counter() - t0) * 1e3:.3f} ms")
if not args.no_pillow:
    t = pillow_ms([np.ascontiguousarray(c[..., ::-1]) for c in crops], 0)
    print(f"    Pillow, one host thread, same crops: {t:.1f} ms = {len(crops) / t * 1e3:.0f} crops/s  (device / host: {t / med:.1f}x)")
enc.close()

# (b) whole frames
enc = JpegEncoder.for_frames(n, h, w, 2)
d2 = torch.empty((n, 2), dtype=torch.int64, device="cuda")
d2[:, 0] = torch.arange(n, device="cuda", dtype=torch.int64) * (h * w * 3)
d2[:, 1] = (w << 32) | h
files = torch.empty(n * h * w, dtype=torch.uint8, device="cuda")
rec = torch.empty((n, 2), dtype=torch.int64, device="cuda")
ms = time_calls(lambda: enc.encode_images(fd.reshape(-1), d2, h, w, quality=95, subsampling=2, bgr=True, files=files, records=rec))
blobs = enc.unpack_files(files, rec)
assert enc.overflows() == 0 and all(b for b in blobs)
med = sorted(ms)[len(ms) // 2]
print(f"(b) {n} frames {h} x {w} ({sum(len(b) for b in blobs) / 1e6:.1f} MB of files), q95 4:2:0: {stats(ms)} = {n / med * 1e3:.0f} frames/s")
if not args.no_pillow:
    t = pillow_ms([np.ascontiguousarray(f[..., ::-1]) for f in frames], 2)
    print(f"    Pillow, one host thread, same frames: {t:.1f} ms = {n / t * 1e3:.0f} frames/s  (device / host: {t / med:.1f}x)")
    if t < med:
        print("    THE DEVICE ENCODER IS SLOWER THAN ONE HOST CORE OF PILLOW ON (b)")
enc.close()
eng.close()
