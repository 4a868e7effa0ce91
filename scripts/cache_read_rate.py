"""Read rate of the detector's crop cache: 512 frames x 2 crop files (save_one_box crops of a 1080p synthetic clip, quality 95,
4:4:4, written by ai_cache.write_detector_cache), files in the page cache.
  device: file bytes -> packed crops in HBM through JpegDecoder.decode_files (read the files, plan, upload, decode, status check)
  host:   the path ClipSource.from_cache takes without a decoder -- Image.open(...).convert("RGB") per file on one thread -- plus
          Engine._pack_crop_images (pack on the host, upload), which is what infer_clip_from_crop_images does with the pixels
Wall time around the whole of each, three runs each after one warm-up run; images/s and the spread.
usage: python scripts/cache_read_rate.py [--frames 512] [--runs 3]"""
import argparse
import os
import shutil
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from playaid_core_amd import ai_cache, constants, synth  # noqa: E402
from playaid_core_amd.engine import Engine  # noqa: E402
from playaid_core_amd.jpeg_decode import JpegDecoder  # noqa: E402
from playaid_core_amd.jpeg_encode import JpegEncoder, coded_blocks  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--frames", type=int, default=512)
ap.add_argument("--runs", type=int, default=3)
args = ap.parse_args()
h, w, base = 1080, 1920, 64
n = max(base, args.frames // base * base)

# the cache: 64 distinct frames, written n / 64 times under consecutive frame numbers
frames = synth.make_frames(base, h, w)
boxes = synth.make_boxes(base, h, w)
dets = np.zeros((base, 2, 6), np.float32)
for i in range(base):
    for p in range(2):
        cx, cy, bw, bh = boxes[i, p] * np.array([w, h, w, h])
        x1, y1, x2, y2 = np.rint([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]).clip(0, [w, h, w, h]).astype(np.float32)
        dets[i, p] = [2 + p, (x1 + x2) / 2 / w, (y1 + y2) / 2 / h, (x2 - x1) / w, (y2 - y1) / h, 0.9]
eng = Engine(synth.make_state_dict(seed=1234), max_batch_frames=base, max_clip_frames=base, max_frame_height=h, max_frame_width=w)
enc = JpegEncoder(2 * base, 2 * base * coded_blocks(h, w, 0))
root = tempfile.mkdtemp(prefix="cache_read_")
try:
    part = os.path.join(root, "part")
    ai_cache.write_detector_cache(eng, enc, torch.from_numpy(frames).cuda(), torch.from_numpy(dets).cuda(),
                                  torch.full((base,), 2, dtype=torch.int32, device="cuda"), part, "clip")
    enc.close()
    fighters = [constants.CHAR_LIST[2], constants.CHAR_LIST[3]]
    paths = []
    for f in fighters:
        os.makedirs(os.path.join(root, "crops", f))
    for i in range(n):
        for f in fighters:
            dst = os.path.join(root, "crops", f, f"clip_{i + 1}.jpg")
            shutil.copyfile(os.path.join(part, "crops", f, f"clip_{i % base + 1}.jpg"), dst)
            paths.append(dst)
    sizes = [os.path.getsize(p) for p in paths]
    for p in paths:   # into the page cache
        open(p, "rb").read()

    def device_read(dec):
        blobs = [open(p, "rb").read() for p in paths]
        images, desc, status = dec.decode_files(blobs)   # synchronises and checks every status
        return images, desc

    def host_read():
        from PIL import Image

        ims = []
        for p in paths:
            with Image.open(p) as im:
                ims.append(np.ascontiguousarray(np.asarray(im.convert("RGB"))[..., ::-1]))
        buf, desc = eng._pack_crop_images(ims)
        torch.cuda.synchronize()
        return buf, desc

    def timed(fn):
        fn()
        out = []
        for _ in range(args.runs):
            t0 = time.perf_counter()
            fn()
            out.append(time.perf_counter() - t0)
        return out

    from PIL import Image

    hw = []
    for p in paths[: 2 * base]:
        with Image.open(p) as im0:
            hw.append(im0.size)
    mh, mw = max(s[1] for s in hw), max(s[0] for s in hw)
    dec = JpegDecoder.for_crops(len(paths), mh, mw)
    # the two paths give the same bytes
    a, da = device_read(dec)
    b, db = host_read()
    assert torch.equal(da, db), "device and host descriptors differ"
    assert all(np.array_equal(x, y) for x, y in zip(eng.unpack_crop_images(a, da), eng.unpack_crop_images(b, db))), "decodes differ"
    print(f"device: {torch.cuda.get_device_name(0)}; {len(paths)} crop files of {n} frames (up to {mh} x {mw}, "
          f"{sum(sizes) / 1e6:.1f} MB of files, {b.numel() / 1e6:.1f} MB decoded), one host thread")
    res = {}
    for name, fn in (("device (JpegDecoder.decode_files)", lambda: device_read(dec)), ("host (Image.open loop + _pack_crop_images)", host_read)):
        t = timed(fn)
        rate = [len(paths) / x for x in t]
        res[name] = sorted(rate)[len(rate) // 2]
        print(f"{name}: " + ", ".join(f"{x * 1e3:.1f} ms" for x in t) + f" -> median {res[name]:.0f} images/s "
              f"(min {min(rate):.0f}, max {max(rate):.0f})")
    # where the device path's time goes: the host's share (file reads, marker segments, join) against the enqueued work
    t0 = time.perf_counter()
    blobs = [open(p, "rb").read() for p in paths]
    t1 = time.perf_counter()
    dec.plan(blobs)
    t2 = time.perf_counter()
    print(f"device path, host share: file reads {(t1 - t0) * 1e3:.1f} ms, pa_jpegdec_plan {(t2 - t1) * 1e3:.1f} ms")
    d, h_ = list(res.values())
    print(f"device / host: {d / h_:.2f}x" + ("" if d > h_ else "  -- THE DEVICE PATH IS NOT FASTER THAN ONE HOST THREAD OF PILLOW"))
    dec.close()
finally:
    shutil.rmtree(root, ignore_errors=True)
    eng.close()
