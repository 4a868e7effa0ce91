"""The detection stage for every YOLOv5 P5 size (n / s / m / l / x) and compute dtype: 64 x 1080p frames at 384 x 640, seeded
weights (synth.make_yolov5_state_dict, nc = 6). Per (size, dtype): ms per 64 frames (median of 5 calls after 2 warm-ups, HIP
events around pa_detector_forward), executed TFLOP/s (YoloV5Detector.flops_per_image: padding channels included) and the share of
the stem rows (pa_detector_forward_timed). Then the NMS entries on 64 frames of live rows at nc = 6 and nc = 80.
Usage: python scripts/detect_sizes.py [OUT] -- OUT (optional): a file that gets a copy of what the script prints
(profiles/r08_detect_sizes.txt holds one such run)."""
import ctypes as C
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd.engine import Engine, EngineError, _ptr  # noqa: E402
from playaid_core_amd.yolov5 import YoloV5Detector  # noqa: E402

N, H, W, NET = 64, 1080, 1920, (384, 640)
SIZES = os.environ.get("SIZES", "n,s,m,l,x").split(",")
DTYPES = os.environ.get("DTYPES", "f32,emulated_f32,bf16").split(",")
dev = torch.device("cuda:0")
out_lines = []


def say(s=""):
    print(s, flush=True)
    out_lines.append(s)


def ok(rc):
    assert rc == 0, rc


def events_ms(fn, reps=5, warm=2):
    for _ in range(warm):
        fn()
    t = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        torch.cuda.synchronize()
        t.append(a.elapsed_time(b))
    return float(np.median(t)), float(np.min(t)), float(np.max(t))


frames = torch.from_numpy(synth.make_frames(4, H, W)).to(dev).repeat(N // 4, 1, 1, 1).contiguous()
say(f"detection stage, {N} x {H}x{W} frames at {NET[0]}x{NET[1]}, seeded weights nc = 6; median (min..max) of 5 calls")
say(f"{'size':4s} {'dtype':13s} {'batches':7s} {'ms/64':>8s} {'min..max':>15s} {'GFLOP/img':>9s} {'TFLOP/s':>8s} {'stem rows':>9s} {'stem us':>8s} {'stem %':>6s}")
preds = {}
for size in SIZES:
    sd = synth.make_yolov5_state_dict(size, nc=6)
    for dt in DTYPES:
        batch = N
        try:
            det = YoloV5Detector(sd, 6, NET, max_images=N, compute_dtype=dt)
        except EngineError as e:
            say(f"{size:4s} {dt:13s} create refused at max_images = {N}: {e}; timing two batches of {N // 2}")
            batch = N // 2
            det = YoloV5Detector(sd, 6, NET, max_images=batch, compute_dtype=dt)
        pred = torch.empty((N, det.rows, 11), dtype=torch.float32, device=dev)
        stream = C.c_void_p(torch.cuda.current_stream(dev).cuda_stream)

        def run():
            for f0 in range(0, N, batch):
                rc = det._lib.pa_detector_forward(det._h, C.c_void_p(frames[f0:].data_ptr()), batch, H, W, C.c_void_p(pred[f0:].data_ptr()), stream)
                assert rc == 0, det._lib.pa_detector_last_error(det._h)

        med, lo, hi = events_ms(run)
        us = np.zeros((5, det.n_layers), np.float32)
        for it in range(5):
            rc = det._lib.pa_detector_forward_timed(det._h, C.c_void_p(frames.data_ptr()), batch, H, W, C.c_void_p(pred.data_ptr()), stream,
                                                    us[it].ctypes.data_as(C.c_void_p), det.n_layers)
            assert rc == 0
        lay = np.median(us[1:], axis=0) * (N // batch)
        stem = [i for i, L in enumerate(det.layers) if L.kind == 3]
        stem_us = float(lay[stem].sum())
        tf = det.flops_per_image * N / (med * 1e-3) / 1e12
        say(f"{size:4s} {dt:13s} {N // batch}x{batch:<4d} {med:8.2f} {lo:7.2f}..{hi:<7.2f} {det.flops_per_image / 1e9:9.1f} {tf:8.1f} {len(stem):9d} "
            f"{stem_us:8.0f} {100 * stem_us / float(lay.sum()):6.1f}")
        if dt == "f32" and size == "s":
            preds[6] = pred.clone()
        det.close()
        del det, pred
        torch.cuda.empty_cache()

# NMS: live rows of 64 frames; nc = 80 from an s network with 80 classes
say()
say("NMS on 64 frames of live rows (384 x 640: 15120 rows per frame), conf 0.25, iou 0.45, max_det 2; median (min..max) of 20 calls")
det = YoloV5Detector(synth.make_yolov5_state_dict("s", nc=80), 80, NET, max_images=N)
preds[80] = det(frames)
torch.cuda.synchronize()
det.close()
if 6 not in preds:
    det = YoloV5Detector(synth.make_yolov5s_state_dict(), 6, NET, max_images=N)
    preds[6] = det(frames)
    torch.cuda.synchronize()
    det.close()
eng = Engine(synth.make_state_dict(seed=1234), max_batch_frames=N, max_clip_frames=N)
lib, h = eng._lib, eng._h
dets = torch.empty((N, 8, 6), dtype=torch.float32, device=dev)
counts = torch.empty((N,), dtype=torch.int32, device=dev)
for nc, conf in ((6, 0.25), (80, 0.25), (6, 0.001), (80, 0.001)):
    pd = preds[nc]
    words = (C.c_uint32 * 3)(0xFFFFFFFF, 0xFFFFFFFF, 0xFFFFFFFF)
    n_gate = int(((pd[..., 4:5] * pd[..., 5:]).amax(-1) > conf).logical_and(pd[..., 4] > conf).sum(-1).max())
    tail = (2, NET[0], NET[1], H, W, _ptr(dets), _ptr(counts), eng._stream())
    runs = [("pa_detect_postprocess_classes", lambda: lib.pa_detect_postprocess_classes(h, _ptr(pd), N, pd.shape[1], nc, conf, 0.45, words, *tail))]
    if nc <= 32:
        runs.insert(0, ("pa_detect_postprocess", lambda: lib.pa_detect_postprocess(h, _ptr(pd), N, pd.shape[1], nc, conf, 0.45, (1 << nc) - 1, *tail)))
    for name, fn in runs:
        med, lo, hi = events_ms(lambda: ok(fn()), reps=20, warm=3)
        say(f"nc {nc:2d} conf {conf:<5g} (most rows over the gates in a frame: {n_gate:5d})  {name:30s} {1e3 * med:8.1f} us ({1e3 * lo:.1f}..{1e3 * hi:.1f})")
eng.close()
if len(sys.argv) > 1:
    out = os.path.abspath(sys.argv[1])
    os.makedirs(os.path.dirname(out), exist_ok=True)
    with open(out, "w") as f:
        f.write("\n".join(out_lines) + "\n")
