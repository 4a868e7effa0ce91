"""Rate of the annotator's drawing step (pa_annotate_frames) on one GPU: 64 1080p frames with two Manuscript-style labels each,
no padding, against two baselines in the same process:
  (copy) a plain device-to-device copy of the same 64 frames -- the kernel is a copy that paints on the way
  (host) the route it replaces: frames device -> host, the reference's Pillow sequence per frame, host -> device
HIP events around whole calls (draw lists already built) after warm-up, alternating annotate / copy, median and min-max over --reps calls; the host route
is timed --host-reps times (events too: the second one is recorded after the upload, so the host's drawing is inside).
The device result is compared with the host route's, byte for byte, before anything is timed.
usage: python scripts/annotate_rate.py [--reps 50] [--host-reps 3] [--frames 64] [--out profiles/annotate_rate.txt]"""
import argparse
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
from annotate_reference import reference_annotate  # noqa: E402  (the live-Pillow arbiter of tests/test_annotate.py)
from playaid_core_amd import manuscript, synth  # noqa: E402
from playaid_core_amd.annotator import Annotator  # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--host-reps", type=int, default=3)
ap.add_argument("--frames", type=int, default=64)
ap.add_argument("--out", default=None)
args = ap.parse_args()
if not torch.cuda.is_available():
    sys.exit("annotate_rate.py measures on a GPU; none is visible")
n, h, w = args.frames, 1080, 1920
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def stats(ms):
    ms = sorted(ms)
    return f"median {ms[len(ms) // 2]:.3f} ms (min {ms[0]:.3f}, max {ms[-1]:.3f}, {len(ms)} calls)"


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


frames = synth.make_frames(n, h, w)
boxes = synth.make_boxes(n, h, w)  # the two fighters' boxes per frame, normalised centre / size
calls = []
for i in range(n):
    per = []
    for p, (label, color) in enumerate(((f"ForwardSmash | #{i % 40 + 1} | active", manuscript.LABEL_COLORS[0]),
                                        (f" | #{i + 1}", manuscript.HITSTUN_COLOR))):
        cx, cy, bw, bh = boxes[i, p] * np.array([w, h, w, h])
        per.append(((max(0, int(cx - bw / 2)), max(0, int(cy - bh / 2)), min(w, int(cx + bw / 2)), min(h, int(cy + bh / 2))), label, color))
    calls.append(per)

fd = torch.from_numpy(frames).cuda()
out = torch.empty_like(fd)
ann = Annotator(30, w, h, max_frames=n)


def build_lists():
    ann.set_frames(fd, line_width=manuscript.RENDER_LINE_WIDTH)
    for i, per in enumerate(calls):
        for box, label, color in per:
            ann.box_label(i, box, label=label, color=color, draw_box=False)


def annotate():  # the lists stay as built: one pa_annotate_frames call (checks, two small uploads, one launch)
    return ann.result(out=out)


def host_route():
    host = fd.cpu().numpy()
    drawn = np.stack([reference_annotate(host[i], [(b, l, c, False) for b, l, c in calls[i]], manuscript.RENDER_LINE_WIDTH) for i in range(n)])
    return torch.from_numpy(drawn).cuda()


want = host_route()
t0 = time.perf_counter()
build_lists()
t_lists = (time.perf_counter() - t0) * 1e3
annotate()
torch.cuda.synchronize()
assert torch.equal(out, want), "the device's frames differ from the Pillow route's"
painted = int((out != fd).any(dim=3).sum())
copy_dst = torch.empty_like(fd)
for _ in range(3):
    annotate()
    copy_dst.copy_(fd)
torch.cuda.synchronize()
t_ann, t_copy = [], []
for _ in range(max(args.reps, 20)):
    t_ann.append(timed(annotate))
    t_copy.append(timed(lambda: copy_dst.copy_(fd)))
t_host = [timed(host_route) for _ in range(max(args.host_reps, 1))]
mb = fd.numel() / 1e6
med = lambda t: sorted(t)[len(t) // 2]  # noqa: E731
say(f"device: {torch.cuda.get_device_name(0)}; {n} frames {h} x {w} BGR ({mb:.0f} MB read + {mb:.0f} MB written per call), two labels per frame, "
    f"{painted} pixels painted, pads 0; result byte-identical to the Pillow route")
say(f"annotate (one pa_annotate_frames call, lists built):  {stats(t_ann)} = {n / med(t_ann) * 1e3:.0f} frames/s, {2 * mb / med(t_ann):.0f} GB/s read + written")
say(f"copy     (torch device-to-device copy_):             {stats(t_copy)} = {2 * mb / med(t_copy):.0f} GB/s read + written")
say(f"building the {2 * n} box_label items on the host (Python, once per chunk, overlaps the device): {t_lists:.2f} ms")
say(f"annotate / copy: {med(t_ann) / med(t_copy):.2f}x")
say(f"host     (device -> host, Pillow on one host thread, host -> device): {stats(t_host)} = {n / med(t_host) * 1e3:.0f} frames/s; "
    f"host / annotate: {med(t_host) / med(t_ann):.0f}x")
if args.out:
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as fh:
        fh.write("\n".join(lines) + "\n")
ann.close()
