"""Measurements behind profiles/crop_any_size.md: the sized crop kernels against the 128 x 128 ones at S = 128, the kind-3 stem
against stem_pool_kernel at in_hw = 128, and the ResNet-50 table at 256 x 256. HIP events, warm-up, repeated windows, every
pair alternated inside one process. Usage: python scripts/crop_any_size_measure.py [out.txt]"""
import ctypes as C
import os
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd.engine import Engine, _ptr  # noqa: E402
from playaid_core_amd.resnet_transformer_detector import ConvNet, build_resnet50_table  # noqa: E402

LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, calls, windows=7, warm=3):
    """-> ms per call of each window (device events around `calls` back-to-back calls)."""
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(windows):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(calls):
            fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b) / calls)
    return out


def ab(name_a, fa, name_b, fb, calls, rounds=3):
    """Alternates the two; -> (median a, median b), and says medians, spreads and the ratio."""
    ta, tb = [], []
    for _ in range(rounds):
        ta += timed(fa, calls, windows=3)
        tb += timed(fb, calls, windows=3)
    ma, mb = statistics.median(ta), statistics.median(tb)
    say(f"  {name_a}: median {ma:.4f} ms (min {min(ta):.4f}, max {max(ta):.4f}; {len(ta)} windows of {calls} calls)")
    say(f"  {name_b}: median {mb:.4f} ms (min {min(tb):.4f}, max {max(tb):.4f})")
    say(f"  ratio {name_b} / {name_a}: {mb / ma:.3f}")
    return ma, mb


def crops_section():
    say("## 1. Crop kernels, 128 crops per call (64 frames of 1080p x 2 fighters, padding 30)")
    eng = Engine(synth.make_state_dict(seed=1234), max_batch_frames=64, max_clip_frames=64)
    try:
        n, h, w = 64, 1080, 1920
        frames = np.ascontiguousarray(np.tile(synth.make_frames(8, h, w, seed=11), (8, 1, 1, 1)))
        boxes = synth.make_boxes(n, h, w)
        fd = torch.from_numpy(frames).to(eng.device)
        bd = torch.from_numpy(boxes).to(eng.device)
        st = torch.empty((n, 2), dtype=torch.int32, device=eng.device)
        stream = C.c_void_p(torch.cuda.current_stream(eng.device).cuda_stream)
        d = np.maximum((boxes[..., 2] * w).astype(int), (boxes[..., 3] * h).astype(int))
        say(f"  square sides d = {d.min()} .. {d.max()} pixels")
        outs = {}

        def call(size, sized):
            out = outs.setdefault((size, sized), torch.empty((n, 2, size, size, 3), dtype=torch.uint8, device=eng.device))
            if sized:
                rc = eng._lib.pa_square_crops_sized(eng._h, _ptr(fd), n, h, w, _ptr(bd), 30, 0, size, _ptr(out), _ptr(st), stream)
            else:
                rc = eng._lib.pa_square_crops(eng._h, _ptr(fd), n, h, w, _ptr(bd), 30, 0, _ptr(out), _ptr(st), stream)
            assert rc == 0

        call(128, False), call(128, True)
        torch.cuda.synchronize()
        assert torch.equal(outs[(128, False)], outs[(128, True)]) and int(st.abs().sum()) == 0
        say("  outputs of the two entry points at 128: identical bytes, every status 0")
        ab("pa_square_crops (128 kernels)", lambda: call(128, False), "pa_square_crops_sized(128)", lambda: call(128, True), calls=50)
        for size in (64, 256, 512):
            t = timed(lambda: call(size, True), 50, windows=5)
            say(f"  pa_square_crops_sized({size}): median {statistics.median(t):.4f} ms (min {min(t):.4f}, max {max(t):.4f})")
    finally:
        eng.close()
    say()


def net_ms(net, x, calls=10):
    return timed(lambda: net.forward(x), calls, windows=5)


def stem_section(sd):
    say("## 2. Stem + max-pool at in_hw = 128, 64 crops per call: kind 3 (stem_pool_any) against kind 1 (stem_pool_kernel)")
    descs, bufs, weights, dim = build_resnet50_table(sd)
    k3 = [dict(descs[0], kind=3)] + descs[1:]          # a kind-3 table at 128: through the C ABI only (the builder emits kind 1 at 128)
    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.integers(0, 256, (64, 3, 128, 128)).astype(np.float32) / np.float32(255)).cuda()
    one = 34 * 34 * 64
    a1, a3 = ConvNet(descs[:1], bufs, weights, one, max_crops=64), ConvNet(k3[:1], bufs, weights, one, max_crops=64)
    f1, f3 = ConvNet(descs, bufs, weights, dim, max_crops=64), ConvNet(k3, bufs, weights, dim, max_crops=64)
    try:
        ya, yb = a1.forward(x), a3.forward(x)
        say(f"  stem outputs: max|kind 3 - kind 1| = {float((ya - yb).abs().max()):.3g} (max|kind 1| {float(ya.abs().max()):.3g}); forms {a1.layer_forms()} / {a3.layer_forms()}")
        conv = timed(lambda: a1.trace(x, -1, 0), 20, windows=5)
        say(f"  (input conversion + the copy of one output buffer alone: median {statistics.median(conv):.4f} ms -- part of both rows below)")
        say("  one-row tables (input conversion + stem + copy of the pooled map):")
        m1, m3 = ab("kind 1", lambda: a1.forward(x), "kind 3", lambda: a3.forward(x), calls=20)
        say(f"  stem alone, conversion and copy taken off: kind 1 {m1 - statistics.median(conv):.4f} ms, kind 3 {m3 - statistics.median(conv):.4f} ms")
        say("  whole ResNet-50 table at 128, f32:")
        ab("kind-1 table", lambda: f1.forward(x), "kind-3 table", lambda: f3.forward(x), calls=5)
    finally:
        for net in (a1, a3, f1, f3):
            net.close()
    say()


def resnet_section(sd):
    say("## 3. ResNet-50 table at 256 x 256, 64 crops per call (max_crops 64)")
    ref_descs = build_resnet50_table(sd)[0]
    descs, bufs, weights, dim = build_resnet50_table(sd, crop_size=256)
    rng = np.random.default_rng(6)
    x = torch.from_numpy(rng.integers(0, 256, (64, 3, 256, 256)).astype(np.float32) / np.float32(255)).cuda()
    x128 = x[:, :, :128, :128].contiguous()
    names = ["stem"]
    for li, blocks in enumerate((3, 4, 6, 3), start=1):
        for b in range(blocks):
            names += [f"layer{li}.{b}.conv1", f"layer{li}.{b}.conv2"] + ([f"layer{li}.{b}.downsample"] if b == 0 else []) + [f"layer{li}.{b}.conv3"]
    names.append("avgpool")
    for dtype in ("f32", "emulated_f32"):
        net = ConvNet(descs, bufs, weights, dim, max_crops=64, compute_dtype=dtype)
        net128 = ConvNet(ref_descs, *build_resnet50_table(sd)[1:], max_crops=64, compute_dtype=dtype)
        try:
            t = net_ms(net, x)
            t128 = net_ms(net128, x128)
            say(f"  {dtype}: 256 x 256: median {statistics.median(t):.3f} ms per 64 crops (min {min(t):.3f}, max {max(t):.3f}); "
                f"128 x 128 on the same handle size: {statistics.median(t128):.3f} ms (min {min(t128):.3f}, max {max(t128):.3f}); ratio {statistics.median(t) / statistics.median(t128):.2f} for 4x the pixels")
            forms, forms128 = net.layer_forms(), net128.layer_forms()
            # time up to the end of each group of rows (prefix runs through pa_convnet_trace, each with the copy of the pooled vector)
            ends = {"stem": 0}
            i = 1
            for li, blocks in enumerate((3, 4, 6, 3), start=1):
                i += 3 * blocks + 1
                ends[f"layer{li}"] = i - 1
            pooled = descs[-1]["out_buf"]
            prev = statistics.median(timed(lambda: net.trace(x, -1, pooled), 10, windows=3))
            say(f"    input conversion (+ the trace's copy): {prev:.3f} ms")
            for name, last in ends.items():
                cur = statistics.median(timed(lambda: net.trace(x, last, pooled), 5, windows=3))
                say(f"    through {name}: {cur:.3f} ms (+{cur - prev:.3f})")
                if name == "stem":
                    say(f"    share of the stem row: {(cur - prev) / statistics.median(t) * 100:.1f} % of the call")
                prev = cur
            say("    forms per row (256 | 128 where they differ):")
            for nm, d, a, b in zip(names, descs, forms, forms128):
                mark = "" if a == b or nm == "stem" else f"   | 128: {b}"
                say(f"      {nm:24s} {d['in_hw']:3d} px  {a}{mark}")
        finally:
            net.close()
            net128.close()
    say()


def main():
    say("# crop_any_size measurements (one MI355X, one process)")
    say()
    sd = synth.make_resformer_state_dict(seed=2468)
    crops_section()
    stem_section(sd)
    resnet_section(sd)
    if len(sys.argv) > 1:
        os.makedirs(os.path.dirname(os.path.abspath(sys.argv[1])), exist_ok=True)
        with open(sys.argv[1], "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
