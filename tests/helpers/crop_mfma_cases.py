"""Cases of tests/test_crop_mfma.py, shared with its child (crop_mfma_worker.py): two 360 x 640 frames, boxes in pixels, and a
CPU copy of the crop plan's geometry (csrc/preprocess.hip: crop_plan_kernel, band_rows, band_lds) to say which branch a box takes."""
import math

import numpy as np

from playaid_core_amd import synth

H, W = 360, 640
FUSED_LDS = 77824   # PA_FUSED_LDS_BYTES


def _box(cx, cy, w, h):
    """Normalised box whose yolo_pixels (int(v * size)) are exactly these pixels."""
    return ((cx + 0.5) / W, (cy + 0.5) / H, (w + 0.5) / W, (h + 0.5) / H)


# (name, padding, box). Padding 30 is the pipeline's; 100 makes the slice 2.25 x the square (11 taps).
CASES = [
    ("d129", 30, _box(200, 180, 129, 100)),          # slice starts at x = 106: byte 318, misaligned by 2; 387 bytes a row
    ("d160", 30, _box(201, 170, 120, 160)),          # x = 91: misaligned by 1; 480 bytes a row = 15 whole column blocks
    ("d191", 30, _box(301, 200, 191, 150)),          # x = 176: aligned; 573 bytes a row
    ("d150", 30, _box(206, 160, 150, 150)),          # x = 101: misaligned by 3
    ("vertical_only", 30, _box(710, 51, 160, 100)),   # 40 x 161 slice at the top right corner -> 40 x 160
    ("horizontal_only", 30, _box(51, 430, 160, 100)),  # 161 x 40 slice at the bottom left corner -> 160 x 40
    ("enlarging", 30, _box(20, 30, 200, 180)),       # 150 x 160 slice -> 188 x 200
    ("fallback", 30, _box(320, 180, 1280, 200)),     # 640 x 360 slice -> 1280 x 720: no sub-band fits the LDS budget
    ("wide_filter_a", 100, _box(320, 180, 160, 120)),
    ("wide_filter_b", 100, _box(300, 170, 100, 129)),
    ("d129_frame1", 30, _box(331, 190, 90, 129)),
    ("d191_frame1", 30, _box(420, 130, 191, 191)),
]
PADDINGS = (30, 100)


def frame_of(i):
    """Cases alternate between the two frames."""
    return i & 1


def frames():
    return synth.make_frames(2, H, W, seed=31)


def _bounds(i, o, xx):
    scale = float(np.float32(i)) / o
    sup = 2.0 * max(scale, 1.0)
    c = (xx + 0.5) * scale
    lo = max(int(c - sup + 0.5), 0)
    hi = min(int(c + sup + 0.5), i)
    return lo, hi - lo


def _ksize(i, o):
    return int(math.ceil(2.0 * max(float(np.float32(i)) / o, 1.0))) * 2 + 1


def _area_tab(dx, scale, ss):
    f1 = dx * scale
    f2 = f1 + scale
    sx2 = min(math.floor(f2), ss - 1)
    sx1 = min(math.ceil(f1), sx2)
    hf = 1 if sx1 - f1 > 1e-3 else 0
    hl = 1 if f2 - sx2 > 1e-3 else 0
    return sx1 - hf, hf + (sx2 - sx1) + hl


def _al(v, a):
    return (v + a - 1) // a * a


def plan(box, height, width, pad):
    cx, cy, cw, ch = int(box[0] * width), int(box[1] * height), int(box[2] * width), int(box[3] * height)
    d = max(cw, ch)
    half = d // 2
    y0, y1 = max(cy - half - pad, 0), min(cy + half + pad, height)
    x0, x1 = max(cx - half - pad, 0), min(cx + half + pad, width)
    x0, y0 = min(x0, width), min(y0, height)
    sh, sw = max(y1 - y0, 0), max(x1 - x0, 0)
    assert sh > 0 and sw > 0 and d >= 128
    rw = rh = d
    if sw > sh:
        nh = int(np.rint(sh / sw * d))
        rh = nh if nh != d else d
    elif sw < sh:
        nw = int(np.rint(sw / sh * d))
        rw = nw if nw != d else d
    if (sh, sw) == (d, d):
        rw = rh = d
    need_h, need_v = rw != sw, rh != sh
    py = int(np.rint((d - rh) * 0.5)) if (rw == d and rh != d) else 0
    out_h = int(d * (128.0 / d))
    scale_y = 1.0 / (out_h / d)
    p = dict(d=d, sx0=x0, sy0=y0, sw=sw, sh=sh, rw=rw, rh=rh, need_h=need_h, need_v=need_v, ksize_h=_ksize(sw, rw) if need_h else 0,
             ksize_v=_ksize(sh, rh) if need_v else 0)
    p0, p1 = _al(sw * 3, 4) + 4, _al(rw * 3, 4) + 4
    fits, n0_max, n2_max, over = None, 0, 0, False
    for rb in (8, 4, 2, 1):
        worst = 0
        for r0 in range(0, 128, rb):
            r1 = min(r0 + rb, out_h)
            if r0 >= r1:
                continue
            a, _ = _area_tab(r0, scale_y, d)
            s, n = _area_tab(r1 - 1, scale_y, d)
            ry0, ry1 = min(max(a - py, 0), rh), min(max(s + n - py, 0), rh)
            if ry1 <= ry0:
                continue
            if need_v:
                ty0 = _bounds(sh, rh, ry0)[0]
                m, c = _bounds(sh, rh, ry1 - 1)
                ty1 = m + c
            else:
                ty0, ty1 = ry0, ry1
            n0, n2 = ty1 - ty0, ry1 - ry0
            s0, s1, s2 = _al(n0 * p0, 16), _al(n0 * p1, 16), _al(n2 * p1, 16)
            if need_h and need_v:
                need = s0 + s1 + (s2 if s2 > s0 else 0)
                over = over or s2 > s0
            elif need_h:
                need = s0 + s1
            elif need_v:
                need = s0 + s2
            else:
                need = s0
            worst = max(worst, need)
            if rb == 8:
                n0_max, n2_max = max(n0_max, n0), max(n2_max, n2)
        if worst <= FUSED_LDS:
            fits = rb
            break
    p.update(fallback=fits is None, rb=fits, n0_max=n0_max, n2_max=n2_max, b2_over_b0=over)
    return p
