"""The detection network on the device: YOLOv5s as a layer table for ``pa_detector_*``.

The reference gets its boxes from ``python third_party/yolov5/detect.py --weights models/yolo/<...>.pt --source <video>
--max-det 2 --classes 2 3 ...`` (``playaid/ai_runner.py:191-224``; the checkout and the weights are not in the reference
tree). This module takes a YOLOv5s v7.0 state dict in the checkpoint's key layout (``model.<i>.conv.weight``,
``model.<i>.bn.*``, ``model.<i>.cv1 ...``, ``model.24.m.<k>.{weight,bias}``, ``model.24.anchors``), folds every BatchNorm
(eps 1e-3) into its convolution in float64, lays the weights out for the implicit-GEMM kernel and wires the graph of
``models/yolov5s.yaml`` as ``pa_net_layer`` rows over zero-bordered NHWC buffers in which every concatenation is a buffer
the producers write their channel slice of:

    frames (device, uint8 BGR) -> pa_detector_forward: letterbox, 6x6/2 stem, 57 convolutions on the matrix cores, SPPF
    max-pools, two nearest up-samplings, Detect decode -> pred[n, rows, 5 + nc] -> Engine.detect_postprocess (NMS ...)

``YoloV5Detector.labels(engine, frames)`` returns the label text the runner reads, ``detections`` the device table that
``detector_path.run_detections_to_labels`` takes: decode -> detect -> repair -> crops -> CNN -> labels without leaving the GPU.
The arithmetic contract is ``oracle/yolov5.py`` (live torch CPU kernels on the same state dict; parity unpinned: no
checkpoint, no YOLOv5 checkout). fp32 by default; ``compute_dtype="emulated_f32"`` keeps fp32 accuracy on the bf16 matrix
cores, ``compute_dtype="bf16"`` stores bf16 and multiplies bf16 (include/playaid_hip.h states its rounding model; its detections
are not within the fp32 path's 1e-4 bar).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Mapping, Tuple

import numpy as np
import torch

from . import _lib
from .engine import EngineError

BN_EPS = 1e-3
WIDTHS = (32, 64, 128, 256, 512)      # yolov5s: width_multiple 0.50 of (64, 128, 256, 512, 1024)
STRIDES = (8, 16, 32)


def _np(a) -> np.ndarray:
    return a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)


def _fold(sd: Mapping, prefix: str) -> Tuple[np.ndarray, np.ndarray]:
    """Conv (no bias) + BatchNorm(eval) -> (weight [c2, c1, k, k], bias [c2]) in float64."""
    w = _np(sd[prefix + ".conv.weight"]).astype(np.float64)
    g, b = _np(sd[prefix + ".bn.weight"]).astype(np.float64), _np(sd[prefix + ".bn.bias"]).astype(np.float64)
    m, v = _np(sd[prefix + ".bn.running_mean"]).astype(np.float64), _np(sd[prefix + ".bn.running_var"]).astype(np.float64)
    s = g / np.sqrt(v + BN_EPS)
    return w * s[:, None, None, None], b - m * s


class _Table:
    """Buffers, weights and layers while the graph is wired."""

    def __init__(self):
        self.layers: List[_lib.pa_net_layer] = []
        self.bufs: List[Tuple[int, int, int, int]] = []   # (h, w, pad, channels)
        self.weights: List[np.ndarray] = []
        self.n_weights = 0

    def buf(self, h, w, pad, c) -> int:
        self.bufs.append((h, w, pad, c))
        return len(self.bufs) - 1

    def put(self, a: np.ndarray) -> int:
        off = self.n_weights
        a = np.ascontiguousarray(a, dtype=np.float32).reshape(-1)
        pad = (-a.size) % 4   # 16-byte aligned rows for the vector loads
        self.weights.append(a)
        if pad:
            self.weights.append(np.zeros(pad, np.float32))
        self.n_weights += a.size + pad
        return off

    def conv(self, w, b, src, dst, k, s, act=2, res=None, res_after=0):
        """w [cout, cin, k, k] / b [cout] float64 (already padded to the kernel's multiples); src / dst / res = (buf, coff, c)."""
        cout, cin = w.shape[0], w.shape[1]
        assert cin % 32 == 0 and cout % 32 == 0 and src[2] == cin and dst[2] == cout, (w.shape, src, dst)
        ih, iw, ipad, ic = self.bufs[src[0]]
        oh, ow, opad, oc = self.bufs[dst[0]]
        assert (ih // s, iw // s) == (oh, ow) and ipad >= k // 2, (self.bufs[src[0]], self.bufs[dst[0]], k, s)
        L = _lib.pa_net_layer()
        L.kind, L.cin, L.cout, L.ksize, L.stride, L.in_h, L.in_w = 0, cin, cout, k, s, ih, iw
        L.in_buf, L.in_coff, L.in_cstride, L.in_pad = src[0], src[1], ic, ipad
        L.out_buf, L.out_coff, L.out_cstride, L.out_pad = dst[0], dst[1], oc, opad
        L.res_buf, L.res_coff = (res[0], res[1]) if res is not None else (-1, 0)
        if res is not None:
            assert self.bufs[res[0]] == self.bufs[dst[0]] and res[2] == cout
        L.act, L.res_after = act, res_after
        L.w_off = self.put(w.transpose(0, 2, 3, 1))
        L.b_off = self.put(b)
        self.layers.append(L)

    def move(self, kind, src, dst):
        ih, iw, ipad, ic = self.bufs[src[0]]
        oh, ow, opad, oc = self.bufs[dst[0]]
        L = _lib.pa_net_layer()
        L.kind, L.cin, L.cout, L.ksize, L.stride, L.in_h, L.in_w = kind, src[2], src[2], 5 if kind == 4 else 1, 1, ih, iw
        L.in_buf, L.in_coff, L.in_cstride, L.in_pad = src[0], src[1], ic, ipad
        L.out_buf, L.out_coff, L.out_cstride, L.out_pad = dst[0], dst[1], oc, opad
        L.res_buf = -1
        assert src[2] == dst[2] and (oh, ow) == ((ih * 2, iw * 2) if kind == 5 else (ih, iw))
        self.layers.append(L)


def _pad_rows(w, b, cout):
    if w.shape[0] == cout:
        return w, b
    wp = np.zeros((cout,) + w.shape[1:], np.float64)
    wp[: w.shape[0]] = w
    bp = np.zeros(cout, np.float64)
    bp[: b.shape[0]] = b
    return wp, bp


def build_yolov5s_table(sd: Mapping, net_hw: Tuple[int, int], nc: int):
    """-> (layers, buffer sizes in floats per image, weight blob float32, rows of pred per image)."""
    H, W = net_hw
    assert H % 32 == 0 and W % 32 == 0
    T = _Table()
    c1, c2, c3, c4, c5 = WIDTHS
    size = {2: (H // 2, W // 2), 4: (H // 4, W // 4), 8: (H // 8, W // 8), 16: (H // 16, W // 16), 32: (H // 32, W // 32)}

    def B(scale, pad, c):
        return T.buf(size[scale][0], size[scale][1], pad, c)

    def C3(prefix, src, dst, scale, cin, cout, n, shortcut):
        """src / dst slices; writes cv3's output into dst. cv1 and cv2 read the same input, so ONE convolution writes
        X = [cv1 | cv2]; every bottleneck reads X's first half through its 1x1 into R and its 3x3 writes that half back IN
        PLACE (adding it as the residual after the SiLU when the block has shortcuts), so cv3's input [bottlenecks | cv2] is
        X itself: no concatenation, no ping-pong buffers, src read once. (c_ = 32, model.2: the bottleneck's convolutions run
        on 32-channel tiles.)"""
        c_ = cout // 2
        w1, b1 = _fold(sd, prefix + ".cv1")
        w2, b2 = _fold(sd, prefix + ".cv2")
        w3, b3 = _fold(sd, prefix + ".cv3")
        X = B(scale, 0, 2 * c_)
        R = B(scale, 1, c_)
        T.conv(np.concatenate([w1, w2]), np.concatenate([b1, b2]), src, (X, 0, 2 * c_), 1, 1)
        for j in range(n):
            wa, ba = _fold(sd, f"{prefix}.m.{j}.cv1")
            T.conv(wa, ba, (X, 0, c_), (R, 0, c_), 1, 1)
            wb, bb = _fold(sd, f"{prefix}.m.{j}.cv2")
            T.conv(wb, bb, (R, 0, c_), (X, 0, c_), 3, 1, res=(X, 0, c_) if shortcut else None, res_after=1)
        T.conv(w3, b3, (X, 0, 2 * c_), dst, 1, 1)

    def conv(prefix, src, dst, k, s):
        w, b = _fold(sd, prefix)
        T.conv(w, b, src, dst, k, s)

    # concatenation buffers of the head (the backbone writes its skip connections straight into them)
    C12 = B(16, 1, 2 * c4)   # [up(model.10) | model.6]
    C16 = B(8, 1, 2 * c3)    # [up(model.14) | model.4]
    C19 = B(16, 0, 2 * c3)   # [model.18 | model.14]
    C22 = B(32, 0, 2 * c4)   # [model.21 | model.10]
    # backbone
    assert c1 == 32, "the direct stem kernel is built for 32 output channels"
    B0 = B(2, 1, c1)
    w0, b0 = _fold(sd, "model.0")
    # stem weights in the direct kernel's lane layout: lane = (kx half) * 32 + channel holds W[channel][c][ky][3 * half + j]
    # at ky * 9 + j * 3 + c (csrc/yolo.hip::stem6x6_direct_kernel)
    stem = np.zeros((2, 32, 56), np.float64)
    for half in range(2):
        stem[half, :, :54] = w0[:, :, :, 3 * half:3 * half + 3].transpose(0, 2, 3, 1).reshape(32, 54)
    L = _lib.pa_net_layer()
    L.kind, L.cin, L.cout, L.ksize, L.stride, L.in_h, L.in_w = 3, 3, c1, 6, 2, H, W
    L.in_buf, L.res_buf = -1, -1
    L.out_buf, L.out_coff, L.out_cstride, L.out_pad = B0, 0, c1, 1
    L.act = 2
    L.w_off, L.b_off = T.put(stem), T.put(b0)
    T.layers.append(L)
    B1 = B(4, 0, c2)
    conv("model.1", (B0, 0, c1), (B1, 0, c2), 3, 2)
    B2 = B(4, 1, c2)
    C3("model.2", (B1, 0, c2), (B2, 0, c2), 4, c2, c2, 1, True)
    B3 = B(8, 0, c3)
    conv("model.3", (B2, 0, c2), (B3, 0, c3), 3, 2)
    C3("model.4", (B3, 0, c3), (C16, c3, c3), 8, c3, c3, 2, True)
    B5 = B(16, 0, c4)
    conv("model.5", (C16, c3, c3), (B5, 0, c4), 3, 2)
    C3("model.6", (B5, 0, c4), (C12, c4, c4), 16, c4, c4, 3, True)
    B7 = B(32, 0, c5)
    conv("model.7", (C12, c4, c4), (B7, 0, c5), 3, 2)
    B8 = B(32, 0, c5)
    C3("model.8", (B7, 0, c5), (B8, 0, c5), 32, c5, c5, 1, True)
    # SPPF: x | pool(x) | pool(pool(x)) | pool(pool(pool(x))) side by side
    S9 = B(32, 0, 2 * c5)
    conv("model.9.cv1", (B8, 0, c5), (S9, 0, c4), 1, 1)
    for k in range(3):
        T.move(4, (S9, k * c4, c4), (S9, (k + 1) * c4, c4))
    B9 = B(32, 0, c5)
    conv("model.9.cv2", (S9, 0, 2 * c5), (B9, 0, c5), 1, 1)
    # head
    conv("model.10", (B9, 0, c5), (C22, c4, c4), 1, 1)
    T.move(5, (C22, c4, c4), (C12, 0, c4))
    B13 = B(16, 0, c4)
    C3("model.13", (C12, 0, 2 * c4), (B13, 0, c4), 16, 2 * c4, c4, 1, False)
    conv("model.14", (B13, 0, c4), (C19, c3, c3), 1, 1)
    T.move(5, (C19, c3, c3), (C16, 0, c3))
    B17 = B(8, 1, c3)
    C3("model.17", (C16, 0, 2 * c3), (B17, 0, c3), 8, 2 * c3, c3, 1, False)
    conv("model.18", (B17, 0, c3), (C19, 0, c3), 3, 2)
    B20 = B(16, 1, c4)
    C3("model.20", (C19, 0, 2 * c3), (B20, 0, c4), 16, 2 * c3, c4, 1, False)
    conv("model.21", (B20, 0, c4), (C22, 0, c4), 3, 2)
    B23 = B(32, 0, c5)
    C3("model.23", (C22, 0, 2 * c4), (B23, 0, c5), 32, 2 * c4, c5, 1, False)
    # Detect: one 1x1 convolution per scale (3 x (5 + nc) channels, padded to 64), then the decode
    no = 5 + nc
    assert 3 * no <= 64, "more classes than the 64-channel head slice holds"
    anchors = _np(sd["model.24.anchors"]).astype(np.float64)
    rows = 0
    for i, (feat, ch, scale) in enumerate(((B17, c3, 8), (B20, c4, 16), (B23, c5, 32))):
        D = B(scale, 0, 64)
        w = _np(sd[f"model.24.m.{i}.weight"]).astype(np.float64)
        b = _np(sd[f"model.24.m.{i}.bias"]).astype(np.float64)
        T.conv(*_pad_rows(w, b, 64), (feat, 0, ch), (D, 0, 64), 1, 1, act=0)
        L = _lib.pa_net_layer()
        L.kind, L.cin, L.cout, L.ksize, L.stride = 6, 64, 3 * no, 1, 1
        L.in_h, L.in_w = size[scale]
        L.in_buf, L.in_coff, L.in_cstride, L.in_pad = D, 0, 64, 0
        L.out_buf, L.res_buf = -1, -1
        L.aux[0] = float(STRIDES[i])
        for a in range(3):
            L.aux[1 + 2 * a] = float(anchors[i, a, 0] * STRIDES[i])
            L.aux[2 + 2 * a] = float(anchors[i, a, 1] * STRIDES[i])
        T.layers.append(L)
        rows += 3 * size[scale][0] * size[scale][1]
    buf_floats = [(h + 2 * p) * (w + 2 * p) * c for (h, w, p, c) in T.bufs]
    return T.layers, buf_floats, np.concatenate(T.weights), rows


# -- every YOLOv5 v6.0 / v7.0 P5 size (n / s / m / l / x, or any multiples) --------------------------------------------------
# models/yolov5{n,s,m,l,x}.yaml: one graph, scaled by depth_multiple (gd) and width_multiple (gw)
P5_SIZES = {"n": (0.33, 0.25), "s": (0.33, 0.50), "m": (0.67, 0.75), "l": (1.00, 1.00), "x": (1.33, 1.25)}
C3_LAYERS = (2, 4, 6, 8, 13, 17, 20, 23)          # the C3 blocks of the graph (first four: the backbone's, with shortcuts)
_C3_BASE = {2: 3, 4: 6, 6: 9, 8: 3, 13: 3, 17: 3, 20: 3, 23: 3}   # their yaml repeats before depth_multiple


def make_divisible(x: float, divisor: int = 8) -> int:
    """utils/general.py::make_divisible: the smallest multiple of divisor >= x."""
    return int(np.ceil(x / divisor) * divisor)


def p5_graph(gd: float, gw: float) -> Dict[str, object]:
    """What models/yolo.py::parse_model makes of the P5 yaml at (gd, gw): widths c1..c5 (make_divisible(c * gw, 8)) and the
    bottlenecks per C3 block (max(round(n * gd), 1))."""
    widths = tuple(make_divisible(c * gw, 8) for c in (64, 128, 256, 512, 1024))
    return {"widths": widths, "repeats": {i: max(round(n * gd), 1) for i, n in _C3_BASE.items()}}


def graph_of(sd: Mapping) -> Dict[str, object]:
    """The graph a P5 state dict holds, read from its shapes: widths c1..c5, bottlenecks per C3 block, nc."""
    out = lambda key: int(_np(sd[key]).shape[0])
    if "model.0.conv.conv.weight" in sd:
        raise ValueError("a v5.0-or-older model (Focus stem): only the v6.0 / v7.0 6x6 stem is supported")
    if "model.33.m.3.weight" in sd or "model.24.m.0.weight" not in sd:
        raise ValueError("not a P5 Detect head on model.24 (P6 models with four scales are not supported)")
    widths = tuple(out(f"model.{i}.conv.weight") for i in (0, 1, 3, 5, 7))
    repeats = {}
    for i in C3_LAYERS:
        n = 0
        while f"model.{i}.m.{n}.cv1.conv.weight" in sd:
            n += 1
        repeats[i] = n
    no3 = out("model.24.m.0.weight")
    if no3 % 3 or no3 // 3 < 6:
        raise ValueError(f"Detect head with {no3} output channels is not 3 x (5 + nc)")
    return {"widths": widths, "repeats": repeats, "nc": no3 // 3 - 5}


def _c32(c: int) -> int:
    return -(-c // 32) * 32


def build_yolov5_table(sd: Mapping, net_hw: Tuple[int, int], nc: int, real_masks: List = None):
    """``build_yolov5s_table`` for any YOLOv5 v6.0 / v7.0 P5 state dict: the widths and the bottlenecks per C3 block come from
    its shapes. Channel counts that are not multiples of 32 (c1 = 16 / 48 / 80 of n / m / x, C3 hidden widths) are padded to
    the next multiple: a slice holds its real channels first and zeros behind them, and every weight row, weight column and
    bias of a padded position is exactly 0 (SiLU(0) = 0, so the padding stays 0 through every layer and moves no result).
    A concatenation buffer is its producers' padded slices side by side; the consumer's weight columns follow that layout.
    The stem is one kind-3 row per 32 output channels (out_coff = 32 g). Detect slices hold max(64, 3 (5 + nc) rounded up to
    32) channels. For an s state dict the layers and the weight blob are those of ``build_yolov5s_table``, byte for byte.
    real_masks: if a list, gets (row index, real output rows bool[cout], real input columns bool[cin]) per kind-0 / kind-3 row."""
    H, W = net_hw
    assert H % 32 == 0 and W % 32 == 0
    g = graph_of(sd)
    if g["nc"] != nc:
        raise ValueError(f"the Detect head holds {g['nc']} classes, not nc = {nc}")
    if any(n < 1 for n in g["repeats"].values()):
        raise ValueError(f"a C3 block without bottlenecks: {g['repeats']}")
    T = _Table()
    size = {2: (H // 2, W // 2), 4: (H // 4, W // 4), 8: (H // 8, W // 8), 16: (H // 16, W // 16), 32: (H // 32, W // 32)}

    def B(scale, pad, c):
        return T.buf(size[scale][0], size[scale][1], pad, c)

    def S(buf, coff, *reals):
        """a slice of buf at coff holding the real channel groups `reals`, each padded to a multiple of 32, side by side"""
        segs, o = [], 0
        for r in reals:
            segs.append((o, r))
            o += _c32(r)
        return (buf, coff, o, tuple(segs))

    def lay(w, b, src, dst, k, s, act=2, res=None, res_after=0):
        """w [co, ci, k, k] / b [co] of the real channels -> the padded layout of the slices src / dst"""
        wp = np.zeros((dst[2], src[2], k, k), np.float64)
        bp = np.zeros(dst[2], np.float64)
        rows, cols = np.zeros(dst[2], bool), np.zeros(src[2], bool)
        i = 0
        for o, r in dst[3]:
            j = 0
            for oc, c in src[3]:
                wp[o:o + r, oc:oc + c] = w[i:i + r, j:j + c]
                j += c
            assert j == w.shape[1], (w.shape, src)
            bp[o:o + r] = b[i:i + r]
            rows[o:o + r] = True
            i += r
        assert i == w.shape[0], (w.shape, dst)
        for oc, c in src[3]:
            cols[oc:oc + c] = True
        if real_masks is not None:
            real_masks.append((len(T.layers), rows, cols))
        T.conv(wp, bp, src[:3], dst[:3], k, s, act, None if res is None else res[:3], res_after)

    def C3(prefix, src, dst, scale, n, shortcut):
        """as in build_yolov5s_table: X = [cv1 | cv2], the bottlenecks in place on X's first half, cv3 on X"""
        w1, b1 = _fold(sd, prefix + ".cv1")
        w2, b2 = _fold(sd, prefix + ".cv2")
        w3, b3 = _fold(sd, prefix + ".cv3")
        c_ = w1.shape[0]
        X = B(scale, 0, 2 * _c32(c_))
        R = B(scale, 1, _c32(c_))
        lay(np.concatenate([w1, w2]), np.concatenate([b1, b2]), src, S(X, 0, c_, c_), 1, 1)
        for j in range(n):
            wa, ba = _fold(sd, f"{prefix}.m.{j}.cv1")
            lay(wa, ba, S(X, 0, c_), S(R, 0, c_), 1, 1)
            wb, bb = _fold(sd, f"{prefix}.m.{j}.cv2")
            lay(wb, bb, S(R, 0, c_), S(X, 0, c_), 3, 1, res=S(X, 0, c_) if shortcut else None, res_after=1)
        lay(w3, b3, S(X, 0, c_, c_), dst, 1, 1)

    def conv(prefix, src, dst, k, s):
        w, b = _fold(sd, prefix)
        lay(w, b, src, dst, k, s)

    ch = lambda key: int(_np(sd[key]).shape[0])
    c1, c2, c3, c4, c5 = g["widths"]
    rep = g["repeats"]
    c6, c9, c10 = ch("model.6.cv3.conv.weight"), ch("model.9.cv1.conv.weight"), ch("model.10.conv.weight")
    c14, c18, c21 = ch("model.14.conv.weight"), ch("model.18.conv.weight"), ch("model.21.conv.weight")
    c4o = ch("model.4.cv3.conv.weight")
    # concatenation buffers of the head (the backbone writes its skip connections straight into them)
    C12 = B(16, 1, _c32(c10) + _c32(c6))     # [up(model.10) | model.6]
    C16 = B(8, 1, _c32(c14) + _c32(c4o))     # [up(model.14) | model.4]
    C19 = B(16, 0, _c32(c18) + _c32(c14))    # [model.18 | model.14]
    C22 = B(32, 0, _c32(c21) + _c32(c10))    # [model.21 | model.10]
    # backbone: the stem as one row per 32 output channels, each in the direct kernel's lane layout (build_yolov5s_table)
    B0 = B(2, 1, _c32(c1))
    w0, b0 = _fold(sd, "model.0")
    w0p, b0p = np.zeros((_c32(c1), 3, 6, 6)), np.zeros(_c32(c1))
    w0p[:c1], b0p[:c1] = w0, b0
    for gi in range(_c32(c1) // 32):
        stem = np.zeros((2, 32, 56), np.float64)
        for half in range(2):
            stem[half, :, :54] = w0p[32 * gi:32 * gi + 32, :, :, 3 * half:3 * half + 3].transpose(0, 2, 3, 1).reshape(32, 54)
        L = _lib.pa_net_layer()
        L.kind, L.cin, L.cout, L.ksize, L.stride, L.in_h, L.in_w = 3, 3, 32, 6, 2, H, W
        L.in_buf, L.res_buf = -1, -1
        L.out_buf, L.out_coff, L.out_cstride, L.out_pad = B0, 32 * gi, _c32(c1), 1
        L.act = 2
        if real_masks is not None:
            real_masks.append((len(T.layers), np.arange(32 * gi, 32 * gi + 32) < c1, np.ones(3, bool)))
        L.w_off, L.b_off = T.put(stem), T.put(b0p[32 * gi:32 * gi + 32])
        T.layers.append(L)
    B1 = B(4, 0, _c32(c2))
    conv("model.1", S(B0, 0, c1), S(B1, 0, c2), 3, 2)
    B2 = B(4, 1, _c32(c2))
    C3("model.2", S(B1, 0, c2), S(B2, 0, c2), 4, rep[2], True)
    B3 = B(8, 0, _c32(c3))
    conv("model.3", S(B2, 0, c2), S(B3, 0, c3), 3, 2)
    C3("model.4", S(B3, 0, c3), S(C16, _c32(c14), c4o), 8, rep[4], True)
    B5 = B(16, 0, _c32(c4))
    conv("model.5", S(C16, _c32(c14), c4o), S(B5, 0, c4), 3, 2)
    C3("model.6", S(B5, 0, c4), S(C12, _c32(c10), c6), 16, rep[6], True)
    B7 = B(32, 0, _c32(c5))
    conv("model.7", S(C12, _c32(c10), c6), S(B7, 0, c5), 3, 2)
    c8 = ch("model.8.cv3.conv.weight")
    B8 = B(32, 0, _c32(c8))
    C3("model.8", S(B7, 0, c5), S(B8, 0, c8), 32, rep[8], True)
    # SPPF: x | pool(x) | pool(pool(x)) | pool(pool(pool(x))) side by side
    p9 = _c32(c9)
    S9 = B(32, 0, 4 * p9)
    conv("model.9.cv1", S(B8, 0, c8), S(S9, 0, c9), 1, 1)
    for k in range(3):
        T.move(4, (S9, k * p9, p9), (S9, (k + 1) * p9, p9))
    c9o = ch("model.9.cv2.conv.weight")
    B9 = B(32, 0, _c32(c9o))
    conv("model.9.cv2", S(S9, 0, c9, c9, c9, c9), S(B9, 0, c9o), 1, 1)
    # head
    conv("model.10", S(B9, 0, c9o), S(C22, _c32(c21), c10), 1, 1)
    T.move(5, (C22, _c32(c21), _c32(c10)), (C12, 0, _c32(c10)))
    c13 = ch("model.13.cv3.conv.weight")
    B13 = B(16, 0, _c32(c13))
    C3("model.13", S(C12, 0, c10, c6), S(B13, 0, c13), 16, rep[13], False)
    conv("model.14", S(B13, 0, c13), S(C19, _c32(c18), c14), 1, 1)
    T.move(5, (C19, _c32(c18), _c32(c14)), (C16, 0, _c32(c14)))
    c17 = ch("model.17.cv3.conv.weight")
    B17 = B(8, 1, _c32(c17))
    C3("model.17", S(C16, 0, c14, c4o), S(B17, 0, c17), 8, rep[17], False)
    conv("model.18", S(B17, 0, c17), S(C19, 0, c18), 3, 2)
    c20 = ch("model.20.cv3.conv.weight")
    B20 = B(16, 1, _c32(c20))
    C3("model.20", S(C19, 0, c18, c14), S(B20, 0, c20), 16, rep[20], False)
    conv("model.21", S(B20, 0, c20), S(C22, 0, c21), 3, 2)
    c23 = ch("model.23.cv3.conv.weight")
    B23 = B(32, 0, _c32(c23))
    C3("model.23", S(C22, 0, c21, c10), S(B23, 0, c23), 32, rep[23], False)
    # Detect: one 1x1 convolution per scale into a head slice of hd channels, then the decode
    no = 5 + nc
    hd = max(64, _c32(3 * no))
    anchors = _np(sd["model.24.anchors"]).astype(np.float64)
    rows = 0
    for i, (feat, c, scale) in enumerate(((B17, c17, 8), (B20, c20, 16), (B23, c23, 32))):
        D = B(scale, 0, hd)
        w = _np(sd[f"model.24.m.{i}.weight"]).astype(np.float64)
        b = _np(sd[f"model.24.m.{i}.bias"]).astype(np.float64)
        lay(w, b, S(feat, 0, c), (D, 0, hd, ((0, 3 * no),)), 1, 1, act=0)
        L = _lib.pa_net_layer()
        L.kind, L.cin, L.cout, L.ksize, L.stride = 6, hd, 3 * no, 1, 1
        L.in_h, L.in_w = size[scale]
        L.in_buf, L.in_coff, L.in_cstride, L.in_pad = D, 0, hd, 0
        L.out_buf, L.res_buf = -1, -1
        L.aux[0] = float(STRIDES[i])
        for a in range(3):
            L.aux[1 + 2 * a] = float(anchors[i, a, 0] * STRIDES[i])
            L.aux[2 + 2 * a] = float(anchors[i, a, 1] * STRIDES[i])
        T.layers.append(L)
        rows += 3 * size[scale][0] * size[scale][1]
    buf_floats = [(h + 2 * p) * (w + 2 * p) * c for (h, w, p, c) in T.bufs]
    return T.layers, buf_floats, np.concatenate(T.weights), rows


def buffer_geometry(layers) -> Dict[int, Tuple[int, int, int, int]]:
    """buffer -> (h, w, pad, channels per pixel) as the table's rows address it (every row touching a buffer agrees)."""
    geo = {}
    for L in layers:
        if L.kind in (0, 4, 5, 6):
            geo[L.in_buf] = (L.in_h, L.in_w, L.in_pad, L.in_cstride)
        if L.kind in (0, 3, 4, 5):
            s = 2 if L.kind == 3 else max(L.stride, 1)
            oh, ow = (L.in_h * 2, L.in_w * 2) if L.kind == 5 else (L.in_h // s, L.in_w // s)
            geo[L.out_buf] = (oh, ow, L.out_pad, L.out_cstride)
    return geo


class YoloV5Detector:
    """``pa_detector_*`` handle for a YOLOv5 v6.0 / v7.0 P5 state dict of any size (n / s / m / l / x or custom multiples; up to
    80 classes). ``net_hw``: the network input (what ``letterbox(auto=True)`` picks for the clip: 384 x 640 for 16:9 frames at
    ``--imgsz 640``). ``load_from_checkpoint`` takes an ultralytics ``.pt`` directly."""

    def __init__(self, state_dict: Mapping, nc: int, net_hw: Tuple[int, int] = (384, 640), max_images: int = 64, device: str = "cuda:0",
                 compute_dtype: str = "f32", buf_slack: int = 0, names: List[str] = None):
        """buf_slack: floats added to every buffer's share per image (tests: a table whose buffers are larger than the geometry
        their rows address, which the public table API allows). names: the class names, if known (``self.names``)."""
        self._lib = _lib.load()
        if compute_dtype not in ("f32", "emulated_f32", "bf16"):
            raise ValueError("compute_dtype must be 'f32', 'emulated_f32' or 'bf16'")
        self.compute_dtype = compute_dtype
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no HIP device visible to PyTorch-ROCm; the detection network has no CPU fallback")
        self.device = torch.device(device)
        self.nc, self.net_hw, self.max_images = nc, tuple(net_hw), max_images
        self.names = list(names) if names is not None else None
        layers, buf_floats, weights, rows = build_yolov5_table(state_dict, self.net_hw, nc)
        buf_floats = [b + buf_slack for b in buf_floats]
        self.rows = rows
        self.layers, self.weights = layers, weights
        self.buf_geometry = buffer_geometry(layers)
        # element type of each buffer as stored: bf16 under compute_dtype="bf16" except the Detect heads' (what a decode row reads)
        head_bufs = {L.in_buf for L in layers if L.kind == 6}
        self.buf_dtype = {b: torch.float32 if compute_dtype != "bf16" or b in head_bufs else torch.bfloat16 for b in self.buf_geometry}
        arr = (_lib.pa_net_layer * len(layers))(*layers)
        bf = (C.c_int64 * len(buf_floats))(*buf_floats)
        h = C.c_void_p()
        torch.cuda.set_device(self.device)
        rc = self._lib.pa_detector_create_dtype(self.device.index or 0, arr, len(layers), bf, len(buf_floats), weights.ctypes.data_as(C.c_void_p),
                                                weights.size, max_images, self.net_hw[0], self.net_hw[1], nc, _lib.DTYPES[compute_dtype], C.byref(h))
        self._h = h
        if rc != 0:
            msg = self._lib.pa_detector_last_error(h).decode() if h else "bad argument"
            self.close()
            raise EngineError(rc, msg)
        assert self._lib.pa_detector_rows(self._h) == rows
        self.n_layers = len(layers)
        # multiply-adds the table executes per image (padding channels included) and the ones the graph defines
        self.flops_per_image = 0.0
        for L in layers:
            oh, ow = L.in_h // max(L.stride, 1), L.in_w // max(L.stride, 1)
            if L.kind == 0:
                self.flops_per_image += 2.0 * oh * ow * L.cout * L.ksize * L.ksize * L.cin
            elif L.kind == 3:
                self.flops_per_image += 2.0 * oh * ow * L.cout * 108

    @classmethod
    def load_from_checkpoint(cls, path, net_hw: Tuple[int, int] = (384, 640), max_images: int = 64, device: str = "cuda:0",
                             compute_dtype: str = "f32") -> "YoloV5Detector":
        """An ultralytics YOLOv5 v6.x / v7.0 ``.pt`` (or a bare state dict saved with ``torch.save``), read without the YOLOv5
        checkout (``yolov5_checkpoint.load_yolov5_checkpoint``: what it refuses, and why, is listed there)."""
        from .yolov5_checkpoint import load_yolov5_checkpoint

        sd, meta = load_yolov5_checkpoint(path)
        det = cls(sd, meta["nc"], net_hw, max_images=max_images, device=device, compute_dtype=compute_dtype, names=meta["names"])
        det.meta = meta
        return det

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pa_detector_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def forward(self, frames) -> torch.Tensor:
        """frames uint8[n,H,W,3] BGR (device tensor or numpy) -> pred float32[n, rows, 5 + nc] on the device."""
        fd = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
        fd = fd.to(self.device).contiguous()
        n, h, w, _ = fd.shape
        out = torch.empty((n, self.rows, 5 + self.nc), dtype=torch.float32, device=self.device)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        for f0 in range(0, n, self.max_images):
            cnt = min(self.max_images, n - f0)
            rc = self._lib.pa_detector_forward(self._h, C.c_void_p(fd[f0:].data_ptr()), cnt, h, w, C.c_void_p(out[f0:].data_ptr()), stream)
            if rc != 0:
                raise EngineError(rc, self._lib.pa_detector_last_error(self._h).decode())
        return out

    __call__ = forward

    def trace(self, frames, last_layer: int, buf: int, img0: int = 0, n_img: int = None, pred: torch.Tensor = None):
        """Test aid (``pa_detector_trace``): run what ``forward`` runs for frames uint8[n,H,W,3] (n <= max_images, one range)
        through table row ``last_layer`` (-1: the letterbox alone) and return ``(images [img0, img0 + n_img) of buffer buf as
        stored, the last row run)``: [n_img][h + 2 pad][w + 2 pad][channels] of ``buf_dtype[buf]`` (float32; bfloat16 under
        compute_dtype="bf16" except the Detect heads' buffers), or for buf = -1 the letter-boxed input [n_img][net_h + 4][net_w + 4][4]
        (bfloat16 pixel integers under the bf16 stem of "emulated_f32" and "bf16"). ``pred``: where
        decode rows write (a new [n, rows, 5 + nc] tensor if None; its rows past the decoded ones are left as they are)."""
        fd = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames))
        fd = fd.to(self.device).contiguous()
        n, h, w, _ = fd.shape
        n_img = self.max_images - img0 if n_img is None else n_img
        if buf < 0:
            shape, dt = (max(n_img, 0), self.net_hw[0] + 4, self.net_hw[1] + 4, 4), torch.float32
            if self.compute_dtype in ("emulated_f32", "bf16"):
                dt = torch.bfloat16
        else:
            gh, gw, gp, gc = self.buf_geometry[buf]
            shape, dt = (max(n_img, 0), gh + 2 * gp, gw + 2 * gp, gc), self.buf_dtype[buf]
        out = torch.empty(shape, dtype=dt, device=self.device)
        if pred is None:
            pred = torch.zeros((n, self.rows, 5 + self.nc), dtype=torch.float32, device=self.device)
        done = C.c_int32(-2)
        stream = C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)
        rc = self._lib.pa_detector_trace(self._h, C.c_void_p(fd.data_ptr()), n, h, w, last_layer, buf, img0, n_img, C.c_void_p(out.data_ptr()),
                                         out.numel() * out.element_size(), C.c_void_p(pred.data_ptr()), C.byref(done), stream)
        if rc != 0:
            raise EngineError(rc, self._lib.pa_detector_last_error(self._h).decode())
        return out, done.value

    def layer_forms(self) -> List[str]:
        """The kernel form (``_lib.DET_FORMS``) each table row ran as in the last forward or trace."""
        forms = (C.c_int32 * self.n_layers)()
        rc = self._lib.pa_detector_layer_forms(self._h, forms, self.n_layers)
        if rc != 0:
            raise EngineError(rc, "pa_detector_layer_forms")
        return [_lib.DET_FORMS[f] for f in forms]

    def detections(self, engine, frames, conf_thres: float = 0.25, iou_thres: float = 0.45, classes=(2, 3), max_det: int = 2):
        """-> (dets float32[n, max_det, 6], counts int32[n]) on the device: ``detect.py``'s label rows (``ai_runner.py:209-217``).
        classes: the class ids kept (0..79), None = every class (``detect.py`` without ``--classes``)."""
        fd = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(frames)).to(self.device)
        pred = self.forward(fd)
        return engine.detect_postprocess(pred, self.net_hw, (fd.shape[1], fd.shape[2]), conf_thres, iou_thres, classes, max_det)

    def labels(self, engine, frames, **kw) -> List[str]:
        from .detect import label_lines

        dets, counts = self.detections(engine, frames, **kw)
        torch.cuda.synchronize(self.device)
        d, c = dets.cpu().numpy(), counts.cpu().numpy()
        return [label_lines(d[i, : c[i]]) for i in range(d.shape[0])]
