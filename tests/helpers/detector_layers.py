"""Float64 references for the detector's layer table, and the per-layer checker behind tests/test_detector_layers.py (imported
there and by its knob child, tests/helpers/detector_knob_worker.py).

Every row's reference is built from the buffers as the device stored them after the row before (``YoloV5Detector.trace``),
interior only, with the weights read from the table's fp32 blob in the device layouts: ``[cout][ky][kx][cin]`` per
convolution, the stem's lane layout ``[kx // 3][cout][ky * 9 + (kx % 3) * 3 + c]``.

Bars (each row, per case):
  * model input: bitwise ``oracle.yolov5.letterbox`` (fp32 / 255), or 255 x that as bf16 integers; border and channel 3 zero.
  * convolutions (kinds 0 and 3): ``max|got - ref| <= 2e-5 * max|ref|`` over the written slice's interior (the conv bar of
    test_wino.py, test_psgemm.py, test_backbone_layers.py); the Detect heads' padding channels exactly 0.
  * max-pools and up-samplings, fused or not: bitwise the max / copy of the stored input.
  * decode: see ``decode_bar``.
  * every row: a written buffer with a border keeps it exactly zero; channels outside the written slices and images
    [n, max_images) are bitwise what they were before the row.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

CONV_BAR = 2e-5
U32 = 2.0 ** -24


# -- weights in the device layouts --------------------------------------------------------------------
def row_weights(L, blob):
    """(w [cout][cin][k][k], b [cout]) float64 of a kind-0 or kind-3 row, read from the fp32 blob as the kernels read it."""
    blob = np.asarray(blob)
    if L.kind == 3:
        lane = blob[L.w_off:L.w_off + 64 * 56].astype(np.float64).reshape(2, 32, 56)
        w = np.zeros((32, 3, 6, 6))
        for half in range(2):
            w[:, :, :, 3 * half:3 * half + 3] = lane[half, :, :54].reshape(32, 6, 3, 3).transpose(0, 3, 1, 2)
        return w, blob[L.b_off:L.b_off + 32].astype(np.float64)
    k = L.ksize
    w = blob[L.w_off:L.w_off + L.cout * k * k * L.cin].astype(np.float64).reshape(L.cout, k, k, L.cin).transpose(0, 3, 1, 2)
    return np.ascontiguousarray(w), blob[L.b_off:L.b_off + L.cout].astype(np.float64)


# -- float64 operations on NHWC arrays ---------------------------------------------------------------
def _nchw(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64)).permute(0, 3, 1, 2)


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().numpy()


def activation(y, act):
    if act == 1:
        return np.maximum(y, 0.0)
    if act == 2:
        return y / (1.0 + np.exp(-y))
    return y


def ref_stem(x, w, b):
    """x [n][H][W][3] float64 (letter-boxed, 0..1) -> SiLU(conv 6x6 / 2, padding 2) [n][H/2][W/2][32]."""
    return activation(_nhwc(F.conv2d(_nchw(x), torch.from_numpy(w), torch.from_numpy(b), stride=2, padding=2)), 2)


def ref_conv(x, w, b, stride, act, res=None, res_after=1):
    """x: the input slice's interior [n][h][w][cin]; res: the residual slice [n][oh][ow][cout] or None."""
    y = _nhwc(F.conv2d(_nchw(x), torch.from_numpy(w), torch.from_numpy(b), stride=stride, padding=w.shape[-1] // 2))
    if res is not None and not res_after:
        y = y + res
    y = activation(y, act)
    if res is not None and res_after:
        y = y + res
    return y


def maxpool5(x):
    """nn.MaxPool2d(5, 1, 2) of [n][h][w][c] (exact in any precision: a max rounds nothing)."""
    t = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
    return F.max_pool2d(t.permute(0, 3, 1, 2), 5, 1, 2).permute(0, 2, 3, 1)


def upsample2(x):
    return x.repeat_interleave(2, dim=1).repeat_interleave(2, dim=2)


def ref_decode(v, stride, anchors):
    """Detect decode of one scale in float64: v [n][h][w][3 * no] (the head's output) -> rows [n][3 * h * w][no]."""
    n, h, w, c = v.shape
    no = c // 3
    s = 1.0 / (1.0 + np.exp(-v.reshape(n, h, w, 3, no).astype(np.float64)))
    out = s.copy()
    gx = np.arange(w, dtype=np.float64)[None, None, :, None] - 0.5
    gy = np.arange(h, dtype=np.float64)[None, :, None, None] - 0.5
    out[..., 0] = (s[..., 0] * 2 + gx) * stride
    out[..., 1] = (s[..., 1] * 2 + gy) * stride
    a = np.asarray(anchors, np.float64).reshape(3, 2)
    out[..., 2] = (s[..., 2] * 2) ** 2 * a[:, 0]
    out[..., 3] = (s[..., 3] * 2) ** 2 * a[:, 1]
    return out.transpose(0, 3, 1, 2, 4).reshape(n, 3 * h * w, no), s.transpose(0, 3, 1, 2, 4).reshape(n, 3 * h * w, no)


def decode_bar(ref, s, v, stride, anchors):
    """Element bar of detect_decode_kernel (fp32, -ffp-contract=off) against ref_decode, from its operations; u = 2^-24:
      * expf(-v): at most (2 + |v|) u relative (a correctly rounded libm is within 1 u; a 2^x-based one adds the rounding of
        the argument, |v| u); 1 + e and 1 / (...) one rounding each. d s / s = e / (1 + e) * d e / e, so s is within
        r_s = (4 + |v|) u of its value, relative;
      * scores (k >= 4): r_s * s;
      * x, y: 2 s exact, + (x - 0.5) one rounding, * stride (a power of two) exact: stride * (2 r_s s + u |2 s + g|);
      * w, h: (2 s)^2 one rounding, * anchor one rounding (the anchor as stored, fp32): (2 r_s + 2 u) * |ref|;
      * + 1e-30 absolute: a flushed denormal s, or expf overflowing for v < -88, where s < 1e-38 (second-order terms of u are
        below a 1 % margin on the first-order sum, taken as the factor 1.01)."""
    n, rows, no = ref.shape
    r_s = (4.0 + np.abs(v)) * U32
    bar = r_s * s
    t0 = ref[..., 0] / stride
    t1 = ref[..., 1] / stride
    bar[..., 0] = stride * (2 * r_s[..., 0] * s[..., 0] + U32 * np.abs(t0))
    bar[..., 1] = stride * (2 * r_s[..., 1] * s[..., 1] + U32 * np.abs(t1))
    bar[..., 2] = (2 * r_s[..., 2] + 2 * U32) * np.abs(ref[..., 2])
    bar[..., 3] = (2 * r_s[..., 3] + 2 * U32) * np.abs(ref[..., 3])
    return 1.01 * bar + 1e-30


def _v_rows(v):
    n, h, w, c = v.shape
    no = c // 3
    return v.reshape(n, h, w, 3, no).transpose(0, 3, 1, 2, 4).reshape(n, 3 * h * w, no).astype(np.float64)


# -- the table as a float64 interpreter (CPU) ----------------------------------------------------------
def geometry(layers):
    from playaid_core_amd.yolov5 import buffer_geometry

    return buffer_geometry(layers)


def interpret(layers, blob, x, nc):
    """The table's rows in float64 on their own outputs: x float64 [n][3][H][W] letter-boxed -> pred [n][rows][5 + nc]."""
    geo = geometry(layers)
    n = x.shape[0]
    bufs = {b: np.zeros((n, h + 2 * p, w + 2 * p, c)) for b, (h, w, p, c) in geo.items()}

    def get(b, coff, c, pad):
        a = bufs[b]
        return a[:, pad:a.shape[1] - pad, pad:a.shape[2] - pad, coff:coff + c]

    def put(b, coff, pad, y):
        a = bufs[b]
        a[:, pad:a.shape[1] - pad, pad:a.shape[2] - pad, coff:coff + y.shape[-1]] = y

    rows = []
    x_nhwc = np.ascontiguousarray(np.asarray(x, np.float64).transpose(0, 2, 3, 1))
    for L in layers:
        if L.kind == 3:
            w, b = row_weights(L, blob)
            put(L.out_buf, L.out_coff, L.out_pad, ref_stem(x_nhwc, w, b))
        elif L.kind == 0:
            w, b = row_weights(L, blob)
            res = get(L.res_buf, L.res_coff, L.cout, L.out_pad).copy() if L.res_buf >= 0 else None
            y = ref_conv(get(L.in_buf, L.in_coff, L.cin, L.in_pad), w, b, L.stride, L.act, res, L.res_after)
            put(L.out_buf, L.out_coff, L.out_pad, y)
        elif L.kind == 4:
            put(L.out_buf, L.out_coff, L.out_pad, maxpool5(get(L.in_buf, L.in_coff, L.cin, L.in_pad).copy()).numpy())
        elif L.kind == 5:
            put(L.out_buf, L.out_coff, L.out_pad, upsample2(torch.from_numpy(get(L.in_buf, L.in_coff, L.cin, L.in_pad).copy())).numpy())
        elif L.kind == 6:
            rows.append(ref_decode(get(L.in_buf, L.in_coff, 3 * (5 + nc), L.in_pad), L.aux[0], list(L.aux[1:7]))[0])
    return np.concatenate(rows, axis=1)


# -- the per-layer comparison ----------------------------------------------------------------------------
class LayerFault(AssertionError):
    pass


def conv_ratio(got, ref, what):
    """max|got - ref| over the conv bar; raises LayerFault past it or when the reference is mostly zero (an idle check)."""
    ref = np.asarray(ref, np.float64)
    if not (ref != 0).mean() > 0.2:
        raise LayerFault(f"{what}: the reference is mostly zero, the check would be idle")
    ratio = float(np.abs(np.asarray(got, np.float64) - ref).max() / (CONV_BAR * np.abs(ref).max()))
    if not ratio <= 1.0:
        raise LayerFault(f"{what}: max|err| = {ratio:.3g} x the 2e-5 bar")
    return ratio


def _interior(a, pad):
    return a[:, pad:a.shape[1] - pad, pad:a.shape[2] - pad]


def check_written(before, after, n, pad, slices, what):
    """A buffer a row (or fused group) wrote, whole capacity, as stored before and after it: the border stays zero, channels
    outside the written slices [(coff, c), ...] and images [n, capacity) are bitwise unchanged. torch or numpy arrays."""
    eq = (lambda a, b: bool(torch.equal(a, b))) if isinstance(after, torch.Tensor) else (lambda a, b: np.array_equal(a, b))
    nz = (lambda a: bool(a.any())) if isinstance(after, torch.Tensor) else (lambda a: bool(np.any(a)))
    if pad:
        for part in (after[:, :pad], after[:, -pad:], after[:, :, :pad], after[:, :, -pad:]):
            if nz(part):
                raise LayerFault(f"{what}: non-zero border")
    keep = np.ones(after.shape[-1], bool)
    for coff, c in slices:
        keep[coff:coff + c] = False
    lo = 0
    while lo < keep.size:   # runs of untouched channels
        if not keep[lo]:
            lo += 1
            continue
        hi = lo
        while hi < keep.size and keep[hi]:
            hi += 1
        if not eq(after[:n, ..., lo:hi], before[:n, ..., lo:hi]):
            raise LayerFault(f"{what}: channels {lo}..{hi - 1} outside the written slice changed")
        lo = hi
    if not eq(after[n:], before[n:]):
        raise LayerFault(f"{what}: images past n = {n} changed")


def check_conv_row(L, blob, before, after_out, n, idx, what, no=None):
    """A convolution row (kind 0) against float64. before: buffer -> stored array after the row before (host, float64 or
    float32, whole capacity); after_out: its output buffer after the row. idx: the images checked against float64.
    no: 5 + nc for the Detect heads (channels 3 * no .. cout must be exactly 0). Returns the ratio to the conv bar."""
    check_written(before[L.out_buf], after_out, n, L.out_pad, [(L.out_coff, L.cout)], what)
    w, b = row_weights(L, blob)
    x = _interior(before[L.in_buf][idx], L.in_pad)[..., L.in_coff:L.in_coff + L.cin]
    res = None
    if L.res_buf >= 0:
        res = _interior(before[L.res_buf][idx], L.out_pad)[..., L.res_coff:L.res_coff + L.cout].astype(np.float64)
    ref = ref_conv(x, w, b, L.stride, L.act, res, L.res_after)
    got = _interior(after_out[idx], L.out_pad)[..., L.out_coff:L.out_coff + L.cout]
    c = L.cout
    if no is not None and 3 * no < c:
        c = 3 * no
        if np.any(got[..., c:]):
            raise LayerFault(f"{what}: the head's padding channels are not zero")
    return conv_ratio(got[..., :c], ref[..., :c], what)


# -- the device walk ----------------------------------------------------------------------------------------
def sample_images(n):
    """Images checked against float64: all of a small batch; of a large one the first and last two and both sides of the
    middle, where the persistent GEMMs' 128-pixel tiles and 32-pixel runs straddle image boundaries on the small maps
    (240 and 960 pixels per image at 384 x 640: odd image boundaries fall inside a tile)."""
    if n <= 4:
        return np.arange(n)
    m = n // 2
    return np.array(sorted({0, 1, m - 1, m, m + 1, n - 2, n - 1}))


class _Trace:
    """States after whole rows, fetched with ``det.trace`` in non-decreasing row order (so every call leaves the handle's
    buffers exactly as the fetched states say: the rows run again rewrite what they wrote, bit for bit)."""

    def __init__(self, det, frames, n):
        self.det, self.frames, self.n = det, frames, n
        self.pred = torch.zeros((n, det.rows, 5 + det.nc), dtype=torch.float32, device=det.device)
        self.cache = {}
        self.last = -2

    def get(self, j, b):
        """-> (device tensor of buffer b, whole capacity, after row j; the row the call actually ended at)."""
        if (j, b) in self.cache:
            return self.cache[(j, b)], j
        assert j >= self.last, (j, self.last)
        out, done = self.det.trace(self.frames, j, b, 0, self.det.max_images, pred=self.pred)
        self.last = j
        self.cache[(done, b)] = out
        return out, done

    def drop_before(self, j):
        for key in [k for k in self.cache if k[0] < j]:
            del self.cache[key]


def check_model_input(det, frames_np, tag, x0=None, idx=None, want=None):
    """The model input of a detector of any compute dtype on frames uint8[n,H,W,3]: the stem's 2-pixel border and channel 3
    zero, the interior bitwise ``oracle.yolov5.letterbox`` -- fp32 / 255 ("f32"), or 255 x that as bf16 pixel integers
    ("emulated_f32", "bf16"). x0: the stored input (``det.trace(frames, -1, -1)``; fetched when None). idx: the images compared
    (default ``sample_images``). want: the oracle's letterbox of those images, [len(idx)][3][H][W], when the caller has it.
    -> the interior of those images as stored, float32 [len(idx)][net_h][net_w][3]. Raises LayerFault."""
    from oracle import yolov5 as oy

    n = frames_np.shape[0]
    idx = sample_images(n) if idx is None else np.asarray(idx)
    if x0 is None:
        x0, _ = det.trace(torch.from_numpy(np.ascontiguousarray(frames_np)).to(det.device), -1, -1, 0, det.max_images)
    if det.compute_dtype == "bf16" and x0.dtype != torch.bfloat16:
        raise LayerFault(f"{tag} input: stored as {x0.dtype}, not bf16")
    if bool(x0[..., 3].any()) or bool(x0[:, :2].any()) or bool(x0[:, -2:].any()) or bool(x0[:, :, :2].any()) or bool(x0[:, :, -2:].any()):
        raise LayerFault(f"{tag} input: border or channel 3 not zero")
    x0h = x0[torch.as_tensor(idx, device=x0.device)].float().cpu().numpy()
    if want is None:
        want = np.stack([oy.letterbox(frames_np[i], det.net_hw) for i in idx])
    want = np.asarray(want).transpose(0, 2, 3, 1)
    got = x0h[:, 2:-2, 2:-2, :3]
    if det.compute_dtype in ("emulated_f32", "bf16"):
        if not np.array_equal(got, np.rint(want.astype(np.float64) * 255).astype(np.float32)):
            raise LayerFault(f"{tag} input: not the letterbox's pixel integers")
        if det.compute_dtype == "emulated_f32" and not np.array_equal(got / np.float32(255), want):
            raise LayerFault(f"{tag} input: not the letterbox's pixel integers")
    elif not np.array_equal(got, want):
        raise LayerFault(f"{tag} input: not bitwise the letterbox")
    return got


def check_detector(det, frames_np, tag, log=print):
    """Walks every row of det's table on frames uint8[n,H,W,3] and checks it; returns
    {"forms": [per row], "ratios": {form: worst conv ratio}, "decode": worst decode ratio}. Raises LayerFault (naming row,
    kind and form) on the first failure."""
    n = frames_np.shape[0]
    frames = torch.from_numpy(np.ascontiguousarray(frames_np)).to(det.device)
    layers, blob, nc = det.layers, det.weights, det.nc
    no = 5 + nc
    idx = sample_images(n)
    tr = _Trace(det, frames, n)
    host = lambda t, sel=idx: t[torch.as_tensor(sel, device=t.device)].float().cpu().numpy()
    emu_stem = det.compute_dtype == "emulated_f32"
    # the model input
    x0, _ = tr.get(-1, -1)
    got = check_model_input(det, frames_np, tag, x0=x0, idx=idx)
    x_in = got.astype(np.float64) / 255.0 if emu_stem else got.astype(np.float64)
    ratios, dec_worst, row0 = {}, 0.0, 0
    per_row = {}
    k = 0
    while k < len(layers):
        L = layers[k]
        need = {L.in_buf} if L.kind != 3 else set()
        if L.kind in (0, 3, 4, 5):
            need.add(L.out_buf)
        if L.kind == 0 and L.res_buf >= 0:
            need.add(L.res_buf)
        if L.kind == 0 and k + 1 < len(layers) and layers[k + 1].kind == 5:
            need.add(layers[k + 1].out_buf)
        before = {b: tr.get(k - 1, b)[0] for b in sorted(need)}
        target = L.out_buf if L.kind != 6 else L.in_buf
        after_out, e = tr.get(k, target)
        forms = det.layer_forms()
        form = forms[k]
        what = f"{tag} row {k} (kind {L.kind}, {form})"
        if L.kind in (0, 3):
            bh = {b: host(t) for b, t in before.items()}
            check_written(before[L.out_buf], after_out, n, L.out_pad, [(L.out_coff, L.cout)], what)
            if L.kind == 3:
                w, b = row_weights(L, blob)
                got = _interior(host(after_out), L.out_pad)[..., L.out_coff:L.out_coff + L.cout]
                r = conv_ratio(got, ref_stem(x_in, w, b), what)
            else:
                r = check_conv_row(L, blob, bh, host(after_out), len(idx), np.arange(len(idx)), what,
                                   no=no if L.act == 0 and L.cout == 64 and any(M.kind == 6 and M.in_buf == L.out_buf for M in layers) else None)
            ratios[form] = max(ratios.get(form, 0.0), r)
            per_row[k] = r
            if e == k + 1:   # the next row's up-sampling, written by this launch
                U = layers[k + 1]
                ua, _ = tr.get(k, U.out_buf)
                check_written(before[U.out_buf], ua, n, U.out_pad, [(U.out_coff, U.cin)], what + " fused up-sampling")
                src = _interior(after_out[:n], L.out_pad)[..., L.out_coff:L.out_coff + L.cout]
                if not torch.equal(_interior(ua[:n], U.out_pad)[..., U.out_coff:U.out_coff + U.cin], upsample2(src)):
                    raise LayerFault(f"{what}: the fused up-sampling is not a copy of the stored output")
        elif L.kind in (4, 5):
            group = layers[k:e + 1]
            check_written(before[L.out_buf], after_out, n, L.out_pad, [(G.out_coff, G.cin) for G in group], what)
            x = _interior(before[L.in_buf][:n], L.in_pad)[..., L.in_coff:L.in_coff + L.cin]
            for G in group:
                x = maxpool5(x) if G.kind == 4 else upsample2(x)
                if not torch.equal(_interior(after_out[:n], G.out_pad)[..., G.out_coff:G.out_coff + G.cin], x):
                    raise LayerFault(f"{what}: row {layers.index(G)} is not the exact {'max-pool' if G.kind == 4 else 'copy'} of its input")
        elif L.kind == 6:
            hw = L.in_h * L.in_w
            v = _interior(before[L.in_buf][:n], L.in_pad)[..., L.in_coff:L.in_coff + 3 * no].cpu().numpy()
            ref, s = ref_decode(v, L.aux[0], list(L.aux[1:7]))
            bar = decode_bar(ref, s, _v_rows(v), L.aux[0], list(L.aux[1:7]))
            got = tr.pred[:, row0:row0 + 3 * hw].cpu().numpy().astype(np.float64)
            r = float((np.abs(got - ref) / bar).max())
            if not r <= 1.0:
                raise LayerFault(f"{what}: worst |err| / decode bar = {r:.3g}")
            dec_worst = max(dec_worst, r)
            per_row[k] = r
            row0 += 3 * hw
        tr.drop_before(e)
        k = e + 1
    forms = det.layer_forms()
    assert "not_run" not in forms, forms
    return {"forms": forms, "ratios": ratios, "decode": dec_worst, "rows": per_row}
