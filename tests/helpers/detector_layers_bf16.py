"""Float64 references for the detector's layer table under ``compute_dtype="bf16"``, and the per-row checker behind
tests/test_detector_bf16.py (imported there and by its knob child, tests/helpers/detector_bf16_knob_worker.py). The bf16
counterpart of tests/helpers/detector_layers.py, whose public functions it reuses.

Every row's reference is built in float64 from the buffers as the device stored them after the row before, with the
rounding model's operands (include/playaid_hip.h, PA_DTYPE_BF16): the weights of a convolution rounded to nearest even (RNE)
bf16 from the table's fp32 blob, the stem's W / 255 in fp32 on the pixel integers, inputs and residuals as stored (bf16).

Bars (each row, per case; mirroring the backbone's bf16 check in tests/test_backbone_layers.py):
  * model input: the letterbox's pixel integers as bf16, bitwise; border and channel 3 zero.
  * bf16-stored convolutions (the stem and every convolution but the Detect heads): on every element
    ``|got - ref| <= half_ulp_bf16(ref) + 2e-5 * max|ref|``, and ``got == RNE_bf16(ref)`` on at least 0.999 of them.
  * fp32 Detect heads: the 2e-5 conv bar, the padding channels exactly 0.
  * max-pools and up-samplings, fused or not: bitwise the max / copy of the stored input.
  * decode: ``detector_layers.decode_bar`` on the stored fp32 head.
  * every row: a written buffer keeps its border zero; channels outside the written slices and images [n, max_images) are
    bitwise what they were before the row.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from helpers import detector_layers as dl
from helpers.detector_layers import LayerFault, decode_bar, geometry, maxpool5, ref_decode, row_weights, upsample2  # noqa: F401

CONV_BAR = dl.CONV_BAR
MATCH_MIN = 0.999   # fraction of elements that must equal RNE_bf16(ref)


# -- bf16 roundings (on float64 arrays; the values stay float64) --------------------------------------------------
def rne_bf16(x):
    """Round to nearest even bf16 (through fp32: the operands here are fp32 or closer to a bf16 than fp32 resolves)."""
    u = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32)).view(np.uint32).astype(np.uint64)
    u = (u + 0x7FFF + ((u >> 16) & 1)) & 0xFFFF0000
    return u.astype(np.uint32).view(np.float32).astype(np.float64)


def trunc_bf16(x):
    u = np.ascontiguousarray(np.asarray(x, np.float64).astype(np.float32)).view(np.uint32) & np.uint32(0xFFFF0000)
    return u.view(np.float32).astype(np.float64)


def half_ulp_bf16(x):
    """Half the bf16 spacing at |x| (8 significant bits): 2^(floor(log2|x|) - 8); 0 at 0."""
    m, e = np.frexp(np.abs(np.asarray(x, np.float64)))   # |x| = m 2^e, m in [0.5, 1)
    return np.where(m == 0, 0.0, np.ldexp(1.0, e - 9))


def bf16_weights(L, blob, fault=None):
    """(w, b) float64 of a row with the rounding model's weights: a convolution's folded fp32 weights RNE-rounded to bf16; the
    stem's fp32 W / 255 (applied to the pixel integers). fault: "unrounded_weights" keeps the fp32 weights,
    "stem_scaled_after_rounding" takes RNE_bf16(W) / 255 for the stem."""
    w, b = row_weights(L, blob)
    if L.kind == 3:
        if fault == "stem_scaled_after_rounding":
            return rne_bf16(w) / 255.0, b
        return (w / 255.0).astype(np.float32).astype(np.float64), b
    if fault == "unrounded_weights":
        return w, b
    return rne_bf16(w), b


def ref_stem_int(x_int, w, b):
    """x_int [n][H][W][3] float64 pixel integers, w = W / 255 -> SiLU(conv 6x6 / 2, padding 2) (unrounded)."""
    return dl.ref_stem(x_int, w, b)


# -- the table as a float64 interpreter with the bf16 stores (CPU) --------------------------------------------------
def head_buffers(layers):
    return {L.in_buf for L in layers if L.kind == 6}


def run_row(L, blob, bufs, x_int, heads, fault=None):
    """One row of the rounding model on float64 buffers holding stored values (bf16 ones, fp32 ones for the heads), in place.
    fault (CPU tests): "unrounded_weights", "truncate_store", "fp32_store", "residual_rounded_before_add",
    "stem_scaled_after_rounding"."""
    def get(b, coff, c, pad):
        a = bufs[b]
        return a[:, pad:a.shape[1] - pad, pad:a.shape[2] - pad, coff:coff + c]

    def put(b, coff, pad, y):
        a = bufs[b]
        a[:, pad:a.shape[1] - pad, pad:a.shape[2] - pad, coff:coff + y.shape[-1]] = y

    def store(y, fp32=False):
        if fp32:
            return y.astype(np.float32).astype(np.float64)
        if fault == "fp32_store":
            return y.astype(np.float32).astype(np.float64)
        if fault == "truncate_store":
            return trunc_bf16(y)
        return rne_bf16(y)

    if L.kind == 3:
        w, b = bf16_weights(L, blob, fault)
        put(L.out_buf, L.out_coff, L.out_pad, store(ref_stem_int(x_int, w, b)))
    elif L.kind == 0:
        w, b = bf16_weights(L, blob, fault)
        x = get(L.in_buf, L.in_coff, L.cin, L.in_pad)
        if L.res_buf >= 0:
            res = get(L.res_buf, L.res_coff, L.cout, L.out_pad).copy()
            y = dl.ref_conv(x, w, b, L.stride, L.act, None)
            if fault == "residual_rounded_before_add":
                y = rne_bf16(y)
            y = y + res if L.res_after else dl.activation(dl.ref_conv(x, w, b, L.stride, 0, None) + res, L.act)
        else:
            y = dl.ref_conv(x, w, b, L.stride, L.act, None)
        put(L.out_buf, L.out_coff, L.out_pad, store(y, fp32=L.out_buf in heads))
    elif L.kind == 4:
        put(L.out_buf, L.out_coff, L.out_pad, maxpool5(get(L.in_buf, L.in_coff, L.cin, L.in_pad).copy()).numpy())
    elif L.kind == 5:
        put(L.out_buf, L.out_coff, L.out_pad, upsample2(torch.from_numpy(get(L.in_buf, L.in_coff, L.cin, L.in_pad).copy())).numpy())


def interpret(layers, blob, x_int, nc, fault=None, states=False):
    """The table under the rounding model in float64 with RNE at each bf16 store: x_int float64 [n][3][H][W] pixel integers
    (letter-boxed) -> pred [n][rows][5 + nc]; states=True: also the buffers after every row (list of dicts)."""
    geo = geometry(layers)
    n = x_int.shape[0]
    heads = head_buffers(layers)
    bufs = {b: np.zeros((n, h + 2 * p, w + 2 * p, c)) for b, (h, w, p, c) in geo.items()}
    x_nhwc = np.ascontiguousarray(np.asarray(x_int, np.float64).transpose(0, 2, 3, 1))
    rows, after = [], []
    for L in layers:
        if L.kind == 6:
            a = bufs[L.in_buf]
            v = a[:, L.in_pad:a.shape[1] - L.in_pad, L.in_pad:a.shape[2] - L.in_pad, L.in_coff:L.in_coff + 3 * (5 + nc)]
            rows.append(ref_decode(v, L.aux[0], list(L.aux[1:7]))[0])
        else:
            run_row(L, blob, bufs, x_nhwc, heads, fault)
        if states:
            after.append({b: a.copy() for b, a in bufs.items()})
    pred = np.concatenate(rows, axis=1)
    return (pred, after) if states else pred


# -- the per-row comparison ----------------------------------------------------------------------------------------
def bf16_ratio(got, ref, what):
    """A bf16-stored convolution: -> worst |got - ref| / (half_ulp_bf16(ref) + 2e-5 max|ref|) and the fraction of elements
    equal to RNE_bf16(ref); raises LayerFault past either bar or when the reference is mostly zero (an idle check)."""
    ref = np.asarray(ref, np.float64)
    got = np.asarray(got, np.float64)
    if not (ref != 0).mean() > 0.2:
        raise LayerFault(f"{what}: the reference is mostly zero, the check would be idle")
    bar = half_ulp_bf16(ref) + CONV_BAR * np.abs(ref).max()
    ratio = float((np.abs(got - ref) / bar).max())
    match = float((got == rne_bf16(ref)).mean())
    if not ratio <= 1.0:
        raise LayerFault(f"{what}: max |err| = {ratio:.3g} x the bf16 bar (half ulp + 2e-5 max|ref|)")
    if not match >= MATCH_MIN:
        raise LayerFault(f"{what}: only {match:.5f} of the elements are RNE_bf16(ref) (bar {MATCH_MIN})")
    return ratio, match


def check_conv_row(L, blob, before, after_out, idx, what, head=False, no=None):
    """A convolution row (kind 0) against float64 from the stored operands. before: buffer -> host float64 array after the
    row before (the sampled images idx); after_out: its output buffer after the row, same images. head: an fp32 Detect head
    (the 2e-5 conv bar; channels 3 * no .. cout exactly 0). -> (ratio, fraction equal to RNE(ref)) (head: (ratio, 1.0))."""
    w, b = bf16_weights(L, blob)
    x = dl._interior(before[L.in_buf][idx], L.in_pad)[..., L.in_coff:L.in_coff + L.cin]
    res = None
    if L.res_buf >= 0:
        res = dl._interior(before[L.res_buf][idx], L.out_pad)[..., L.res_coff:L.res_coff + L.cout].astype(np.float64)
    ref = dl.ref_conv(x, w, b, L.stride, L.act, res, L.res_after)
    got = dl._interior(after_out[idx], L.out_pad)[..., L.out_coff:L.out_coff + L.cout]
    if head:
        c = L.cout
        if no is not None and 3 * no < c:
            c = 3 * no
            if np.any(got[..., c:]):
                raise LayerFault(f"{what}: the head's padding channels are not zero")
        return dl.conv_ratio(got[..., :c], ref[..., :c], what), 1.0
    return bf16_ratio(got, ref, what)


def check_stem_row(L, blob, x_int, got, what):
    w, b = bf16_weights(L, blob)
    return bf16_ratio(got, ref_stem_int(x_int, w, b), what)


# -- the device walk --------------------------------------------------------------------------------------------------
def check_detector(det, frames_np, tag, log=print):
    """Walks every row of a bf16 detector's table on frames uint8[n,H,W,3] and checks it; returns {"forms", "ratios" (form ->
    worst ratio), "match" (form -> lowest fraction equal to RNE), "decode", "rows"}. Raises LayerFault naming row, kind and form."""
    from oracle import yolov5 as oy

    assert det.compute_dtype == "bf16", det.compute_dtype
    n = frames_np.shape[0]
    frames = torch.from_numpy(np.ascontiguousarray(frames_np)).to(det.device)
    layers, blob, nc = det.layers, det.weights, det.nc
    no = 5 + nc
    heads = head_buffers(layers)
    idx = dl.sample_images(n)
    tr = dl._Trace(det, frames, n)
    host = lambda t, sel=idx: t[torch.as_tensor(sel, device=t.device)].double().cpu().numpy()
    x0, _ = tr.get(-1, -1)
    if x0.dtype != torch.bfloat16:
        raise LayerFault(f"{tag} input: stored as {x0.dtype}, not bf16")
    if bool(x0[..., 3].any()) or bool(x0[:, :2].any()) or bool(x0[:, -2:].any()) or bool(x0[:, :, :2].any()) or bool(x0[:, :, -2:].any()):
        raise LayerFault(f"{tag} input: border or channel 3 not zero")
    want = np.stack([oy.letterbox(frames_np[i], det.net_hw) for i in idx]).transpose(0, 2, 3, 1)
    x_int = host(x0)[:, 2:-2, 2:-2, :3]
    if not np.array_equal(x_int, np.rint(want.astype(np.float64) * 255)):
        raise LayerFault(f"{tag} input: not the letterbox's pixel integers")
    ratios, match, dec_worst, row0, per_row = {}, {}, 0.0, 0, {}
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
        form = det.layer_forms()[k]
        what = f"{tag} row {k} (kind {L.kind}, {form})"
        if L.kind in (0, 3):
            want_dt = torch.float32 if L.kind == 0 and L.out_buf in heads else torch.bfloat16
            if after_out.dtype != want_dt:
                raise LayerFault(f"{what}: output stored as {after_out.dtype}, not {want_dt}")
            dl.check_written(before[L.out_buf], after_out, n, L.out_pad, [(L.out_coff, L.cout)], what)
            if L.kind == 3:
                got = dl._interior(host(after_out), L.out_pad)[..., L.out_coff:L.out_coff + L.cout]
                r, m = check_stem_row(L, blob, x_int, got, what)
            else:
                bh = {b: host(t) for b, t in before.items()}
                r, m = check_conv_row(L, blob, bh, host(after_out), np.arange(len(idx)), what, head=L.out_buf in heads, no=no)
            ratios[form] = max(ratios.get(form, 0.0), r)
            match[form] = min(match.get(form, 1.0), m)
            per_row[k] = (r, m)
            if e == k + 1:   # the next row's up-sampling, written by this launch
                U = layers[k + 1]
                ua, _ = tr.get(k, U.out_buf)
                dl.check_written(before[U.out_buf], ua, n, U.out_pad, [(U.out_coff, U.cin)], what + " fused up-sampling")
                src = dl._interior(after_out[:n], L.out_pad)[..., L.out_coff:L.out_coff + L.cout]
                if not torch.equal(dl._interior(ua[:n], U.out_pad)[..., U.out_coff:U.out_coff + U.cin], upsample2(src)):
                    raise LayerFault(f"{what}: the fused up-sampling is not a copy of the stored output")
        elif L.kind in (4, 5):
            group = layers[k:e + 1]
            if after_out.dtype != torch.bfloat16:
                raise LayerFault(f"{what}: output stored as {after_out.dtype}, not bf16")
            dl.check_written(before[L.out_buf], after_out, n, L.out_pad, [(G.out_coff, G.cin) for G in group], what)
            x = dl._interior(before[L.in_buf][:n], L.in_pad)[..., L.in_coff:L.in_coff + L.cin]
            for G in group:
                x = maxpool5(x) if G.kind == 4 else upsample2(x)
                if not torch.equal(dl._interior(after_out[:n], G.out_pad)[..., G.out_coff:G.out_coff + G.cin], x):
                    raise LayerFault(f"{what}: row {layers.index(G)} is not the exact {'max-pool' if G.kind == 4 else 'copy'} of its input")
        elif L.kind == 6:
            hw = L.in_h * L.in_w
            v = dl._interior(before[L.in_buf][:n], L.in_pad)[..., L.in_coff:L.in_coff + 3 * no].cpu().numpy()
            ref, s = ref_decode(v, L.aux[0], list(L.aux[1:7]))
            bar = decode_bar(ref, s, dl._v_rows(v), L.aux[0], list(L.aux[1:7]))
            got = tr.pred[:, row0:row0 + 3 * hw].cpu().numpy().astype(np.float64)
            r = float((np.abs(got - ref) / bar).max())
            if not r <= 1.0:
                raise LayerFault(f"{what}: worst |err| / decode bar = {r:.3g}")
            dec_worst = max(dec_worst, r)
            per_row[k] = (r, 1.0)
            row0 += 3 * hw
        tr.drop_before(e)
        k = e + 1
    forms = det.layer_forms()
    assert "not_run" not in forms, forms
    return {"forms": forms, "ratios": ratios, "match": match, "decode": dec_worst, "rows": per_row}
