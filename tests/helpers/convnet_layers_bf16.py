"""The ResNet-50 table (``build_resnet50_table`` on ``pa_convnet_*``) under ``compute_dtype="bf16"``: float64 references of every
row from the STORED operands, the per-row device walk behind tests/test_convnet_bf16.py (and its knob child,
tests/helpers/convnet_bf16_knob_worker.py), and a CPU interpreter of the whole table that rounds where the device rounds.

Rounding model (include/playaid_hip.h, next to pa_convnet_create_dtype): the input image RNE to bf16; the stem's and every
convolution's folded fp32 weights RNE to bf16; products and sums in fp32 (float64 here), + fp32 bias, + the stored bf16
residual BEFORE the ReLU, ReLU (the stem then max-pools), ONE RNE to bf16 on the store; the average pool sums the stored bf16
values, fp32 out.

Bars (the bf16 detector's, tests/helpers/detector_layers_bf16.py):
  * input: bitwise RNE_bf16 of the image, border and channel 3 zero;
  * stem and convolutions: on every element ``|got - ref| <= half_ulp_bf16(ref) + 2e-5 * max|ref|``, and ``got == RNE(ref)``
    on at least 0.999 of them;
  * pool: fp32 against the float64 mean of the stored bf16 values, within ``1e-6 * max|ref|``;
  * every row: a bordered output keeps its border zero, and the part of the output buffer past the n crops it ran for is bit for
    bit what it held before.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from helpers.detector_layers_bf16 import MATCH_MIN, LayerFault, bf16_ratio, half_ulp_bf16, rne_bf16, trunc_bf16  # noqa: F401
from test_backbone_layers import border_is_zero, sample_crops

POOL_BAR = 1e-6
CONV_FORMS = {"bgemm", "bgemm_splitk"}
FAULTS = ("truncated_weights", "residual_after_relu", "no_store_rounding", "bias_dropped", "pool_rounded_to_bf16")


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def out_geom(d):
    if d["kind"] == 1:
        return 32, 1, 64
    if d["kind"] == 2:
        return 1, 0, d["cin"]
    return d["in_hw"] // d["stride"], d["out_pad"], d["cout"]


def _interior(a, pad):
    return a if pad == 0 else a[:, pad:-pad, pad:-pad, :]


def row_weights(d, blob, fault=None):
    """(w [cout][cin][k][k], b [cout]) float64 with the rounding model's weights (RNE bf16; "truncated_weights": truncated)."""
    blob = np.asarray(blob)
    if d["kind"] == 1:
        w = blob[d["w_off"]:d["w_off"] + 64 * 224].astype(np.float64).reshape(64, 7, 8, 4)[:, :, :7, :3].transpose(0, 3, 1, 2)
        b = blob[d["b_off"]:d["b_off"] + 64].astype(np.float64)
    else:
        k = d["ksize"]
        w = blob[d["w_off"]:d["w_off"] + d["cout"] * k * k * d["cin"]].astype(np.float64).reshape(d["cout"], k, k, d["cin"]).transpose(0, 3, 1, 2)
        b = blob[d["b_off"]:d["b_off"] + d["cout"]].astype(np.float64)
    w = trunc_bf16(w) if fault == "truncated_weights" else rne_bf16(w)
    return w, (np.zeros_like(b) if fault == "bias_dropped" else b)


def ref_stem(x, d, blob, fault=None):
    """x float64 [n][128][128][3] stored (bf16) pixels -> the pooled stem map [n][32][32][64], before the store's rounding."""
    w, b = row_weights(d, blob, fault)
    y = F.relu(F.conv2d(_t(x).permute(0, 3, 1, 2), _t(w), _t(b), stride=2, padding=3))
    return F.max_pool2d(y, 3, 2, 1).permute(0, 2, 3, 1).numpy()


def ref_conv(x, res, d, blob, fault=None):
    """x float64 [n][hw][hw][cin] stored input interior, res the stored residual interior or None -> the row's value before
    the store's rounding."""
    w, b = row_weights(d, blob, fault)
    y = F.conv2d(_t(x).permute(0, 3, 1, 2), _t(w), _t(b), stride=d["stride"], padding=d["ksize"] // 2).permute(0, 2, 3, 1).numpy()
    if res is not None and fault != "residual_after_relu":
        y = y + res
    if d["relu"]:
        y = np.maximum(y, 0.0)
    if res is not None and fault == "residual_after_relu":
        y = y + res
    return y


def store(y, fault=None):
    return y if fault == "no_store_rounding" else rne_bf16(y)


def pool_ratio(got, a):
    """got [n][C] fp32 pooled vector, a [n][hw][hw][C] the stored bf16 interior -> worst |got - mean| / (1e-6 max|mean|)."""
    ref = a.mean(axis=(1, 2))
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / (POOL_BAR * np.abs(ref).max()))


# -- the table as a float64 interpreter with RNE at each bf16 store (CPU) ---------------------------------------------
def run_row(d, blob, bufs, x, fault=None):
    """One row on float64 buffers (buffer -> [n][h][w][c] with its border) holding stored values, in place. x: the stored input
    interior [n][128][128][3]. fault (CPU tests): one of FAULTS."""
    ohw, opad, oc = out_geom(d)
    if d["kind"] == 1:
        y = store(ref_stem(x, d, blob, fault), fault)
    elif d["kind"] == 2:
        a = _interior(bufs[d["in_buf"]], d["in_pad"])
        y = a.mean(axis=(1, 2)).astype(np.float32).astype(np.float64)[:, None, None, :]
        if fault == "pool_rounded_to_bf16":
            y = rne_bf16(y)
    else:
        a = _interior(bufs[d["in_buf"]], d["in_pad"])
        res = _interior(bufs[d["res_buf"]], opad) if d["res_buf"] >= 0 else None
        y = store(ref_conv(a, res, d, blob, fault), fault)
    out = np.zeros((y.shape[0], ohw + 2 * opad, ohw + 2 * opad, oc))
    out[:, opad:opad + ohw, opad:opad + ohw, :] = y
    bufs[d["out_buf"]] = out


def interpret(descs, blob, x, keep=(), fault=None, fault_row=None):
    """The table under the rounding model in float64: x float32 [n][3][128][128] -> (features float64 [n][C], {row: the
    buffers as they were BEFORE that row} for the rows in keep, the buffers after the last row). fault applies to fault_row."""
    xs = rne_bf16(np.asarray(x, np.float64)).transpose(0, 2, 3, 1)
    bufs, before = {}, {}
    for li, d in enumerate(descs):
        if li in keep:
            before[li] = {b: a.copy() for b, a in bufs.items()}
        run_row(d, blob, bufs, xs, fault if li == fault_row else None)
    return bufs[descs[-1]["out_buf"]].reshape(x.shape[0], -1), before, bufs


def check_row(d, blob, before, got, x):
    """A row's output got (its buffer's interior for a stem / convolution, [n][C] for the pool) against float64 from the stored
    operands in before (buffer -> float64 array with border). -> (ratio, fraction equal to RNE(ref)); raises LayerFault."""
    ohw, opad, oc = out_geom(d)
    what = f"row {d.get('_row', '?')} (kind {d['kind']})"
    if d["kind"] == 2:
        r = pool_ratio(got, _interior(before[d["in_buf"]], d["in_pad"]))
        if not r <= 1.0:
            raise LayerFault(f"{what}: pool |err| = {r:.3g} x the bar (1e-6 max|ref|)")
        return r, 1.0
    if d["kind"] == 1:
        ref = ref_stem(x, d, blob)
    else:
        res = _interior(before[d["res_buf"]], opad) if d["res_buf"] >= 0 else None
        ref = ref_conv(_interior(before[d["in_buf"]], d["in_pad"]), res, d, blob)
    return bf16_ratio(got, ref, what)


# -- the device walk ----------------------------------------------------------------------------------------------------
def _crops(flat, n_max, hw, pad, c, idx):
    """device buffer -> host float64 [len(idx)][hw + 2 pad][hw + 2 pad][c] of the crops idx, as stored."""
    w = hw + 2 * pad
    return flat[:n_max * w * w * c].view(n_max, w, w, c)[torch.as_tensor(idx, device=flat.device)].double().cpu().numpy()


def check_table(net, descs, weights, n, seed, tag, log=print):
    """Traces every row of a bf16 ConvNet for n crops and checks it against float64 from the stored operands.
    -> {"forms": [...], "ratios": {form: worst}, "match": {form: lowest RNE fraction}}; raises LayerFault / AssertionError."""
    assert net.compute_dtype == "bf16", net.compute_dtype
    mc = net.max_crops
    rng = np.random.default_rng([seed, n])
    x = (rng.integers(0, 256, (n, 3, 128, 128)).astype(np.float32) / np.float32(255))
    xd = torch.from_numpy(x).cuda()
    idx = sample_crops(n)
    state = {b: torch.zeros(mc * f, dtype=net.buf_dtype[b], device="cuda") for b, f in enumerate(net.buf_floats)}   # buffers start zeroed
    x0 = net.trace(xd, -1, -1)
    assert x0.dtype == torch.bfloat16, f"{tag} input stored as {x0.dtype}"
    x0v = x0.view(mc, 134, 134, 4)
    want = rne_bf16(x.transpose(0, 2, 3, 1))
    assert np.array_equal(x0v[:n, 3:-3, 3:-3, :3].double().cpu().numpy(), want), f"{tag} input: not RNE_bf16 of the image"
    assert border_is_zero(x0v[:n].double().cpu().numpy(), 3) and not bool(x0v[:n, ..., 3].any()), f"{tag} input: border / channel 3"
    xs = want[idx]
    ratios, match, rows = {}, {}, []
    for li, d in enumerate(descs):
        out = net.trace(xd, li, d["out_buf"])
        torch.cuda.synchronize()
        form = net.layer_forms()[li]
        ohw, opad, oc = out_geom(d)
        ow = ohw + 2 * opad
        want_dt = torch.float32 if d["kind"] == 2 else torch.bfloat16
        assert out.dtype == want_dt, f"{tag} row {li} ({form}): stored as {out.dtype}"
        tail = n * ow * ow * oc
        assert torch.equal(out[tail:], state[d["out_buf"]][tail:]), f"{tag} row {li} ({form}): wrote past crop {n}"
        got = _crops(out, n, ohw, opad, oc, idx)
        if opad:
            assert border_is_zero(_crops(out, n, ohw, opad, oc, np.arange(n)), opad), f"{tag} row {li} ({form}): non-zero border"
        before = {}
        for key in ("in_buf", "res_buf"):
            b = d[key]
            if b >= 0 and d["kind"] != 1 and (key == "in_buf" or d["kind"] == 0):
                hw, pad, c = (d["in_hw"], d["in_pad"], d["cin"]) if key == "in_buf" else (ohw, opad, oc)
                before[b] = _crops(state[b], n, hw, pad, c, idx)
        dd = dict(d, _row=f"{li} [{tag}, {form}]")
        g = got.reshape(len(idx), -1) if d["kind"] == 2 else _interior(got, opad)
        r, m = check_row(dd, weights, before, g, xs)
        ratios[form] = max(ratios.get(form, 0.0), r)
        match[form] = min(match.get(form, 1.0), m)
        rows.append(form)
        state[d["out_buf"]] = out
    assert net.layer_forms() == rows, tag
    log(f"{tag}: " + ", ".join(f"{k} {v:.3f} (RNE {match[k]:.5f})" for k, v in sorted(ratios.items())))
    return {"forms": rows, "ratios": ratios, "match": match}
