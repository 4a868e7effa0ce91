"""Shared by tests/test_convnet_layers.py and its knob child (tests/helpers/convnet_knob_worker.py): every row of the
ResNet-50 table (``build_resnet50_table`` on ``pa_convnet_*``) traced one at a time and rebuilt in float64 from the STORED
buffers of the rows it reads (input, and residual where there is one) with the folded fp32 weights of the table's own blob,
so errors do not add up from row to row and a corrupted border shows up in the next row.

Bars (those of tests/test_backbone_layers.py for the same kernels): every convolution and the stem + max-pool
``max|got - ref| <= 2e-5 * max|ref|``; the average pool at the fp32 rounding of its hw^2-term mean; every bordered output's
border exactly zero; and the part of an output buffer past the n crops a row was run for (in that row's geometry) bit for
bit what it held before the row ran.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from test_backbone_layers import U32, border_is_zero, f32_ratio, sample_crops


def _geom(d, which):
    if which == "in":
        return d["in_hw"], d["in_pad"], d["cin"]
    if d["kind"] == 1:
        return 32, 1, 64
    if d["kind"] == 2:
        return 1, 0, d["cin"]
    return d["in_hw"] // d["stride"], d["out_pad"], d["cout"]


def _crops(flat, n_max, hw, pad, c, idx):
    """device buffer -> host float64 [len(idx)][hw + 2 pad][hw + 2 pad][c] of the crops idx (as stored)."""
    w = hw + 2 * pad
    return flat[:n_max * w * w * c].view(n_max, w, w, c)[torch.as_tensor(idx, device=flat.device)].double().cpu().numpy()


def _interior(a, pad):
    return a if pad == 0 else a[:, pad:-pad, pad:-pad, :]


def _t(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float64))


def check_table(net, descs, weights, n, seed, tag, log=print):
    """Traces every row of `net` (a fresh ConvNet) for n crops and checks it. -> {"forms": [...], "ratios": {form: worst}}."""
    mc = net.max_crops
    rng = np.random.default_rng([seed, n])
    x = (rng.integers(0, 256, (n, 3, 128, 128)).astype(np.float32) / np.float32(255))
    xd = torch.from_numpy(x).cuda()
    idx = sample_crops(n)
    wts = weights.astype(np.float64)
    state = {b: torch.zeros(mc * f, dtype=torch.float32, device="cuda") for b, f in enumerate(net.buf_floats)}   # buffers start zeroed
    x0 = net.trace(xd, -1, -1)
    assert torch.equal(x0.view(mc, 134, 134, 4)[:n, 3:-3, 3:-3, :3].cpu(), torch.from_numpy(x).permute(0, 2, 3, 1)), tag
    ratios = {}
    rows = []
    for li, d in enumerate(descs):
        out = net.trace(xd, li, d["out_buf"])
        torch.cuda.synchronize()
        form = net.layer_forms()[li]
        ohw, opad, oc = _geom(d, "out")
        ow = ohw + 2 * opad
        got = _crops(out, n, ohw, opad, oc, idx)
        if opad:
            assert border_is_zero(_crops(out, n, ohw, opad, oc, np.arange(n)), opad), f"{tag} row {li} ({form}): non-zero border"
        tail = n * ow * ow * oc
        assert torch.equal(out[tail:], state[d["out_buf"]][tail:]), f"{tag} row {li} ({form}): wrote past crop {n}"
        if d["kind"] == 1:
            st = wts[d["w_off"]:d["w_off"] + 64 * 7 * 8 * 4].reshape(64, 7, 8, 4)[:, :, :7, :3].transpose(0, 3, 1, 2)
            b = wts[d["b_off"]:d["b_off"] + 64]
            y = F.conv2d(_t(x[idx]), _t(st), _t(b), stride=2, padding=3)
            ref = F.max_pool2d(F.relu(y), 3, 2, 1).permute(0, 2, 3, 1).numpy()
            r = f32_ratio(_interior(got, 1), ref)
        elif d["kind"] == 2:
            ihw, ipad, ic = _geom(d, "in")
            a = _interior(_crops(state[d["in_buf"]], n, ihw, ipad, ic, idx), ipad)
            ref = a.mean(axis=(1, 2))
            bar = ihw * ihw * U32 * np.abs(a).mean(axis=(1, 2))
            r = float((np.abs(got.reshape(len(idx), -1) - ref) / np.maximum(bar, 1e-300)).max())
        else:
            ihw, ipad, ic = _geom(d, "in")
            k = d["ksize"]
            a = _interior(_crops(state[d["in_buf"]], n, ihw, ipad, ic, idx), ipad)
            wk = wts[d["w_off"]:d["w_off"] + d["cout"] * k * k * d["cin"]].reshape(d["cout"], k, k, d["cin"]).transpose(0, 3, 1, 2)
            b = wts[d["b_off"]:d["b_off"] + d["cout"]]
            y = F.conv2d(_t(a).permute(0, 3, 1, 2), _t(wk), _t(b), stride=d["stride"], padding=k // 2).permute(0, 2, 3, 1).numpy()
            if d["res_buf"] >= 0:
                y = y + _interior(_crops(state[d["res_buf"]], n, ohw, opad, oc, idx), opad)
            ref = np.maximum(y, 0.0) if d["relu"] else y
            r = f32_ratio(_interior(got, opad), ref)
        assert (ref != 0).mean() > 0.2, f"{tag} row {li}: the reference is mostly zero, the check would be idle"
        assert r <= 1.0, f"{tag} row {li} ({form}): max|err| = {r:.3g} x its bar"
        ratios[form] = max(ratios.get(form, 0.0), r)
        rows.append(form)
        state[d["out_buf"]] = out
    assert net.layer_forms() == rows, tag
    log(f"{tag}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(ratios.items())))
    return {"forms": rows, "ratios": ratios}
