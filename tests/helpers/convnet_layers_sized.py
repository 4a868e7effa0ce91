"""``tests/helpers/convnet_layers.check_table`` for a ResNet-50 table of any input size (``build_resnet50_table(crop_size=...)``:
a kind-3 stem row, maps of crop_size / 4, / 8, / 16, / 32 pixels): every row traced one at a time and rebuilt in float64 from
the STORED buffers of the rows it reads, with the folded fp32 weights of the table's own blob.

Bars, unchanged from that helper: every convolution and the stem + max-pool ``max|got - ref| <= 2e-5 * max|ref|``; the
average pool at the fp32 rounding of its hw^2-term mean; every bordered output's border exactly zero; the part of an output
buffer past the n crops bit for bit what it held before the row ran; the input conversion exact.

``expected_forms`` restates, from the launchers' own preconditions, which kernel form each row takes:
the test compares every row with it.
"""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from test_backbone_layers import U32, border_is_zero, f32_ratio, sample_crops


def in_size(descs):
    return int(descs[0]["in_hw"])


def _geom(d, which):
    if which == "in":
        return d["in_hw"], d["in_pad"], d["cin"]
    if d["kind"] in (1, 3):
        return d["in_hw"] // 4, 1, 64
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


def expected_forms(descs, n, max_crops, dtype):
    """The form each row of an fp32 table takes at n crops on a handle created for max_crops, from the stated preconditions:

    * kind 3 -> ``stem_pool_any``, kind 1 -> ``stem_pool``, kind 2 -> ``avgpool``;
    * a stride-1 3x3 row on a map of 8 pixels or more whose side is a multiple of 4 -> ``wino`` (wino.hip: sides % 4 == 0,
      cin % 8 == 0, cout % 32 == 0; the table's rule keeps maps below 8 off it);
    * ``emulated_f32`` only, rows that are not Winograd rows: ``psgemm`` where ceil(max_crops * out_hw^2 / 128) pixel tiles x
      cout / bn channel tiles (bn = 128 | 64, psgemm_pick_bn) are at least 128, half the chip (psgemm.hip takes any map with
      fewer than 65536 pixels);
    * a stride-1 3x3 row left over on a map 4, 8, 16 or 32 pixels wide -> ``patch`` where 64 (or, with 128-pixel tiles, 128)
      pixels are whole images or whole rows of one and the patch fits its LDS buffer (patchconv.hip);
    * everything else -> the implicit GEMM, tile by ``im2col_tile``: 128 x 128 where cout % 128 == 0 and there are 512 such
      tiles, 128 x 64 where there are 512 of those, else 64 x 64."""
    out = []
    for d in descs:
        if d["kind"] != 0:
            out.append({1: "stem_pool", 2: "avgpool", 3: "stem_pool_any"}[d["kind"]])
            continue
        k, s, hw, cin, cout = d["ksize"], d["stride"], d["in_hw"], d["cin"], d["cout"]
        ohw = hw // s
        wino = k == 3 and s == 1 and d["in_pad"] == 1 and hw >= 8 and hw % 4 == 0 and cin % 8 == 0
        if wino:
            out.append("wino")
            continue
        if dtype == "emulated_f32":
            bn = 128 if cout % 128 == 0 else 64
            if -(-max_crops * ohw * ohw // 128) * (cout // bn) >= 128:
                out.append("psgemm")
                continue
        m = n * ohw * ohw
        t128 = -(-m // 128) * (cout // 64)
        tile = "128x128" if cout % 128 == 0 and t128 // 2 >= 512 else ("128x64" if t128 >= 512 else "64x64")
        if k == 3 and s == 1 and d["in_pad"] == 1 and hw in (4, 8, 16, 32):
            bm = 64 if tile == "64x64" else 128
            howo = ohw * ohw
            if howo >= bm:
                fits = howo % bm == 0 and bm % ohw == 0
                patch_px = (bm // ohw + 2) * (ohw + 2) if fits else 0
            else:
                fits = bm % howo == 0
                patch_px = (bm // howo) * (ohw + 2) * (ohw + 2) if fits else 0
            if fits and (patch_px + 31) // 32 * 32 <= (160 if bm == 64 else 224):
                out.append("patch")
                continue
        out.append("igemm_" + tile)
    return out


def check_table(net, descs, weights, n, seed, tag, log=print):
    """Traces every row of `net` (a fresh ConvNet) for n crops and checks it. -> {"forms": [...], "ratios": {form: worst}}."""
    mc = net.max_crops
    size = in_size(descs)
    assert net.in_hw == size, tag
    rng = np.random.default_rng([seed, n, size])
    x = (rng.integers(0, 256, (n, 3, size, size)).astype(np.float32) / np.float32(255))
    xd = torch.from_numpy(x).cuda()
    idx = sample_crops(n)
    wts = weights.astype(np.float64)
    state = {b: torch.zeros(mc * f, dtype=torch.float32, device="cuda") for b, f in enumerate(net.buf_floats)}   # buffers start zeroed
    x0 = net.trace(xd, -1, -1).view(mc, size + 6, size + 6, 4)
    assert torch.equal(x0[:n, 3:-3, 3:-3, :3].cpu(), torch.from_numpy(x).permute(0, 2, 3, 1)), f"{tag}: the input conversion is not exact"
    assert not x0[:n, 3:-3, 3:-3, 3].any() and border_is_zero(x0[:n].cpu().numpy(), 3) and not x0[n:].any(), f"{tag}: input border / tail"
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
        if d["kind"] in (1, 3):
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
    return {"forms": rows, "ratios": ratios, "x": xd}
