"""A float64 forward of any YOLOv5 v6.0 / v7.0 P5 model (n / s / m / l / x or custom multiples) for the tests of the whole
detection network: ``oracle/yolov5.py``'s graph with the bottlenecks per C3 block read from the state dict instead of
yolov5s's fixed 1, 2, 3, 1 / 1 (``playaid_core_amd.yolov5.graph_of``), in float64 on the CPU."""
from __future__ import annotations

import numpy as np
import torch
import torch.nn.functional as F

from oracle import yolov5 as oy

STRIDES = (8.0, 16.0, 32.0)


def f64_state_dict(sd):
    return {k: torch.from_numpy(np.asarray(v, np.float64)) for k, v in sd.items()}


def forward(x, sd, nc):
    """x [n, 3, H, W] (letter-boxed RGB, 0..1) -> pred float64 [n, rows, 5 + nc]; sd: arrays or tensors (cast to float64)."""
    from playaid_core_amd.yolov5 import graph_of

    rep = graph_of(sd)["repeats"]
    sd = f64_state_dict(sd)
    x = torch.as_tensor(np.asarray(x, np.float64))
    with torch.no_grad():
        y = F.conv2d(x, sd["model.0.conv.weight"], None, 2, 2)
        y = F.batch_norm(y, sd["model.0.bn.running_mean"], sd["model.0.bn.running_var"], sd["model.0.bn.weight"], sd["model.0.bn.bias"],
                         False, 0.0, oy.BN_EPS)
        x0 = F.silu(y)
        x1 = oy.conv(x0, sd, "model.1", 3, 2)
        x2 = oy.c3(x1, sd, "model.2", rep[2], True)
        x3 = oy.conv(x2, sd, "model.3", 3, 2)
        x4 = oy.c3(x3, sd, "model.4", rep[4], True)
        x5 = oy.conv(x4, sd, "model.5", 3, 2)
        x6 = oy.c3(x5, sd, "model.6", rep[6], True)
        x7 = oy.conv(x6, sd, "model.7", 3, 2)
        x8 = oy.c3(x7, sd, "model.8", rep[8], True)
        x9 = oy.sppf(x8, sd, "model.9")
        x10 = oy.conv(x9, sd, "model.10", 1)
        x13 = oy.c3(torch.cat([F.interpolate(x10, scale_factor=2, mode="nearest"), x6], 1), sd, "model.13", rep[13], False)
        x14 = oy.conv(x13, sd, "model.14", 1)
        x17 = oy.c3(torch.cat([F.interpolate(x14, scale_factor=2, mode="nearest"), x4], 1), sd, "model.17", rep[17], False)
        x18 = oy.conv(x17, sd, "model.18", 3, 2)
        x20 = oy.c3(torch.cat([x18, x14], 1), sd, "model.20", rep[20], False)
        x21 = oy.conv(x20, sd, "model.21", 3, 2)
        x23 = oy.c3(torch.cat([x21, x10], 1), sd, "model.23", rep[23], False)
        no, z = 5 + nc, []
        anchors = sd["model.24.anchors"]
        for i, f in enumerate((x17, x20, x23)):
            t = F.conv2d(f, sd[f"model.24.m.{i}.weight"], sd[f"model.24.m.{i}.bias"])
            bs, _, ny, nx = t.shape
            t = t.view(bs, 3, no, ny, nx).permute(0, 1, 3, 4, 2).contiguous()
            yv, xv = torch.meshgrid(torch.arange(ny, dtype=torch.float64), torch.arange(nx, dtype=torch.float64), indexing="ij")
            grid = torch.stack((xv, yv), 2).expand(1, 3, ny, nx, 2) - 0.5
            anchor_grid = (anchors[i] * STRIDES[i]).view(1, 3, 1, 1, 2).expand(1, 3, ny, nx, 2)
            xy, wh, conf = t.sigmoid().split((2, 2, nc + 1), 4)
            xy = (xy * 2 + grid) * STRIDES[i]
            wh = (wh * 2) ** 2 * anchor_grid
            z.append(torch.cat((xy, wh, conf), 4).view(bs, 3 * ny * nx, no))
        return torch.cat(z, 1).numpy()
