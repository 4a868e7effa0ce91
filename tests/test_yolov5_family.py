"""Every YOLOv5 v6.0 / v7.0 P5 size (n / s / m / l / x, custom multiples) on the device detector, and NMS for up to 80 classes.

CPU: the tables ``build_yolov5_table`` wires (widths, repeats, padding to multiples of 32, parameter counts), the s table
byte for byte against ``build_yolov5s_table``, and the float64 forward of tests/helpers/yolov5_f64.py against the oracle.
GPU: every row of the n / m / l / x tables against float64 (tests/helpers/detector_layers*.py, the bars stated there), the
whole network against the float64 forward, and ``pa_detect_postprocess_classes`` against ``oracle.detect`` at nc = 80.
"""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import yolov5_f64  # noqa: E402

from playaid_core_amd import synth  # noqa: E402

SIZES = ["n", "s", "m", "l", "x"]
PUBLISHED = {"n": (16, 1), "s": (32, 1), "m": (48, 2), "l": (64, 3), "x": (80, 4)}   # c1, head repeats
PUBLISHED_MPARAMS = {"n": 1.9, "s": 7.2, "m": 21.2, "l": 46.5, "x": 86.7}   # ultralytics' table (BatchNorm folded), nc = 80
NET = (384, 640)


def _table(sd, nc, net=NET):
    from playaid_core_amd.yolov5 import build_yolov5_table

    masks = []
    out = build_yolov5_table(sd, net, nc, real_masks=masks)
    return out + (masks,)


def _row_weights(L, blob):
    if L.kind == 3:
        lane = blob[L.w_off:L.w_off + 64 * 56].reshape(2, 32, 56)
        return lane[..., :54].transpose(1, 0, 2).reshape(32, 1, 108), blob[L.b_off:L.b_off + 32]
    k = L.ksize
    return blob[L.w_off:L.w_off + L.cout * k * k * L.cin].reshape(L.cout, k * k, L.cin), blob[L.b_off:L.b_off + L.cout]


@pytest.mark.parametrize("size", SIZES + [(0.5, 0.375)])
def test_tables_of_every_size(size):
    from playaid_core_amd.yolov5 import P5_SIZES, graph_of, p5_graph

    nc = 80
    sd = synth.make_yolov5_state_dict(size, nc=nc)
    gd, gw = P5_SIZES[size] if isinstance(size, str) else size
    want = p5_graph(gd, gw)
    g = graph_of(sd)
    assert g["widths"] == want["widths"] and g["repeats"] == want["repeats"] and g["nc"] == nc
    if isinstance(size, str):
        c1, head = PUBLISHED[size]
        assert g["widths"] == tuple(c1 * m for m in (1, 2, 4, 8, 16))
        assert [g["repeats"][i] for i in (2, 4, 6, 8)] == [head, 2 * head, 3 * head, head]
        assert all(g["repeats"][i] == head for i in (13, 17, 20, 23))
    layers, bufs, blob, rows, masks = _table(sd, nc)
    assert rows == 3 * (48 * 80 + 24 * 40 + 12 * 20)
    kinds = [L.kind for L in layers]
    # model.1 / 3 / 5 / 7, SPPF's two, model.10 / 14 / 18 / 21, three Detect heads; per C3: [cv1 | cv2], cv3, two per bottleneck
    n_conv = 4 + 2 + 4 + 3 + sum(2 + 2 * n for n in g["repeats"].values())
    assert kinds.count(3) == -(-g["widths"][0] // 32) and kinds.count(0) == n_conv and kinds.count(6) == 3
    assert kinds.count(4) == 3 and kinds.count(5) == 2
    real_w = real_b = 0
    by_row = {i: (r, c) for i, r, c in masks}
    assert sorted(by_row) == [i for i, L in enumerate(layers) if L.kind in (0, 3)]
    for i, L in enumerate(layers):
        if L.kind == 0:
            assert L.cin % 32 == 0 and L.cout % 32 == 0 and L.in_coff % 32 == 0 and L.out_coff % 32 == 0, i
        if L.kind == 3:
            assert L.cout == 32 and L.out_coff % 32 == 0
        if L.kind not in (0, 3):
            continue
        w, b = _row_weights(L, blob)
        r, c = by_row[i]
        # every padded weight row, weight column and bias entry is exactly 0
        assert not np.any(w[~r]) and not np.any(b[~r]), i
        if L.kind == 0:
            assert not np.any(w[:, :, ~c]), i
            real_w += int(r.sum()) * L.ksize * L.ksize * int(c.sum())
        else:
            real_w += int(r.sum()) * 108
        real_b += int(r.sum())
    # the real parameters are the state dict's: conv weights, one folded bias per BatchNorm channel, the Detect convolutions
    sd_w = sum(v.size for k, v in sd.items() if k.endswith("conv.weight") or (k.startswith("model.24.m") and k.endswith("weight")))
    sd_b = sum(v.size for k, v in sd.items() if k.endswith("bn.bias") or (k.startswith("model.24.m") and k.endswith("bias")))
    assert (real_w, real_b) == (sd_w, sd_b)
    if isinstance(size, str):
        assert round((real_w + real_b) / 1e6, 1) == PUBLISHED_MPARAMS[size], (real_w + real_b) / 1e6
    # head slices: 3 (5 + nc) rounded up to 32
    assert all(L.cin == 256 for L in layers if L.kind == 6)


@pytest.mark.parametrize("nc", [1, 6, 16])
def test_generic_table_is_the_s_table_byte_for_byte(nc):
    from playaid_core_amd.yolov5 import build_yolov5_table, build_yolov5s_table

    sd = synth.make_yolov5s_state_dict(nc=nc)
    for net in ((384, 640), (64, 96)):
        a, b = build_yolov5s_table(sd, net, nc), build_yolov5_table(sd, net, nc)
        assert len(a[0]) == len(b[0]) and all(bytes(x) == bytes(y) for x, y in zip(a[0], b[0]))
        assert a[1] == b[1] and a[3] == b[3] and a[2].dtype == b[2].dtype and a[2].tobytes() == b[2].tobytes()
    assert all(np.array_equal(v, synth.make_yolov5_state_dict("s", nc=nc)[k]) for k, v in sd.items())


def test_builder_refuses_what_it_cannot_wire():
    from playaid_core_amd.yolov5 import build_yolov5_table

    sd = synth.make_yolov5_state_dict("n", nc=6)
    with pytest.raises(ValueError, match="6 classes"):
        build_yolov5_table(sd, (64, 96), 7)
    focus = dict(sd)
    focus["model.0.conv.conv.weight"] = focus.pop("model.0.conv.weight")
    with pytest.raises(ValueError, match="Focus"):
        build_yolov5_table(focus, (64, 96), 6)


@pytest.mark.parametrize("size", ["s", "n"])
def test_float64_forward_is_the_oracle(size):
    """For s and n (the oracle's hard-coded 1, 2, 3, 1 / 1 bottlenecks) the helper's forward is oracle.yolov5.forward."""
    import torch

    from oracle import yolov5 as oy

    sd = synth.make_yolov5_state_dict(size, nc=6)
    x = np.random.default_rng(3).random((2, 3, 64, 96))
    got = yolov5_f64.forward(x, sd, 6)
    want = oy.forward(torch.from_numpy(x), yolov5_f64.f64_state_dict(sd), 6).numpy()
    assert got.dtype == want.dtype == np.float64
    assert np.abs(got - want).max() <= 1e-12 * np.abs(want).max()


def test_float64_interpreter_of_every_size_is_the_graph():
    """The padded table, run row by row in float64 (tests/helpers/detector_layers.interpret), is the float64 graph."""
    from helpers import detector_layers as dl

    for size in ("n", "m", (0.5, 0.375)):
        sd = synth.make_yolov5_state_dict(size, nc=80)
        layers, _, blob, _, _ = _table(sd, 80, (64, 96))
        x = np.random.default_rng(5).random((1, 3, 64, 96))
        got = dl.interpret(layers, blob, x, 80)
        want = yolov5_f64.forward(x, {k: np.asarray(v, np.float32) for k, v in sd.items()}, 80)
        assert np.abs(got - want).max() <= 2e-5 * np.abs(want).max(), size


# ---- GPU ---------------------------------------------------------------------------------------------------------------
def _frames(n, h=720, w=1280, seed=11):
    return synth.make_frames(n, h, w, seed=seed)


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "emulated_f32", "bf16"])
@pytest.mark.parametrize("size", ["n", "m", "l", "x"])
def test_rows_of_every_size_against_float64(size, dtype):
    from helpers import detector_layers as dl
    from helpers import detector_layers_bf16 as dlb

    from playaid_core_amd.yolov5 import YoloV5Detector

    sd = synth.make_yolov5_state_dict(size, nc=80 if size == "x" else 6)
    nc = 80 if size == "x" else 6
    chk = dlb.check_detector if dtype == "bf16" else dl.check_detector
    for net, n, (fh, fw) in (((64, 96), 3, (270, 480)), ((128, 224), 2, (720, 1280))):
        det = YoloV5Detector(sd, nc, net, max_images=n, compute_dtype=dtype)
        try:
            res = chk(det, _frames(n, fh, fw), f"{size} {dtype} net {net}")
        finally:
            det.close()
        stems = [f for f, L in zip(res["forms"], det.layers) if L.kind == 3]
        assert stems == [("stem_direct" if dtype == "f32" else "stem_bf16")] * (-(-sd["model.0.conv.weight"].shape[0] // 32))
        print(f"{size} {dtype} {net}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(res["ratios"].items())) + f"; decode {res['decode']:.3f}")


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["f32", "emulated_f32"])
@pytest.mark.parametrize("size,net", [("n", (128, 224)), ("s", (128, 224)), ("m", (128, 224)), ("l", (128, 224)), ("x", (128, 224)),
                                      ("m", (384, 640)), ("x", (384, 640))])
def test_network_of_every_size_against_float64(size, net, dtype):
    import torch

    from oracle import yolov5 as oy
    from playaid_core_amd.yolov5 import YoloV5Detector

    nc = 80 if size in ("s", "x") else 6
    sd = synth.make_yolov5_state_dict(size, nc=nc)
    frames = _frames(2, 720, 1280, seed=7)
    det = YoloV5Detector(sd, nc, net, max_images=2, compute_dtype=dtype)
    try:
        got = det(frames)
        torch.cuda.synchronize()
        got = got.cpu().numpy().astype(np.float64)
    finally:
        det.close()
    x = np.stack([oy.letterbox(f, net) for f in frames]).astype(np.float64)
    want = yolov5_f64.forward(x, sd, nc)
    e_box, e_score = np.abs(got[..., :4] - want[..., :4]).max(), np.abs(got[..., 4:] - want[..., 4:]).max()
    print(f"{size} {dtype} {net}: boxes {e_box:.2e} px, scores {e_score:.2e}")
    assert e_box <= 1e-4 * min(net) and e_score <= 1e-4


@pytest.fixture(scope="module")
def nms_engine():
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from playaid_core_amd.engine import Engine

    eng = Engine(synth.make_state_dict(seed=1234), max_batch_frames=8, max_clip_frames=64)
    yield eng
    eng.close()


@pytest.mark.gpu
def test_nms_at_80_classes_against_the_oracle(nms_engine):
    """Rows of a live nc = 80 network with crafted candidates written over the first rows (tests/test_chain.py's way: the seeded
    network itself stays far below the gate), classes None / (2, 3) / (0,) / (79,) / (33, 64): label text byte for byte."""
    import torch

    from oracle import detect as odet
    from playaid_core_amd import detect as pdet
    from playaid_core_amd.yolov5 import YoloV5Detector

    nc, net, (h, w), n = 80, (384, 640), (720, 1280), 4
    det = YoloV5Detector(synth.make_yolov5_state_dict("s", nc=nc), nc, net, max_images=n)
    try:
        pred = det(_frames(n, h, w, seed=21))
        torch.cuda.synchronize()
    finally:
        det.close()
    CONF = 0.7   # (the seeded network's best row over all 80 classes reaches ~0.61)
    want = pred.cpu().numpy()
    assert (want[..., 4:5] * want[..., 5:]).max() < CONF - 0.05
    rng = np.random.default_rng(4)
    cand = np.zeros((n, 12, 5 + nc), np.float32)
    for i in range(n):
        for k in range(12):   # four groups of near-duplicates; classes across all three mask words, some shared
            cls = (0, 2, 3, 33, 64, 79)[(k + i) % 6] if k % 3 else (2, 79, 33, 0)[k // 3]
            cx, cy = 100 + 120 * (k // 3) + 3 * (k % 3), 150 + 20 * i - 2 * (k % 3)
            cand[i, k, :5] = [cx, cy, 80 + rng.integers(0, 20), 60 + rng.integers(0, 20), 0.97 - 0.04 * k]
            cand[i, k, 5 + cls] = 0.9 - 0.01 * (k % 3)
            cand[i, k, 5 + (cls + 1) % nc] = 0.3
    cand[1, 3:6, 4] = 0.0   # a group lost in one frame
    pred[:, :12] = torch.from_numpy(cand).cuda()
    want[:, :12] = cand
    for classes in (None, (2, 3), (0,), (79,), (33, 64)):
        for max_det in (2, 8):
            dets, counts = nms_engine.detect_postprocess(pred, net, (h, w), conf_thres=CONF, classes=classes, max_det=max_det)
            torch.cuda.synchronize()
            d, c = dets.cpu().numpy(), counts.cpu().numpy()
            dev = [pdet.label_lines(d[i, : c[i]]) for i in range(n)]
            orc = [odet.detect_frame(want[i], net, (h, w), conf_thres=CONF, classes=range(nc) if classes is None else classes,
                                     max_det=max_det)[1] for i in range(n)]
            assert dev == orc, (classes, max_det)
            assert sum(t.count("\n") for t in orc) > 0, classes
    # a gate so low that every row of the frame is a candidate: more than the 4096 the compact list holds
    dets, counts = nms_engine.detect_postprocess(pred, net, (h, w), conf_thres=1e-9, classes=None, max_det=8)
    torch.cuda.synchronize()
    d, c = dets.cpu().numpy(), counts.cpu().numpy()
    assert int(((want[0, :, 4:5] * want[0, :, 5:]).max(1) > 1e-9).sum()) > 4096
    for i in range(n):
        assert pdet.label_lines(d[i, : c[i]]) == odet.detect_frame(want[i], net, (h, w), conf_thres=1e-9, classes=range(nc), max_det=8)[1]


@pytest.mark.gpu
def test_nms_entry_for_80_classes_equals_the_32_class_entry(nms_engine):
    """For nc <= 32 both entries give the same dets and counts, bit for bit (the wide one with its one mask word)."""
    import ctypes as C

    import torch

    from playaid_core_amd.engine import _ptr
    from playaid_core_amd.yolov5 import YoloV5Detector

    nc, net, n = 6, (384, 640), 4
    det = YoloV5Detector(synth.make_yolov5s_state_dict(), nc, net, max_images=n)
    try:
        pred = det(_frames(n, 1080, 1920, seed=3))
        torch.cuda.synchronize()
    finally:
        det.close()
    lib, h = nms_engine._lib, nms_engine._h
    for conf, mask in ((0.0005, 0b001100), (1e-6, 0b111111), (1e-6, 0b000001)):
        out = []
        for wide in (False, True):
            dets = torch.full((n, 8, 6), -1.0, device=pred.device)
            counts = torch.full((n,), -1, dtype=torch.int32, device=pred.device)
            args = (_ptr(pred), n, det.rows, nc, conf, 0.45)
            tail = (8, net[0], net[1], 1080, 1920, _ptr(dets), _ptr(counts), nms_engine._stream())
            if wide:
                rc = lib.pa_detect_postprocess_classes(h, *args, (C.c_uint32 * 1)(mask), *tail)
            else:
                rc = lib.pa_detect_postprocess(h, *args, mask, *tail)
            assert rc == 0
            torch.cuda.synchronize()
            out.append((dets.cpu().numpy(), counts.cpu().numpy()))
        assert out[0][1].min() > 0
        assert np.array_equal(out[0][1], out[1][1]) and out[0][0].tobytes() == out[1][0].tobytes()


def test_postprocess_refuses_class_ids_past_79():
    from playaid_core_amd.engine import Engine

    import torch

    class Fake:
        device = "cpu"

        @staticmethod
        def _dev(a, dt):
            return torch.as_tensor(a, dtype=dt)

    with pytest.raises(ValueError, match="0..79"):
        Engine.detect_postprocess(Fake(), np.zeros((1, 3, 85), np.float32), (64, 96), (64, 96), classes=(80,))
