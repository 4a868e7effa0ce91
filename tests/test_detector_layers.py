"""Every row of the detector's layer table against float64, one row at a time (``pa_detector_trace``), on both compute dtypes.

Each row's reference is built in float64 from the buffers the device stored after the row before, interior only, so errors
do not add up along the table and a row is named with the kernel form it ran as (``pa_detector_layer_forms``). The
references, bars and the walk live in tests/helpers/detector_layers.py (its docstring states the bars); the in-place
bottleneck (``X += conv3x3(R)``) takes as its residual the output slice as the row before left it.

Cases, frames of 720p, 1080p and 270 x 480 (enlarged) mixed, both dtypes:
  * net 384 x 640 on 480 x 640 frames (left and right borders) and net 640 x 384 on 853 x 481 frames (portrait, unequal borders);
  * net 384 x 640: 1 and 3 frames of a 4-image handle; 64 of 64 (configs[1]), every image on the exact and the bitwise
    checks, a float64 sample of seven images on the convolutions (``sample_images``);
  * nets 320 x 320, 352 x 608, 64 x 96, 3 frames: maps whose sides are not multiples of four (10 x 10; 22 x 38 and 11 x 19;
    4 x 6 and 2 x 3), where Winograd refuses and the others take over;
  * the 384 x 640 table with every buffer 4096 floats larger per image than its rows' geometry.

Kernel forms reached at the default knobs, from the launch chain of csrc/yolo.hip (psgemm -> Winograd -> patch -> persistent
GEMM -> igemm, each refusing a shape with hipErrorInvalidValue), confirmed by the coverage test on an MI355X:
  * f32: stem_direct, wino, pgemm, pgemm_up (model.10 / model.14 with the next row's up-sampling), igemm (the residual
    bottlenecks on maps Winograd refuses: 320 x 320, 352 x 608, 64 x 96), sppf, absorbed, decode;
  * emulated_f32: stem_bf16, wino, psgemm (also the stride-1 3x3 layers Winograd refuses, residual ones included),
    psgemm_up, sppf, absorbed, decode.
Not reachable at the default knobs: ``patch`` (the blocked kernel takes 4 x 4, 8 x 8 or 8 x 16 blocks, so every map it accepts
Winograd accepts first), ``maxpool`` (SPPF fuses its three pools on every map up to 480 pixels: 12 x 20 at 384 x 640),
``upsample`` (both up-samplings fuse into their producer). They are reached by the knob pass: PA_DET_WINO=0 (f32: the patch
kernel on every stride-1 3x3 layer whose map it blocks; the emulated dtype sends those layers to psgemm), PA_DET_SPPF=0,
PA_DET_UP_FUSE=0, and PA_DET_EMU_S1=1 sends the emulated stride-1 3x3 layers to psgemm.
"""
import json
import os
import subprocess
import sys
import time

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import detector_layers as dl  # noqa: E402

from playaid_core_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NC = 6
DTYPES = ["f32", "emulated_f32"]
DEFAULT_FORMS = {
    "f32": {"stem_direct", "wino", "pgemm", "pgemm_up", "igemm", "sppf", "absorbed", "decode"},
    "emulated_f32": {"stem_bf16", "wino", "psgemm", "psgemm_up", "sppf", "absorbed", "decode"},
}
# (net, max_images, [(n, frame h, frame w)], buf_slack)
CASES = {
    "384x640": ((384, 640), 4, [(3, 1080, 1920), (1, 270, 480)], 0),
    "384x640_64": ((384, 640), 64, [(64, 720, 1280)], 0),
    "320x320": ((320, 320), 3, [(3, 720, 1280)], 0),
    "352x608": ((352, 608), 3, [(3, 1080, 1920)], 0),
    "64x96": ((64, 96), 3, [(3, 270, 480)], 0),
    "384x640_padded": ((384, 640), 4, [(3, 720, 1280)], 4096),
    # frames that are not 16:9 (tests/test_frame_geometry.py walks the letterbox alone over more of them): 4:3 with 64 grey
    # columns on each side, and a portrait frame in a portrait input with 11 / 12 grey columns
    "384x640_4:3": ((384, 640), 3, [(3, 480, 640)], 0),
    "640x384_portrait": ((640, 384), 3, [(3, 853, 481)], 0),
}
_SEEN = {}   # dtype -> {form: worst ratio}, and the forms per case, for the coverage test


def run_case(dtype, net, cap, runs, slack=0, log=print):
    from playaid_core_amd.yolov5 import YoloV5Detector

    sd = synth.make_yolov5s_state_dict()
    det = YoloV5Detector(sd, NC, net, max_images=cap, compute_dtype=dtype, buf_slack=slack)
    out = []
    try:
        for n, fh, fw in runs:
            frames = synth.make_frames(n, fh, fw, seed=n + fh)
            res = dl.check_detector(det, frames, f"{dtype} net {net[0]}x{net[1]} n={n}/{cap}" + (" padded" if slack else ""))
            out.append(res)
            worst = ", ".join(f"{k} {v:.3f}" for k, v in sorted(res["ratios"].items()))
            log(f"{dtype} net {net} n={n}/{cap}{' padded' if slack else ''}: conv ratios {worst}; decode {res['decode']:.3f}")
    finally:
        det.close()
    return out


@pytest.mark.gpu
@pytest.mark.parametrize("case", list(CASES))
@pytest.mark.parametrize("dtype", DTYPES)
def test_detector_rows_against_float64(dtype, case):
    net, cap, runs, slack = CASES[case]
    t0 = time.time()
    results = run_case(dtype, net, cap, runs, slack)
    seen = _SEEN.setdefault(dtype, {})
    for res in results:
        for form, r in res["ratios"].items():
            seen[form] = max(seen.get(form, 0.0), r)
        for form in res["forms"]:
            seen.setdefault(form, 0.0)
        seen.setdefault("decode", 0.0)
        seen["decode"] = max(seen["decode"], res["decode"])
    print(f"{dtype} {case}: {time.time() - t0:.1f} s")


@pytest.mark.gpu
def test_padded_table_gives_the_same_rows():
    """A table whose buffers are larger per image than their rows' geometry (the public table API allows it): the same rows,
    bit for bit, as the tight table, at the default knobs (the checker above runs on it as well)."""
    from playaid_core_amd.yolov5 import YoloV5Detector

    sd = synth.make_yolov5s_state_dict()
    frames = synth.make_frames(3, 720, 1280, seed=5)
    for dtype in DTYPES:
        rows = []
        for slack in (0, 4096):
            det = YoloV5Detector(sd, NC, (384, 640), max_images=4, compute_dtype=dtype, buf_slack=slack)
            try:
                rows.append(det(frames).cpu().numpy())
            finally:
                det.close()
        assert np.array_equal(rows[0], rows[1]), dtype


@pytest.mark.gpu
def test_every_default_form_is_covered():
    """The union of the forms the cases above ran (per dtype) is every form reachable at the default knobs (module docstring).
    Prints the worst ratio to the bar per form and dtype."""
    if set(_SEEN) != set(DTYPES):
        pytest.skip("needs the cases of test_detector_rows_against_float64 in this session")
    for dtype in DTYPES:
        forms = set(_SEEN[dtype])
        print(dtype + ": " + ", ".join(f"{f} {_SEEN[dtype][f]:.3f}" for f in sorted(_SEEN[dtype])))
        assert forms == DEFAULT_FORMS[dtype], (dtype, sorted(forms ^ DEFAULT_FORMS[dtype]))


# (knob, dtypes, the form it must reach)
KNOB_PASS = [
    ({"PA_DET_SPPF": "0"}, DTYPES, "maxpool"),
    ({"PA_DET_UP_FUSE": "0"}, DTYPES, "upsample"),
    ({"PA_DET_EMU_S1": "1"}, ["emulated_f32"], "psgemm"),
    ({"PA_DET_WINO": "0"}, ["f32"], "patch"),   # (the emulated dtype then runs those layers on psgemm, as PA_DET_EMU_S1=1)
]


@pytest.mark.gpu
@pytest.mark.parametrize("knob,dtypes,form", KNOB_PASS, ids=[",".join(f"{k}={v}" for k, v in kn.items()) for kn, _, _ in KNOB_PASS])
def test_knob_forms_against_float64(knob, dtypes, form):
    """Kernel forms reached only under A/B knobs, checked by the same walk in a child process (knobs are read once per
    process): 384 x 640 and 64 x 96, three frames."""
    env = dict(os.environ, **knob)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "detector_knob_worker.py"), ",".join(dtypes)],
                       capture_output=True, text=True, env=env, timeout=600)
    print(r.stdout[-3000:])
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for dtype in dtypes:
        assert form in res[dtype]["forms"], (knob, dtype, res[dtype]["forms"])
        if knob == {"PA_DET_EMU_S1": "1"}:
            # every stride-1 3x3 row on psgemm: none left on Winograd
            assert "wino" not in res[dtype]["forms"], res[dtype]["forms"]


@pytest.mark.gpu
def test_trace_refuses_bad_arguments():
    import ctypes as C

    from playaid_core_amd import _lib
    from playaid_core_amd.yolov5 import YoloV5Detector

    det = YoloV5Detector(synth.make_yolov5s_state_dict(), NC, (64, 96), max_images=2)
    try:
        frames = torch.from_numpy(synth.make_frames(2, 270, 480)).cuda()
        pred = torch.zeros((2, det.rows, 5 + NC), device="cuda")
        out = torch.empty(1 << 22, device="cuda")
        lib, s = det._lib, C.c_void_p(torch.cuda.current_stream().cuda_stream)
        nb = det.buf_geometry[0]
        one = (nb[0] + 2 * nb[2]) * (nb[1] + 2 * nb[2]) * nb[3] * 4   # buffer 0, one image, in bytes

        def call(n=2, last=5, buf=0, img0=0, n_img=1, nbytes=one):
            return lib.pa_detector_trace(det._h, C.c_void_p(frames.data_ptr()), n, 270, 480, last, buf, img0, n_img, C.c_void_p(out.data_ptr()), nbytes,
                                         C.c_void_p(pred.data_ptr()), None, s)

        bad = _lib.PA_ERR_INVALID_ARG
        assert call(last=det.n_layers) == bad and call(last=-2) == bad
        assert call(buf=len(det.buf_geometry)) == bad and call(buf=-2) == bad
        assert call(img0=2) == bad and call(img0=1, n_img=2) == bad and call(n_img=0) == bad and call(img0=-1) == bad
        assert call(n=3) == bad and call(n=0) == bad
        assert call(nbytes=one - 4) == bad
        assert call() == _lib.PA_OK and call(img0=1, n_img=1) == _lib.PA_OK and call(last=-1, buf=-1, nbytes=1 << 24) == _lib.PA_OK
        forms = (C.c_int32 * det.n_layers)()
        assert lib.pa_detector_layer_forms(det._h, forms, det.n_layers - 1) == bad
        assert lib.pa_detector_layer_forms(det._h, forms, det.n_layers) == _lib.PA_OK
        torch.cuda.synchronize()
        # the trace through row 5 ran rows 0..5 only; the letterbox-only call ran none (forms are of the last call that ran a row)
        assert [f for f in det.layer_forms()[:6]] != ["not_run"] * 6 and det.layer_forms()[6:] == ["not_run"] * (det.n_layers - 6)
        # a row an earlier launch absorbs: the call reports the end of the group
        sppf = next(i for i, L in enumerate(det.layers) if L.kind == 4)
        assert det.trace(frames, sppf, det.layers[sppf].out_buf, 0, 2)[1] == sppf + 2
        assert det.trace(frames, sppf + 1, det.layers[sppf].out_buf, 0, 2)[1] == sppf + 2
        assert det.trace(frames, -1, -1, 0, 2)[1] == -1
    finally:
        det.close()


# -- CPU: the references themselves ------------------------------------------------------------------------
def _fp32_folded_state_dict(sd):
    """sd with every Conv + BatchNorm replaced by its fold (eps 1e-3) rounded to fp32 and an identity BatchNorm -- mean 0,
    var 1 - 1e-3 (var + eps == 1.0 exactly in float64), weight 1, bias the folded bias: the graph with the weights rounded
    as the table stores them, computed from the state dict independently of the table builder."""
    out = dict(sd)
    for key in sd:
        if not key.endswith(".conv.weight"):
            continue
        p = key[:-len(".conv.weight")]
        w = np.asarray(sd[key], np.float64)
        g, b, m, v = (np.asarray(sd[p + ".bn." + k], np.float64) for k in ("weight", "bias", "running_mean", "running_var"))
        s = g / np.sqrt(v + 1e-3)
        out[key] = (w * s[:, None, None, None]).astype(np.float32)
        out[p + ".bn.bias"] = (b - m * s).astype(np.float32)
        out[p + ".bn.weight"] = np.ones_like(g, np.float32)
        out[p + ".bn.running_mean"] = np.zeros_like(g, np.float32)
        out[p + ".bn.running_var"] = np.full(g.shape, 1.0 - 1e-3)
    return {k: torch.from_numpy(np.asarray(v)).double() for k, v in out.items()}


@pytest.mark.parametrize("net", [(64, 96), (384, 640)])
def test_interpreter_of_the_table_is_the_graph(net):
    """A float64 interpreter of build_yolov5s_table's rows (helpers.detector_layers.interpret: the per-row references of the
    GPU test, chained on their own outputs) equals oracle.yolov5.forward in float64 on a letter-boxed frame.

    Bar. The table stores each folded weight and bias rounded to fp32 once; that rounding is the only difference the bar
    allows for, and it is taken out exactly: the oracle runs on the state dict whose Conv + BatchNorm pairs are replaced by
    those fp32 folds with identity BatchNorms (``_fp32_folded_state_dict``, folded from the checkpoint keys, not by the
    table builder). Both runs then hold the same real weights and differ by float64 summation order alone: at most K * 2^-53
    relative per row for K <= 9 * 512 terms, ~5e-13, through 60 rows. The bar, 1e-9 of the largest |value| per column
    group (boxes, scores), leaves a factor of ~30 for amplification along the table per row on top of that and is still
    five orders below one fp32 rounding of the weights left in (measured 1e-5 px, 1e-7 on scores), so a wrong slice,
    weight layout, fold or wiring cannot pass."""
    from oracle import yolov5 as oy
    from playaid_core_amd.yolov5 import build_yolov5s_table

    sd = synth.make_yolov5s_state_dict()
    layers, _, blob, rows = build_yolov5s_table(sd, net, NC)
    frames = synth.make_frames(1, 270, 480, seed=3)
    x = torch.from_numpy(np.stack([oy.letterbox(f, net) for f in frames])).double()
    got = dl.interpret(layers, blob, x.numpy(), NC)
    want = oy.forward(x, _fp32_folded_state_dict(sd), NC).numpy()
    assert got.shape == want.shape == (1, rows, 5 + NC)
    for name, sl in (("boxes", slice(0, 4)), ("scores", slice(4, None))):
        err = np.abs(got[..., sl] - want[..., sl]).max() / np.abs(want[..., sl]).max()
        print(f"net {net} {name}: max |interpreter - oracle| = {err:.2e} of max |oracle|")
        assert err <= 1e-9, (name, err)


def _row(**kw):
    from playaid_core_amd import _lib

    L = _lib.pa_net_layer()
    d = dict(kind=0, cin=64, cout=64, ksize=3, stride=1, in_h=8, in_w=8, in_buf=0, in_coff=0, in_cstride=64, in_pad=1, out_buf=1,
             out_coff=64, out_cstride=128, out_pad=1, res_buf=1, res_coff=64, act=2, res_after=1, w_off=0, b_off=64 * 9 * 64)
    d.update(kw)
    for k, v in d.items():
        setattr(L, k, v)
    return L


def test_conv_checker_accepts_fp32_and_rejects_known_faults():
    """The per-row convolution check (helpers.detector_layers.check_conv_row, the GPU test's) passes the float64 result
    rounded to fp32 and rejects: a dropped 32-channel K chunk, a tap shifted by one pixel, a stride-2 phase off by one, a
    residual added before SiLU instead of after, ReLU in place of SiLU, and a write into the neighbouring channel slice."""
    import torch.nn.functional as F

    rng = np.random.default_rng(4)
    n = 3
    blob = np.concatenate([(rng.standard_normal(64 * 9 * 64) / np.sqrt(9 * 64)).astype(np.float32),
                           (rng.standard_normal(64) * 0.3).astype(np.float32)])

    def buffers(hw):
        b0 = np.zeros((n, hw + 2, hw + 2, 64), np.float32)
        b0[:, 1:-1, 1:-1] = dl.activation(rng.standard_normal((n, hw, hw, 64)), 2)
        oh = hw
        b1 = np.zeros((n, oh + 2, oh + 2, 128), np.float32)
        b1[:, 1:-1, 1:-1] = dl.activation(rng.standard_normal((n, oh, oh, 128)), 2)
        return {0: b0, 1: b1}

    def stored(L, before, y):
        a = before[1].copy()
        a[:, 1:-1, 1:-1, 64:128] = y.astype(np.float32)
        return a

    def conv(L, before, **kw):
        w, b = dl.row_weights(L, blob)
        x = before[0][:, 1:-1, 1:-1, :].astype(np.float64)
        res = before[1][:, 1:-1, 1:-1, 64:128].astype(np.float64)
        if kw.get("drop"):
            w = w.copy()
            w[:, 32:64, 1, 2] = 0.0
        if kw.get("shift"):
            w1 = np.zeros_like(w)
            w1[:, :, 0, 1] = w[:, :, 0, 1]
            w = w.copy()
            w[:, :, 0, 1] = 0.0
            shifted = np.roll(np.pad(x, ((0, 0), (1, 1), (1, 1), (0, 0))), -1, axis=2)[:, 1:-1, 1:-1]
            return (dl.ref_conv(x, w, b, 1, 0) + dl.ref_conv(shifted, w1, np.zeros_like(b), 1, 0), res)
        return w, b, x, res

    L = _row()
    before = buffers(8)
    w, b, x, res = conv(L, before)
    good1 = dl.ref_conv(x, w, b, 1, 2, res, 1)
    assert dl.check_conv_row(L, blob, before, stored(L, before, good1), n, np.arange(n), "good") <= 0.1
    faults = {}
    w2, b2, x2, r2 = conv(L, before, drop=True)
    faults["dropped K chunk"] = dl.ref_conv(x2, w2, b2, 1, 2, r2, 1)
    pre, r3 = conv(L, before, shift=True)
    faults["shifted tap"] = dl.activation(pre, 2) + r3
    faults["residual before SiLU"] = dl.ref_conv(x, w, b, 1, 2, res, 0)
    faults["ReLU for SiLU"] = dl.ref_conv(x, w, b, 1, 1, res, 1)
    for what, y in faults.items():
        with pytest.raises(dl.LayerFault):
            dl.check_conv_row(L, blob, before, stored(L, before, y), n, np.arange(n), what)
    # a write into the neighbouring channel slice (the other producer's half of a concatenation buffer)
    a = stored(L, before, good1)
    a[:, 1:-1, 1:-1, 60:64] = a[:, 1:-1, 1:-1, 64:68]
    with pytest.raises(dl.LayerFault, match="outside the written slice"):
        dl.check_conv_row(L, blob, before, a, n, np.arange(n), "neighbour slice")
    # a stride-2 convolution (16 x 16 -> 8 x 8) whose output pixel reads the input one pixel off its phase
    L2 = _row(in_h=16, in_w=16, stride=2, res_buf=-1)
    before2 = buffers(16)
    before2[1] = before[1].copy()
    w, b = dl.row_weights(L2, blob)
    x = before2[0][:, 1:-1, 1:-1, :].astype(np.float64)
    good = dl.ref_conv(x, w, b, 2, 2)
    assert dl.check_conv_row(L2, blob, before2, stored(L2, before2, good), n, np.arange(n), "good s2") <= 0.1
    t = torch.from_numpy(x).permute(0, 3, 1, 2)
    off = F.conv2d(F.pad(t, (0, 2, 0, 2)), torch.from_numpy(w), torch.from_numpy(b), stride=2)   # rows / columns 2 o .. 2 o + 2
    bad = dl.activation(off.permute(0, 2, 3, 1).numpy(), 2)
    with pytest.raises(dl.LayerFault):
        dl.check_conv_row(L2, blob, before2, stored(L2, before2, bad), n, np.arange(n), "stride-2 phase")
    # a partial last tile that stores into image n of a batch of n = 2
    a = stored(L, before, good1)
    a[2, 3, 3, 70] += 1.0
    with pytest.raises(dl.LayerFault, match="images past n"):
        dl.check_conv_row(L, blob, before, a, 2, np.arange(2), "store past n")


def test_decode_bar_accepts_fp32_and_rejects_a_wrong_grid():
    """The decode bar passes the kernel's fp32 arithmetic (emulated here in numpy float32, expf from float64) and rejects a
    grid offset of 0.5 px."""
    rng = np.random.default_rng(8)
    v = (rng.standard_normal((2, 4, 6, 33)) * 4).astype(np.float32)
    anchors = [np.float32(a) for a in (10.0, 13.0, 16.0, 30.0, 33.0, 23.0)]
    ref, s = dl.ref_decode(v, 8.0, anchors)
    bar = dl.decode_bar(ref, s, dl._v_rows(v), 8.0, anchors)
    vr = dl._v_rows(v).astype(np.float32)
    s32 = (np.float32(1) / (np.float32(1) + np.exp(-vr.astype(np.float64)).astype(np.float32))).astype(np.float32)
    got = s32.copy()
    hw = np.arange(3 * 4 * 6) % 24
    gx = (hw % 6).astype(np.float32) - np.float32(0.5)
    gy = (hw // 6).astype(np.float32) - np.float32(0.5)
    got[..., 0] = (s32[..., 0] * np.float32(2) + gx) * np.float32(8)
    got[..., 1] = (s32[..., 1] * np.float32(2) + gy) * np.float32(8)
    a = np.repeat(np.array(anchors, np.float32).reshape(3, 2), 24, axis=0)
    got[..., 2] = (s32[..., 2] * np.float32(2)) * (s32[..., 2] * np.float32(2)) * a[:, 0]
    got[..., 3] = (s32[..., 3] * np.float32(2)) * (s32[..., 3] * np.float32(2)) * a[:, 1]
    assert (np.abs(got - ref) <= bar).all(), float((np.abs(got - ref) / bar).max())
    bad = got.copy()
    bad[..., 0] += np.float32(8 * 0.5)
    assert not (np.abs(bad - ref) <= bar).all()
