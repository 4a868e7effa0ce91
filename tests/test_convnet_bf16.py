"""The ResNet-50 table (``pa_convnet_*``, csrc/convnet.hip) under ``compute_dtype="bf16"`` (PA_DTYPE_BF16): every row against
float64 from the stored operands (``pa_convnet_trace``), the forms it runs, the split-K form's repeatability and its knob, the whole
network against a CPU interpreter that rounds where the device rounds, ``ResnetTransformerDetector`` end to end, and on the CPU the
bars' sensitivity and the create-time refusals. References and bars: tests/helpers/convnet_layers_bf16.py; the rounding model:
include/playaid_hip.h next to pa_convnet_create_dtype.

bf16 is NOT within the fp32 path's 1e-4 bar: the whole network is held to the float64 interpreter of the same rounding model, and
the detector's distance to the fp32 oracle is held to a loose bar only.
"""
import ctypes as C
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import convnet_layers_bf16 as clb  # noqa: E402

from playaid_core_amd import _lib, synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SPLIT_FORBIDDEN = {"wino", "patch", "igemm_128x128", "igemm_128x64", "igemm_64x64", "psgemm", "avgpool"}


@pytest.fixture(scope="module")
def table():
    from playaid_core_amd.resnet_transformer_detector import build_resnet50_table

    return build_resnet50_table(synth.make_resformer_state_dict(seed=2468))


def _small_maps(descs):
    """The rows whose output map is 4 x 4 and whose K is 9 x 512: layer4's three conv2 rows."""
    return [i for i, d in enumerate(descs) if d["kind"] == 0 and d["ksize"] == 3 and d["in_hw"] // d["stride"] == 4 and d["cin"] == 512]


def _net(table, max_crops):
    from playaid_core_amd.resnet_transformer_detector import ConvNet

    descs, bufs, weights, dim = table
    return ConvNet(descs, bufs, weights, dim, max_crops=max_crops, compute_dtype="bf16")


# -- GPU ------------------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("max_crops, ns", [(64, (1, 37, 64)), (1, (1,))], ids=["64", "1"])
def test_bf16_convnet_rows_against_float64(table, max_crops, ns):
    descs, _, weights, _ = table
    for n in ns:
        net = _net(table, max_crops)
        try:
            r = clb.check_table(net, descs, weights, n, 7, f"bf16 n={n}/{max_crops}")
        finally:
            net.close()
        forms = r["forms"]
        print(f"bf16 n={n}/{max_crops} forms: " + ", ".join(f"{f} x{forms.count(f)}" for f in sorted(set(forms))))
        assert forms[0] == "stem_pool" and forms[-1] == "avgpool_bf16"
        assert set(forms[1:-1]) <= clb.CONV_FORMS, sorted(set(forms))
        assert not set(forms) & SPLIT_FORBIDDEN
        if max_crops == 64 and n == 64:
            split = [i for i, f in enumerate(forms) if f == "bgemm_splitk"]
            print(f"bf16 n=64/64: split-K rows {split}")
            assert set(_small_maps(descs)) <= set(split), (split, _small_maps(descs))


@pytest.mark.gpu
def test_bf16_convnet_forward_is_bitwise_repeatable(table):
    """Two forwards of the same 64 crops (split-K rows included) give the same bits; the features are live."""
    import torch

    net = _net(table, 64)
    try:
        x = torch.from_numpy(np.random.default_rng(11).integers(0, 256, (64, 3, 128, 128)).astype(np.float32) / 255).cuda()
        a = net.forward(x)
        assert "bgemm_splitk" in net.layer_forms()
        b = net.forward(x)
        torch.cuda.synchronize()
        assert torch.equal(a, b)
        assert a.dtype == torch.float32 and a.shape == (64, 2048) and float(a.abs().max()) > 0 and bool(torch.isfinite(a).all())
    finally:
        net.close()


@pytest.mark.gpu
def test_bf16_convnet_rows_without_split_k():
    """PA_CONVNET_BG_SPLIT=0 (read once: a child process): every row still passes the row bars, and no row is split."""
    env = dict(os.environ, PA_CONVNET_BG_SPLIT="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "convnet_bf16_knob_worker.py"), "37,64"],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for n, v in res.items():
        print(f"PA_CONVNET_BG_SPLIT=0 n={n}: " + ", ".join(f"{k} {x:.3f}" for k, x in sorted(v["ratios"].items())))
        assert "bgemm_splitk" not in v["forms"] and "bgemm" in v["forms"]


# Whole network: pooled features of the bf16 table against the float64 interpreter of the rounding model (clb.interpret), chained
# on its own values. A store that rounds the other way near a tie (the per-row bars allow 1 in 1000) moves every later row, so
# the distance is that of two bf16 runs. Measured on an MI355X (the run is bitwise repeatable), worst over the three crops,
# relative to max|feature|: 2.24e-3 (mean |d| / mean |ref| 1.7e-3); the bar is 3x that.
WHOLE_MEASURED = 2.24e-3
WHOLE_BAR = 3 * WHOLE_MEASURED


@pytest.mark.gpu
def test_bf16_convnet_features_against_the_rounding_model(table):
    import torch

    descs, _, weights, _ = table
    x = np.random.default_rng(23).integers(0, 256, (3, 3, 128, 128)).astype(np.float32) / np.float32(255)
    net = _net(table, 64)
    try:
        got = net.forward(torch.from_numpy(x).cuda()).double().cpu().numpy()
    finally:
        net.close()
    want, _, _ = clb.interpret(descs, weights, x)
    rel = float(np.abs(got - want).max() / np.abs(want).max())
    print(f"bf16 features vs the rounding model: max|d| / max|ref| = {rel:.3g} (bar {WHOLE_BAR:.3g}); "
          f"mean|d| / mean|ref| = {np.abs(got - want).mean() / np.abs(want).mean():.3g}")
    assert np.abs(want).max() > 0 and (want != 0).mean() > 0.2
    assert rel <= WHOLE_BAR


# ResnetTransformerDetector(compute_dtype="bf16") against the fp32 oracle (oracle/resformer.forward), which bf16 is not held to at
# 1e-4: measured on an MI355X over the three calls below, max |d log p| = 0.040 with 98 of 98 argmaxes agreeing; the bar is 3x the
# measurement, and at least 0.9 of the argmaxes must agree.
WHOLE_LOGP_MEASURED = 0.040
LOGP_BAR = 3 * WHOLE_LOGP_MEASURED


@pytest.mark.gpu
def test_bf16_resformer_detector_against_the_oracle():
    import torch

    from oracle import resformer as oracle_rf
    from playaid_core_amd.resnet_transformer_detector import ResnetTransformerDetector

    sd = synth.make_resformer_state_dict(seed=2468, num_actions=63, sequence_length=7)
    model = ResnetTransformerDetector([f"a{i}" for i in range(63)], sequence_length=7, state_dict=sd, max_rows=70, compute_dtype="bf16").eval()
    try:
        assert model._net.compute_dtype == "bf16" and model._net.max_crops == 64
        worst, agree, total = 0.0, 0, 0
        for b in (1, 3, 10):
            rng = np.random.default_rng(20 + b)
            x = torch.from_numpy(rng.integers(0, 256, size=(b, 7, 3, 128, 128)).astype(np.float32) / 255.0)
            want = oracle_rf.forward(x, sd).numpy()
            got = model(x).numpy()
            assert got.shape == (b, 7, 63) and np.isfinite(got).all()
            worst = max(worst, float(np.abs(got - want).max()))
            agree += int((got.argmax(2) == want.argmax(2)).sum())
            total += b * 7
        print(f"bf16 detector vs the fp32 oracle: max |d log p| = {worst:.4g} (bar {LOGP_BAR:.3g}), argmax agreement {agree}/{total}")
        assert worst <= LOGP_BAR and agree >= 0.9 * total
        with pytest.raises(ValueError):
            model(torch.zeros((2, 5, 3, 128, 128)))     # the checkpoint encodes 7 frame slots
        with pytest.raises(ValueError):
            model(torch.zeros((11, 7, 3, 128, 128)))    # 77 rows > max_rows
    finally:
        model.close()


@pytest.mark.gpu
def test_bf16_convnet_trace_checks_the_element_size(table):
    """pa_convnet_trace copies a bf16 buffer (and the input, buf = -1) as 2-byte elements and checks out_bytes against that size;
    the pooled buffer is 4-byte fp32."""
    import torch

    from playaid_core_amd.engine import _ptr

    descs, bufs, _, _ = table
    net = _net(table, 2)
    try:
        x = torch.zeros((2, 3, 128, 128), device="cuda")
        out = torch.empty(2 * max(max(bufs), 134 * 134 * 4), device="cuda")
        lib, h = net._lib, net._h
        pooled = descs[-1]["out_buf"]
        for b, es in ((-1, 2), (0, 2), (pooled, 4)):
            full = 2 * (134 * 134 * 4 if b < 0 else bufs[b]) * es
            assert lib.pa_convnet_trace(h, _ptr(x), 2, 0, b, _ptr(out), full - 2, None) == _lib.PA_ERR_INVALID_ARG
            assert lib.pa_convnet_trace(h, _ptr(x), 2, 0, b, _ptr(out), full, None) == _lib.PA_OK
            assert net.trace(x, 0, b).dtype == (torch.float32 if b == pooled else torch.bfloat16)
        torch.cuda.synchronize()
    finally:
        net.close()


# -- CPU --------------------------------------------------------------------------------------------------------------
def test_bf16_is_accepted_and_named():
    from playaid_core_amd.resnet_transformer_detector import ConvNet

    with pytest.raises(ValueError, match="'f32', 'emulated_f32' or 'bf16'"):
        ConvNet([], [], np.zeros(1, np.float32), 1, compute_dtype="fp16")
    assert _lib.CN_FORMS[9:] == ("bgemm", "bgemm_splitk", "avgpool_bf16")
    hdr = open(os.path.join(ROOT, "include", "playaid_hip.h")).read()
    body = re.search(r"typedef enum pa_cn_form \{(.*?)\} pa_cn_form;", hdr, re.S).group(1)
    enum = {int(v): name.lower() for name, v in re.findall(r"PA_CN_FORM_(\w+)\s*=\s*(\d+)", body)}
    assert tuple(enum[i] for i in range(len(enum))) == _lib.CN_FORMS
    assert re.search(r"#define PA_ABI_VERSION (\d+)", hdr).group(1) == "15"


def _create(descs, bufs, weights, dtype):
    lib = _lib.load()
    arr = (_lib.pa_conv_desc * len(descs))()
    for i, d in enumerate(descs):
        for k, v in d.items():
            setattr(arr[i], k, int(v))
    bb = (C.c_int64 * len(bufs))(*bufs)
    w = np.ascontiguousarray(weights, np.float32)
    h = C.c_void_p()
    rc = lib.pa_convnet_create_dtype(0, arr, len(descs), bb, len(bufs), w.ctypes.data_as(C.c_void_p), w.size, 4, dtype, C.byref(h))
    msg = lib.pa_convnet_last_error(h).decode() if h else ""
    lib.pa_convnet_destroy(h)
    return rc, msg


def test_bf16_create_refuses_what_it_cannot_run():
    """Refused before the device is touched, naming the row: a buffer written as both bf16 and fp32, a row reading fp32, a
    convolution bgemm cannot take (SiLU), a table that does not end in a pool. The same tables in fp32 get past validation."""
    conv = dict(kind=0, cin=64, cout=64, ksize=1, stride=1, in_hw=8, in_buf=0, in_pad=0, out_buf=1, out_pad=0, res_buf=-1, relu=1, w_off=0, b_off=4096)
    pool = dict(kind=2, cin=64, cout=64, ksize=1, stride=1, in_hw=8, in_buf=1, in_pad=0, out_buf=2, out_pad=0, res_buf=-1, relu=0, w_off=0, b_off=0)
    bufs, w = [4096, 4096, 4096], np.zeros(4096 + 64, np.float32)
    cases = {
        "written as both": [conv, dict(pool, out_buf=1), dict(pool, out_buf=2)],
        "reads an fp32 buffer": [conv, pool, dict(conv, in_hw=1, in_buf=2, out_buf=0), dict(pool, in_hw=1, in_buf=0)],
        "cannot take": [dict(conv, relu=2), pool],
        "must end in a pool": [conv],
    }
    for what, descs in cases.items():
        rc, msg = _create(descs, bufs, w, _lib.DTYPES["bf16"])
        assert rc == _lib.PA_ERR_INVALID_ARG and what in msg and msg.startswith("layer "), (what, rc, msg)
        rc, msg = _create(descs, bufs, w, _lib.DTYPES["f32"])
        assert what not in msg, (what, msg)


@pytest.fixture(scope="module")
def interpreted(table):
    """Two crops through the whole table under the rounding model, the buffers kept in front of the rows the fault tests use."""
    descs, _, weights, _ = table
    x = np.random.default_rng(3).integers(0, 256, (2, 3, 128, 128)).astype(np.float32) / np.float32(255)
    rows = _fault_rows(descs)
    feats, before, last = clb.interpret(descs, weights, x, keep=set(rows.values()) | {len(descs) - 1})
    return x, feats, before, last, rows


def _fault_rows(descs):
    last3 = next(i for i, d in enumerate(descs) if d["kind"] == 0 and d["ksize"] == 3 and d["stride"] == 1 and d["cin"] == 128)
    res = next(i for i, d in enumerate(descs) if d["kind"] == 0 and d["res_buf"] >= 0 and d["cout"] == 512)
    return {"stem": 0, "conv3x3": last3, "residual": res, "pool": len(descs) - 1}


CASES = [("truncated_weights", "stem"), ("truncated_weights", "conv3x3"), ("residual_after_relu", "residual"),
         ("no_store_rounding", "stem"), ("no_store_rounding", "conv3x3"), ("bias_dropped", "stem"), ("bias_dropped", "residual"),
         ("pool_rounded_to_bf16", "pool")]


@pytest.mark.parametrize("fault, kind", CASES, ids=[f"{f}-{k}" for f, k in CASES])
def test_bf16_row_bar_rejects_seeded_faults(table, interpreted, fault, kind):
    """The interpreter's row passes the row bar on its stored operands; the same row with one fault of the rounding model does not."""
    descs, _, weights, _ = table
    x, _, before, _, rows = interpreted
    k = rows[kind]
    d = dict(descs[k], _row=k)
    xs = clb.rne_bf16(np.asarray(x, np.float64)).transpose(0, 2, 3, 1)
    ohw, opad, _ = clb.out_geom(d)

    def out_of(f):
        bufs = {b: a.copy() for b, a in before[k].items()}
        clb.run_row(d, weights, bufs, xs, f)
        a = bufs[d["out_buf"]]
        return a.reshape(a.shape[0], -1) if d["kind"] == 2 else clb._interior(a, opad)

    r, m = clb.check_row(d, weights, before[k], out_of(None), xs)
    assert r <= 1.0 and m == 1.0, (r, m)
    with pytest.raises(clb.LayerFault):
        clb.check_row(d, weights, before[k], out_of(fault), xs)


def test_bf16_interpreter_buffers_hold_bf16(table, interpreted):
    """Every buffer a stem or convolution row writes holds bf16 values only; the pooled fp32 features do not, and are live."""
    descs, _, _, _ = table
    _, feats, _, last, _ = interpreted
    pooled = descs[-1]["out_buf"]
    for b, a in last.items():
        if b == pooled:
            assert not np.array_equal(a, clb.rne_bf16(a)), b
        else:
            assert np.array_equal(a, clb.rne_bf16(a)), b
    assert np.isfinite(feats).all() and (feats > 0).mean() > 0.2
