"""Every row of the ResNet-50 table (``pa_convnet_*``, csrc/convnet.hip) against float64, one row at a time
(``pa_convnet_trace``), on both arithmetic choices of the fp32 path. Walk, bars and checks: tests/helpers/convnet_layers.py.

Cases (a fresh handle each): max_crops 64 -- the served group, ``min(max_rows, 64)`` -- with n = 1 (every tile partial),
37 (ragged: 37 x 16 pixels of the 4 x 4 maps end mid-tile) and 64; and max_crops 1, where no row has the tiles psgemm asks
for, so the emulated dtype runs every row on the exact kernels. Which kernel each row ran as comes from
``pa_convnet_layer_forms``; PA_CONVNET_WINO=0 runs in a child process so that the stride-1 3x3 rows reach the patch kernel.
"""
import json
import os
import subprocess
import sys

import pytest

from helpers import convnet_layers as cl

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def table():
    from playaid_core_amd import synth
    from playaid_core_amd.resnet_transformer_detector import build_resnet50_table

    return build_resnet50_table(synth.make_resformer_state_dict(seed=2468))


@pytest.mark.gpu
@pytest.mark.parametrize("max_crops, ns", [(64, (1, 37, 64)), (1, (1,))], ids=["64", "1"])
@pytest.mark.parametrize("dtype", ["f32", "emulated_f32"])
def test_convnet_rows_against_float64(table, dtype, max_crops, ns):
    from playaid_core_amd.resnet_transformer_detector import ConvNet

    descs, bufs, weights, dim = table
    for n in ns:
        net = ConvNet(descs, bufs, weights, dim, max_crops=max_crops, compute_dtype=dtype)
        try:
            r = cl.check_table(net, descs, weights, n, 7, f"{dtype} n={n}/{max_crops}")
        finally:
            net.close()
        forms = set(r["forms"])
        print(f"{dtype} n={n}/{max_crops} forms: {sorted(forms)}")
        assert r["forms"][0] == "stem_pool" and r["forms"][-1] == "avgpool"
        assert "wino" in forms and forms & {"igemm_128x128", "igemm_128x64", "igemm_64x64"}
        if dtype == "emulated_f32" and max_crops == 64:
            assert "psgemm" in forms
        else:
            assert "psgemm" not in forms


@pytest.mark.gpu
def test_convnet_patch_kernel_rows_against_float64():
    env = dict(os.environ, PA_CONVNET_WINO="0")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "convnet_knob_worker.py"), "f32,emulated_f32"],
                       capture_output=True, text=True, env=env, timeout=900)
    assert r.returncode == 0, f"exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    res = json.loads(r.stdout.strip().splitlines()[-1])
    for dtype, v in res.items():
        forms = set(v["forms"])
        print(f"PA_CONVNET_WINO=0 {dtype}: forms {sorted(forms)}; " + ", ".join(f"{k} {x:.3f}" for k, x in sorted(v["ratios"].items())))
        assert "wino" not in forms
        if dtype == "f32":
            assert "patch" in forms


@pytest.mark.gpu
def test_convnet_trace_refuses_bad_arguments(table):
    import torch

    from playaid_core_amd import _lib
    from playaid_core_amd.engine import EngineError, _ptr
    from playaid_core_amd.resnet_transformer_detector import ConvNet

    descs, bufs, weights, dim = table
    net = ConvNet(descs, bufs, weights, dim, max_crops=2)
    try:
        x = torch.zeros((3, 3, 128, 128), device="cuda")
        out = torch.empty(2 * max(bufs), device="cuda")
        lib, h = net._lib, net._h
        full = 2 * bufs[0] * 4
        assert lib.pa_convnet_trace(h, _ptr(x), 3, 0, 0, _ptr(out), full, None) == _lib.PA_ERR_INVALID_ARG   # n > max_crops
        assert lib.pa_convnet_trace(h, _ptr(x), 2, len(descs), 0, _ptr(out), full, None) == _lib.PA_ERR_INVALID_ARG
        assert lib.pa_convnet_trace(h, _ptr(x), 2, 0, len(bufs), _ptr(out), full, None) == _lib.PA_ERR_INVALID_ARG
        assert lib.pa_convnet_trace(h, _ptr(x), 2, 0, 0, _ptr(out), full - 4, None) == _lib.PA_ERR_INVALID_ARG
        assert lib.pa_convnet_trace(h, _ptr(x), 2, 0, 0, _ptr(out), full, None) == _lib.PA_OK
        with pytest.raises(EngineError):
            net.trace(x, 0, 0)
        torch.cuda.synchronize()
        assert net.layer_forms()[0] == "stem_pool" and set(net.layer_forms()[1:]) == {"not_run"}
    finally:
        net.close()
