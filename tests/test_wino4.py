"""Winograd F(4x4, 3x3) taken apart (``csrc/wino4.hip``: input transform, 36 grouped GEMMs on ``csrc/pigemm.hip``, output transform
with the epilogue) -- the form the exact fp32 engine runs ``torchvision.resnet18``'s layer 4 on (``cnn_action_detector.py:16,32``)
from ``PA_WINO_F4_MIN`` crops -- through the C ABI (``pa_wino4_conv3x3``) against torch's CPU ``conv2d`` in float64 at the project's
per-layer bar, 2e-5 of the layer's largest output, and inside the engine against a ``PA_WINO_F4=0`` process and the oracle's golden
clip.

Shapes: 4 x 4 maps at 1, 5, 64, 65 and 130 crops (one padded row tile; a full one; a group boundary inside a workgroup's run of
tiles; three row tiles per group) with (cin, cout) = (64, 64), (128, 64), (64, 128) (two and four k-steps, one and two channel
columns)."""
import ctypes
import os
import re
import shutil
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = os.path.join(ROOT, "tests", "golden")
BAR = 2e-5                    # tests/test_backbone_layers.py::F32_BAR
RATIO_BAR = 2 * 17            # error against F(2x2)'s on the same inputs: twice the CPU simulation's 4.2e-6 / 2.4e-7
CROPS = (1, 5, 64, 65, 130)
CHANNELS = ((64, 64), (128, 64), (64, 128))


def _inputs(n, cin, cout, seed, kind="random"):
    rng = np.random.default_rng(seed)
    if kind == "random":
        x = rng.standard_normal((n, cin, 4, 4)).astype(np.float32)
    elif kind == "zero":
        x = np.zeros((n, cin, 4, 4), np.float32)
    else:   # a single 1.0 per crop: the four corners and the centre in turn, in a channel that moves with the crop
        x = np.zeros((n, cin, 4, 4), np.float32)
        spots = ((0, 0), (0, 3), (3, 0), (3, 3), (1, 2))
        for i in range(n):
            y, xx = spots[i % 5]
            x[i, (7 * i + 3) % cin, y, xx] = 1.0
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    res = rng.standard_normal((n, cout, 4, 4)).astype(np.float32)
    return x, wt, b, res


def _pad(x_nchw, fill=0.0, pad=1):
    n, c, h, w = x_nchw.shape
    t = torch.full((n, h + 2 * pad, w + 2 * pad, c), fill, dtype=torch.float32)
    t[:, pad:pad + h, pad:pad + w, :] = torch.from_numpy(x_nchw).permute(0, 2, 3, 1)
    return t


def _ref(x, wt, b, res, act, residual, res_after):
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double() if b is not None else None, padding=1)
    if residual and not res_after:
        ref = ref + torch.from_numpy(res).double()
    if act == 1:
        ref = F.relu(ref)
    if residual and res_after:
        ref = ref + torch.from_numpy(res).double()
    return ref


def _case(n, cin, cout, seed, kind="random", act=0, bias=True, residual=False, res_after=False):
    """-> max |err| / max |ref| of one launch; also checks that nothing outside the interior is written."""
    from playaid_core_amd import wino

    dev = torch.device("cuda:0")
    x, wt, b, res = _inputs(n, cin, cout, seed, kind)
    u = torch.from_numpy(wino.transform_weights_f4(wt)).to(dev)
    out = torch.full((n, 6, 6, cout), -3.0, dtype=torch.float32)
    got = wino.conv3x3_f4(_pad(x).to(dev), u, cin, cout, bias=torch.from_numpy(b).to(dev) if bias else None,
                          residual=_pad(res).to(dev) if residual else None, out=out.to(dev), act=act, res_after=res_after).cpu()
    ref = _ref(x, wt, b if bias else None, res, act, residual, res_after)
    ring = torch.ones_like(got, dtype=torch.bool)
    ring[:, 1:5, 1:5, :] = False
    assert bool((got[ring] == -3.0).all()), "the output transform wrote outside the interior"
    inner = got[:, 1:5, 1:5, :].permute(0, 3, 1, 2).double()
    scale = float(ref.abs().max())
    if scale == 0.0:
        assert not inner.any()
        return 0.0
    return float((inner - ref).abs().max()) / scale


@pytest.mark.gpu
@pytest.mark.parametrize("channels", CHANNELS)
@pytest.mark.parametrize("n", CROPS)
def test_f4_matches_conv2d(n, channels):
    cin, cout = channels
    seed = n * 131 + cin + 7 * cout
    errs = {
        "random, bias": _case(n, cin, cout, seed),
        "random, residual + ReLU": _case(n, cin, cout, seed + 1, act=1, residual=True),
        "random, ReLU + residual": _case(n, cin, cout, seed + 2, act=1, residual=True, res_after=True),
        "random, no bias": _case(n, cin, cout, seed + 3, bias=False),
        "zero, bias + ReLU": _case(n, cin, cout, seed + 4, kind="zero", act=1),
        "zero, nothing": _case(n, cin, cout, seed + 5, kind="zero", bias=False),
        "single 1.0": _case(n, cin, cout, seed + 6, kind="ones", bias=False),
        "single 1.0, residual": _case(n, cin, cout, seed + 7, kind="ones", residual=True),
    }
    print(f"n={n} cin={cin} cout={cout}: " + ", ".join(f"{k}: {v:.3g}" for k, v in errs.items()))
    for k, v in errs.items():
        assert v <= BAR, (n, channels, k, v)


@pytest.mark.gpu
@pytest.mark.parametrize("channels", CHANNELS)
def test_f4_error_against_f2_on_the_same_inputs(channels):
    """The plain convolution (no epilogue) of the 130-crop batch on both Winograd kernels: F(4x4)'s error must stay under 2 x 17
    times F(2x2)'s (17 = the CPU simulation's 4.2e-6 / 2.4e-7; the margin covers another summation grouping)."""
    from playaid_core_amd import wino

    cin, cout = channels
    n = 130
    dev = torch.device("cuda:0")
    x, wt, b, res = _inputs(n, cin, cout, 977 + cin + 3 * cout)
    xp = _pad(x).to(dev)
    ref = _ref(x, wt, None, res, 0, False, False)
    g4 = wino.conv3x3_f4(xp, torch.from_numpy(wino.transform_weights_f4(wt)).to(dev), cin, cout).cpu()
    g2 = wino.conv3x3(xp, torch.from_numpy(wino.transform_weights(wt)).to(dev), cin, cout).cpu()
    e4, e2 = (float((g[:, 1:5, 1:5, :].permute(0, 3, 1, 2).double() - ref).abs().max() / ref.abs().max()) for g in (g4, g2))
    print(f"cin={cin} cout={cout} n={n}: F(4x4) {e4:.3g}, F(2x2) {e2:.3g}, ratio {e4 / e2:.3g}")
    assert e4 <= BAR and e2 <= BAR
    assert e4 / e2 <= RATIO_BAR, (channels, e4, e2)


@pytest.mark.gpu
def test_f4_is_repeatable_and_batch_independent():
    """Twenty launches give the same bits, and a crop alone (n = 1) has the bits it has at every position of the 130-crop batch:
    the grouped GEMM does not split K and a row's sum does not depend on its tile."""
    from playaid_core_amd import wino

    dev = torch.device("cuda:0")
    n, cin, cout = 130, 128, 64
    x, wt, b, res = _inputs(n, cin, cout, 55)
    u = torch.from_numpy(wino.transform_weights_f4(wt)).to(dev)
    xd, bd, rd = _pad(x).to(dev), torch.from_numpy(b).to(dev), _pad(res).to(dev)
    run = lambda lo, hi: wino.conv3x3_f4(xd[lo:hi].contiguous(), u, cin, cout, bias=bd, residual=rd[lo:hi].contiguous(), act=1).cpu().numpy().view(np.uint32)
    first = run(0, n)
    assert first.any()
    for _ in range(20):
        assert np.array_equal(run(0, n), first)
    for i in range(n):
        assert np.array_equal(run(i, i + 1)[0], first[i]), f"crop {i} of the batch differs from the crop alone"


def test_f4_refusals():
    """A map that is not 4 x 4, channels that are not multiples of 64, misaligned pointers, too little scratch: PA_ERR_INVALID_ARG
    before any launch (non-null addresses that are never dereferenced, as tests/test_abi.py reaches the launchers' host checks)."""
    from playaid_core_amd import _lib

    lib = _lib.load()
    z, a16, a4 = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    big = 36 * 64 * 128

    def call(x=a16, u=a16, bias=z, res=z, out=a16, n=1, h=4, w=4, cin=64, cout=64, ips=64, ops=64, pad=1, act=0, scratch=a16, floats=big):
        return lib.pa_wino4_conv3x3(x, u, bias, res, out, n, h, w, cin, cout, ips, ops, pad, act, 0, scratch, floats, z)

    bad = _lib.PA_ERR_INVALID_ARG
    assert call(h=8, w=8) == bad and call(h=4, w=8) == bad and call(h=2, w=2) == bad
    assert call(cin=32, ips=32) == bad and call(cin=96, ips=96) == bad and call(cout=32, ops=32) == bad and call(cout=72, ops=72) == bad
    assert call(x=a4) == bad and call(u=a4) == bad and call(out=a4) == bad and call(bias=a4) == bad and call(res=a4) == bad and call(scratch=a4) == bad
    assert call(x=z) == bad and call(u=z) == bad and call(out=z) == bad and call(scratch=z) == bad
    assert call(ips=60) == bad and call(ops=66) == bad and call(n=0) == bad and call(act=3) == bad
    assert call(floats=big - 1) == bad and call(n=65, floats=big) == bad


def test_group_kernel_store_count_matches_its_counted_waits():
    """The grouped GEMM is the persistent GEMM's body: its waits count NST = 4 MI sixteen-byte stores per tile and wave, and the
    built object must hold exactly that many per kernel (as tests/test_abi.py checks the plain kernels)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_abi import _device_disassembly

    asm = _device_disassembly("pigemm.o")
    if asm is None:
        pytest.skip("no llvm-objdump / object in this environment")
    parts = re.split(r"\n[0-9a-f]+ <(_ZN2pa18pgemm_group_kernel[^>]*)>:\n", asm)
    found = {}
    for name, body in zip(parts[1::2], parts[2::2]):
        m = re.match(r"_ZN2pa18pgemm_group_kernelILi(\d+)ELi(\d+)EEEvNS_10GemmParamsE", name)
        assert m, name
        bm, bn = int(m.group(1)), int(m.group(2))
        body = re.split(r"\n[0-9a-f]+ <[^>]+>:\n", body)[0].split("s_endpgm")[0]
        found[(bm, bn)] = (len(re.findall(r"\bglobal_store_dwordx4\b", body)), (bm // (2 if bn == 64 else 4) // 32) * 4)
    assert sorted(found) == [(64, 64), (128, 32), (128, 64)], sorted(found)
    for k, (count, nst) in found.items():
        assert count == nst, (k, count, nst)


# ---- the plan: a field of its own, two knobs ----------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def plan_table(tmp_path_factory):
    cxx = os.environ.get("CXX") or "g++"
    if not shutil.which(cxx.split()[0]):
        pytest.skip(f"no host C++ compiler ({cxx})")
    exe = str(tmp_path_factory.mktemp("wino4_plan") / "engine_plan_table")
    subprocess.run(cxx.split() + ["-std=c++17", "-O1", "-o", exe, os.path.join(ROOT, "tests", "helpers", "engine_plan_table.cpp")], check=True)

    def run(*args):
        """The knobs line and the rows of the four layers' second blocks (layerN.1.conv1: cin = cout = 64 .. 512 on maps of 32 .. 4)
        of the engine's own table; has_f4_filters: LayerDesc::wino4."""
        env = {k: v for k, v in os.environ.items() if not k.startswith("PA_")}
        out = subprocess.run([exe, *args], check=True, capture_output=True, text=True, env=env).stdout.splitlines()
        knobs = dict(x.split("=", 1) for x in out[0].split()[1:])
        plans = {}
        for line in out[1:]:
            kind, *fields = line.split()
            f = dict(x.split("=", 1) for x in fields)
            if kind == "plan" and f["layer"].endswith(".1.conv1"):
                f["has_f4_filters"] = f["wino4"]
                plans[(f["dtype"], int(f["max_crops"]), int(f["crops"]), f["layer"])] = f
        return knobs, plans

    return run


def test_plan_field_and_knobs(plan_table):
    knobs, plans = plan_table("f32:128:128", "f32:128:80", "f32:128:64", "f32:128:63", "f32:128:5", "f32:32:32", "emulated_f32:128:128", "bf16:128:128")
    assert knobs["wino_f4"] == "1" and knobs["wino_f4_min"] == knobs["default_min"]
    t = int(knobs["default_min"])
    assert t <= 80 or t > 128, "clips of 40 and of 64 frames (80 and 128 crops) must fall on the same side of the threshold"
    l4 = "layer4.1.conv1"
    for dt in ("f32", "emulated_f32"):
        p = plans[(dt, 128, 128, l4)]
        assert p["form"] == "wino" and p["wino_f4"] == str(int(128 >= t))
        if 128 >= t:
            assert float(p["flops_executed"]) == float(p["flops"]) / 4 == 2.0 * 128 * 16 * 512 * 512 * 9 / 4
    for n in (80, 64, 63, 5):
        p = plans[("f32", 128, n, l4)]
        assert p["form"] == "wino" and p["wino_f4"] == str(int(n >= t)), n
        assert float(p["flops_executed"]) == float(p["flops"]) * (1 / 4 if n >= t else 4 / 9)
    # an engine whose full batch stays below the threshold does not get the filters; layers 1-3 and the bf16 path never do
    assert plans[("f32", 32, 32, l4)]["has_f4_filters"] == str(int(32 >= t)) and plans[("f32", 32, 32, l4)]["wino_f4"] == str(int(32 >= t))
    for key, p in plans.items():
        if key[3] != l4 or key[0] == "bf16":
            assert p["wino_f4"] == "0" and p["has_f4_filters"] == "0", key
        if key[0] != "bf16":
            assert p["form"] == "wino", key
    # PA_WINO_F4=0: today's launches at every batch; PA_WINO_F4_MIN moves the threshold; PA_WINO=0 takes the layer off Winograd altogether
    _, off = plan_table("PA_WINO_F4=0", "f32:128:128")
    assert off[("f32", 128, 128, l4)]["wino_f4"] == "0" and off[("f32", 128, 128, l4)]["form"] == "wino"
    assert float(off[("f32", 128, 128, l4)]["flops_executed"]) == float(off[("f32", 128, 128, l4)]["flops"]) * 4 / 9
    k2, moved = plan_table("PA_WINO_F4_MIN=100", "f32:128:128", "f32:128:100", "f32:128:99", "f32:96:96")
    assert k2["wino_f4_min"] == "100"
    assert [moved[("f32", 128, n, l4)]["wino_f4"] for n in (128, 100, 99)] == ["1", "1", "0"]
    assert moved[("f32", 96, 96, l4)]["has_f4_filters"] == "0"
    _, nowino = plan_table("PA_WINO=0", "f32:128:128")
    assert nowino[("f32", 128, 128, l4)]["wino_f4"] == "0" and nowino[("f32", 128, 128, l4)]["form"] == "patch"


# ---- inside the engine ---------------------------------------------------------------------------------------------------------


@pytest.fixture(scope="module")
def engine_traces(tmp_path_factory):
    """The default process and a PA_WINO_F4=0 child (the knob is read once per process)."""
    d = tmp_path_factory.mktemp("wino4_engine")
    res = {}
    for tag, extra in (("default", {}), ("off", {"PA_WINO_F4": "0"})):
        path = str(d / f"{tag}.npz")
        env = {k: v for k, v in os.environ.items() if not k.startswith("PA_WINO_F4")}
        env.update(extra)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "wino4_worker.py"), path], capture_output=True, text=True, env=env,
                           timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = dict(np.load(path))
    return res


@pytest.mark.gpu
def test_engine_layer4_at_128_crops_against_the_f2_process(engine_traces):
    """Stages 14..17 at 128 crops: layer4.0.conv1 (not a Winograd layer) is bit-identical, the three stride-1 convolutions -- each
    fed by the previous stage of its own process -- stay within the per-layer bar of the F(2x2) process."""
    a, b = engine_traces["default"], engine_traces["off"]
    assert np.array_equal(a["n128_s14"].view(np.uint32), b["n128_s14"].view(np.uint32))
    for s in (15, 16, 17):
        x, y = a[f"n128_s{s}"].astype(np.float64), b[f"n128_s{s}"].astype(np.float64)
        assert (y != 0).mean() > 0.2, f"stage {s}: mostly zero, the comparison would be idle"
        d = float(np.abs(x - y).max() / np.abs(y).max())
        print(f"stage {s} at 128 crops: max |F(4x4) - F(2x2)| / max |F(2x2)| = {d:.3g}")
        assert d <= BAR, (s, d)
        assert not np.array_equal(x, y), f"stage {s}: the default process did not run another kernel than PA_WINO_F4=0"


@pytest.mark.gpu
def test_engine_below_the_threshold_is_bit_identical_to_the_knob(engine_traces):
    a, b = engine_traces["default"], engine_traces["off"]
    for s in (14, 15, 16, 17):
        assert a[f"n5_s{s}"].any()
        assert np.array_equal(a[f"n5_s{s}"].view(np.uint32), b[f"n5_s{s}"].view(np.uint32)), s


@pytest.mark.gpu
def test_engine_log_probabilities_against_the_oracle(engine_traces):
    """The committed 128-frame 1080p golden clip (oracle output) in 64-frame backbone batches -- 128 crops each, layer 4 as
    F(4x4) -- at the project's 1e-4, in both processes; max |dlogp| between the two is printed."""
    z = np.load(os.path.join(GOLD, "clip1080_128_logp.npz"))
    a, b = engine_traces["default"], engine_traces["off"]
    print(f"max |dlogp| default vs PA_WINO_F4=0: {np.abs(a['logp'] - b['logp']).max():.3g}; against the oracle: "
          f"{np.abs(a['logp'] - z['logp']).max():.3g} (default), {np.abs(b['logp'] - z['logp']).max():.3g} (PA_WINO_F4=0)")
    for got in (a, b):
        assert np.abs(got["logp"] - z["logp"]).max() <= 1e-4
        assert np.array_equal(got["action_id"], z["action_id"])
