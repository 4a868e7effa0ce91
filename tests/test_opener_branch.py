"""A ResNet block's stride-2 3x3 opener that takes the block's 1x1/2 downsample branch along on its centre tap
(``csrc/pigemm.hip``: ``pgemm_branch_kernel``; ``torchvision.resnet18``'s ``layerX.0.conv1`` + ``layerX.0.downsample``,
``cnn_action_detector.py:16,32``), through the C ABI (``pa_conv2d_branch``) and inside the exact fp32 engine.

The fused launch replaces two launches and is held to THEIR bits: ``out`` to ``pa_conv2d``'s 3x3/2 with bias + ReLU, ``out2`` to
``pa_conv2d``'s 1x1/2 without bias or activation (same k order: channel chunk, eight-wide group, lane half, from zero). Both are
also held to torch's CPU ``conv2d`` in float64 at the exact kernel's bar of tests/test_psgemm.py: 2e-5 of the layer's largest
output. In the engine the default process is compared with ``PA_F32_DS_FUSE=0`` (the branch as a GEMM of its own), bit for bit."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHAPES = [
    # n, in h, in w, cin, cout
    (1, 8, 8, 32, 64),        # M = 16: a single partial tile (its second wave row stores nothing)
    (5, 8, 8, 64, 128),       # M = 80: a full and a partial tile, two channel columns, the centre tap spans two k-steps
    (192, 16, 16, 32, 512),   # M = 12288, eight channel columns: three tiles per workgroup, centre-tap copies issued across tile boundaries
    (2, 32, 32, 64, 128),     # layer 2's own geometry
]


def _inputs(shape, seed):
    n, h, w, cin, cout = shape
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    w3 = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    w1 = (rng.standard_normal((cout, cin, 1, 1)) / np.sqrt(cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    return x, w3, w1, b


def _device_case(shape, seed):
    """-> (x, w3, w1, b on the host; x_pad, packed 3x3, packed 1x1, [cout][cin] branch weights, bias on the device)"""
    from playaid_core_amd import conv

    n, h, w, cin, cout = shape
    x, w3, w1, b = _inputs(shape, seed)
    dev = torch.device("cuda:0")
    xp = torch.zeros((n, h + 2, w + 2, cin), dtype=torch.float32)
    xp[:, 1:1 + h, 1:1 + w, :] = torch.from_numpy(x).permute(0, 2, 3, 1)
    w3p = torch.from_numpy(conv.pack_weights(w3, "f32")).to(dev)
    w1p = torch.from_numpy(conv.pack_weights(w1, "f32")).to(dev)
    w2 = torch.from_numpy(np.ascontiguousarray(w1.reshape(cout, cin))).to(dev)
    return (x, w3, w1, b), (xp.to(dev), w3p, w1p, w2, torch.from_numpy(b).to(dev))


def _canvas(shape):
    n, h, w, cin, cout = shape
    return torch.full((n, h // 2 + 2, w // 2 + 2, cout), -3.0, dtype=torch.float32, device="cuda:0")


@pytest.mark.gpu
@pytest.mark.parametrize("shape", SHAPES)
def test_fused_opener_has_the_bits_of_the_two_convolutions_and_meets_float64(shape):
    from playaid_core_amd import conv

    n, h, w, cin, cout = shape
    (x, w3, w1, b), (xp, w3p, w1p, w2, bd) = _device_case(shape, seed=h * 131 + cin)
    out, out2 = conv.conv2d_branch(xp, w3p, w2, cin, cout, bias=bd, out=_canvas(shape), out2=_canvas(shape), out_pad=1, act=1)
    ref_o = conv.conv2d(xp, w3p, cin, cout, 3, 2, in_pad=1, bias=bd, out=_canvas(shape), out_pad=1, act=1, compute_dtype="f32")
    ref_b = conv.conv2d(xp, w1p, cin, cout, 1, 2, in_pad=1, out=_canvas(shape), out_pad=1, act=0, compute_dtype="f32")
    torch.cuda.synchronize()
    out, out2, ref_o, ref_b = out.cpu(), out2.cpu(), ref_o.cpu(), ref_b.cpu()
    # bitwise, the untouched border (-3) included: nothing is written outside the interior
    assert np.array_equal(out.numpy().view(np.uint32), ref_o.numpy().view(np.uint32)), shape
    assert np.array_equal(out2.numpy().view(np.uint32), ref_b.numpy().view(np.uint32)), shape
    border = torch.ones_like(out, dtype=torch.bool)
    border[:, 1:-1, 1:-1, :] = False
    assert bool((out[border] == -3.0).all()) and bool((out2[border] == -3.0).all()), shape
    # float64
    xd = torch.from_numpy(x).double()
    f_o = F.relu(F.conv2d(xd, torch.from_numpy(w3).double(), torch.from_numpy(b).double(), stride=2, padding=1))
    f_b = F.conv2d(xd, torch.from_numpy(w1).double(), None, stride=2)
    for what, got, ref in (("opener", out, f_o), ("branch", out2, f_b)):
        inner = got[:, 1:-1, 1:-1, :].permute(0, 3, 1, 2).double()
        err = float((inner - ref).abs().max() / ref.abs().max())
        print(f"{shape} {what}: max|err| / max|ref| = {err:.3g}")
        assert err <= 2e-5, (shape, what, err)


@pytest.mark.gpu
def test_fused_opener_refuses_what_it_does_not_cover():
    """stride 1, a 1x1 convolution, a tap that is not the whole pixel (wider pixels than cin), another dtype: status, no launch."""
    from playaid_core_amd import conv

    shape = (2, 8, 8, 64, 64)
    n, h, w, cin, cout = shape
    _, (xp, w3p, w1p, w2, bd) = _device_case(shape, seed=3)
    ok = lambda **kw: conv.conv2d_branch(xp, w3p, w2, cin, cout, bias=bd, out_pad=1, act=1, **kw)
    ok()
    big = lambda: torch.zeros((n, h + 2, w + 2, cout), dtype=torch.float32, device="cuda:0")   # (large enough for every refused geometry)
    with pytest.raises(ValueError):
        ok(stride=1, out=big(), out2=big())
    with pytest.raises(ValueError):
        ok(ksize=1, out=big(), out2=big())
    with pytest.raises(ValueError):
        ok(compute_dtype="emulated_f32")
    wide = torch.zeros((n, h + 2, w + 2, 2 * cin), dtype=torch.float32, device="cuda:0")
    with pytest.raises(ValueError):
        conv.conv2d_branch(wide, w3p, w2, cin, cout, bias=bd, out_pad=1, act=1)
    with pytest.raises(ValueError):
        conv.conv2d_branch(xp, w3p, w2, cin, cout, bias=bd, out_pad=1, act=2)   # SiLU
    torch.cuda.synchronize()


@pytest.mark.gpu
def test_fused_opener_is_repeatable():
    from playaid_core_amd import conv

    shape = SHAPES[1]
    n, h, w, cin, cout = shape
    _, (xp, w3p, w1p, w2, bd) = _device_case(shape, seed=11)
    first = None
    for _ in range(20):
        out, out2 = conv.conv2d_branch(xp, w3p, w2, cin, cout, bias=bd, out_pad=1, act=1)
        torch.cuda.synchronize()
        got = (out.cpu().numpy().view(np.uint32), out2.cpu().numpy().view(np.uint32))
        if first is None:
            first = got
            assert got[0].any() and got[1].any()
        assert np.array_equal(got[0], first[0]) and np.array_equal(got[1], first[1])


def _trace(env_extra, path):
    env = dict(os.environ, **env_extra)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "opener_branch_worker.py"), path], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return np.load(path)


@pytest.mark.gpu
def test_engine_with_fused_openers_reproduces_the_separate_branch_gemms(tmp_path):
    """Default process against PA_F32_DS_FUSE=0 (fresh children: the knob is read once): the openers, the convolutions that add
    the branch, the stored branch and the features, bit for bit -- at 1 and 5 crops (the openers run split K there and launch the
    branch behind them) and at 128 crops (blocks 2 and 3 on the fused kernel). Block 4 keeps its launches, so its stages are
    held to the same."""
    fused = _trace({}, str(tmp_path / "fused.npz"))
    apart = _trace({"PA_F32_DS_FUSE": "0"}, str(tmp_path / "apart.npz"))
    assert sorted(fused.files) == sorted(apart.files)
    checked = 0
    for key in fused.files:
        if key.endswith("_nonzero"):
            assert float(fused[key]) > 0.05, f"{key}: mostly zero, the comparison would be idle"
            continue
        a, b = fused[key], apart[key]
        assert a.shape == b.shape and a.dtype == b.dtype, key
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8)), f"{key}: the fused opener changed bits"
        checked += 1
    # per batch: 7 stages + 3 stored branches, each as a digest; the small batches (and block 4 at 128 crops) also whole
    assert checked == 3 * 10 + 2 * 10 + 3, checked


def test_branch_kernel_store_count_matches_its_counted_waits():
    """The branch kernel's waits count NST = 8 sixteen-byte stores per tile and wave (four of ``out``, four of ``out2``) and four
    or six LDS-DMA copies per k-step (a centre-tap step brings the branch's weights): the built object must hold exactly the eight
    stores, and the copies of two prologue steps + three inlined loop issues (4 + 6 + 6 + 6)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    from test_abi import _device_disassembly   # (the disassembly of an in-tree object, as test_abi's own object checks read it)

    asm = _device_disassembly("pigemm.o")
    if asm is None:
        pytest.skip("no llvm-objdump / object in this environment")
    parts = re.split(r"\n[0-9a-f]+ <(_ZN2pa19pgemm_branch_kernel[^>]*)>:\n", asm)
    assert len(parts) == 3, [p[:80] for p in parts[1::2]]
    body = re.split(r"\n[0-9a-f]+ <[^>]+>:\n", parts[2])[0].split("s_endpgm")[0]
    assert len(re.findall(r"\bglobal_store_dwordx4\b", body)) == 8
    assert len(re.findall(r"\bbuffer_load_dwordx4\b[^\n]*\blds\b", body)) == 22
