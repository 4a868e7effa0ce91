"""The Winograd F(2x2, 3x3) kernel's third unsplit workgroup shape (``csrc/wino.hip``, ``wino3x3_kernel<2, 2, 2>``: four waves as two
tile groups by two channel groups, 8 sub-blocks x 64 channels over the full K) through ``pa_wino_conv3x3_shape``. Per lane the
arithmetic is the eight-wave workgroup's -- same chunk order, same transform, same accumulators, same epilogue -- so the main test
is bit for bit against ``pa_wino_conv3x3`` (unsplit, no scratch) on the same inputs; against torch's CPU ``conv2d`` in float64 the
bar is the project's per-layer 2e-5 of the layer's largest output, as ``tests/test_wino.py`` uses."""
import ctypes
import itertools

import numpy as np
import pytest
import torch
import torch.nn.functional as F

RES_NONE, RES_BEFORE, RES_AFTER, RES_ALIAS = range(4)   # RES_ALIAS: before the activation, read from the output buffer itself


def _run_both(n, h, w, cin, cout, seed, bias=True, res=RES_NONE, act=0, in_extra=0, out_extra=0, out_pad=1):
    """One set of inputs through pa_wino_conv3x3 and through the 2 x 2 shape -> (eight-wave output, 2 x 2 output, float64 reference),
    outputs as the whole padded buffers (host)."""
    from playaid_core_amd import wino

    rng = np.random.default_rng(seed)
    dev = torch.device("cuda:0")
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32) if bias else None
    r = rng.standard_normal((n, cout, h, w)).astype(np.float32) if res != RES_NONE else None
    xp = torch.zeros((n, h + 2, w + 2, cin + in_extra), dtype=torch.float32)
    xp[:, 1:-1, 1:-1, :cin] = torch.from_numpy(x).permute(0, 2, 3, 1)
    if in_extra:
        xp[:, :, :, cin:] = 7.0   # channels of a wider buffer the kernel must not read
    out0 = torch.full((n, h + 2 * out_pad, w + 2 * out_pad, cout + out_extra), -3.0, dtype=torch.float32)
    inner = (slice(None), slice(out_pad, out_pad + h), slice(out_pad, out_pad + w), slice(0, cout))
    resp = None
    if res == RES_ALIAS:
        out0[inner] = torch.from_numpy(r).permute(0, 2, 3, 1)
    elif res != RES_NONE:
        resp = torch.zeros_like(out0)
        resp[inner] = torch.from_numpy(r).permute(0, 2, 3, 1)
        resp = resp.to(dev)
    ug = torch.from_numpy(wino.transform_weights(wt, bn=64)).to(dev)
    xd = xp.to(dev)
    bd = torch.from_numpy(b).to(dev) if bias else None
    got = []
    for shape in (None, wino.WG_2X2):
        o = out0.to(dev)
        wino.conv3x3(xd, ug, cin, cout, bias=bd, residual=o if res == RES_ALIAS else resp, out=o, out_pad=out_pad, act=act,
                     res_after=res == RES_AFTER, bn=64, shape=shape)
        got.append(o.cpu())
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double() if bias else None, padding=1)
    if res in (RES_BEFORE, RES_ALIAS):
        ref = ref + torch.from_numpy(r).double()
    ref = F.relu(ref) if act == 1 else F.silu(ref) if act == 2 else ref
    if res == RES_AFTER:
        ref = ref + torch.from_numpy(r).double()
    # nothing outside the interior / the layer's channels is written
    mask = torch.ones_like(out0, dtype=torch.bool)
    mask[inner] = False
    for g in got:
        assert bool((g[mask] == -3.0).all()), "the kernel wrote outside its output"
    return got[0], got[1], (ref, inner)


def _rel_err(got, ref_inner):
    ref, inner = ref_inner
    return float((got[inner].permute(0, 3, 1, 2).double() - ref).abs().max() / ref.abs().max())


@pytest.mark.gpu
@pytest.mark.parametrize("hw", [(8, 8), (4, 4), (16, 8)], ids=lambda m: f"{m[0]}x{m[1]}")
def test_2x2_shape_is_bit_identical_to_the_eight_wave_shape(hw):
    """Crops 1 (a half-empty workgroup on 8 x 8), 3 (12 sub-blocks on 8 x 8: a partial last workgroup) and 5; cin 8 (one chunk), 16 (the
    ring wraps once) and 72 (an odd chunk count); cout 64 and 128 -- every combination, the epilogue cycling through bias / no bias x
    no residual / before / after the activation / aliasing the output, the activation through none / ReLU / SiLU, and every third case
    reading from, every other third writing into, a channel slice of a wider buffer."""
    h, w = hw
    seen = set()
    for idx, (n, cin, cout) in enumerate(itertools.product((1, 3, 5), (8, 16, 72), (64, 128))):
        bias, res = idx % 2 == 0, (idx // 2) % 4
        a, b, _ = _run_both(n, h, w, cin, cout, seed=1000 * h + 10 * idx + w, bias=bias, res=res, act=idx % 3,
                            in_extra=8 if idx % 3 == 0 else 0, out_extra=64 if idx % 3 == 1 else 0)
        assert a[..., :cout].abs().max() > 0
        assert torch.equal(a, b), (hw, n, cin, cout, bias, res, float((a - b).abs().max()))
        seen.add((bias, res))
    assert len(seen) == 8


@pytest.mark.gpu
@pytest.mark.parametrize("res,act", [(RES_BEFORE, 1), (RES_AFTER, 2)], ids=["residual_before_relu", "residual_after_silu"])
def test_2x2_shape_matches_conv2d(res, act):
    _, got, ref = _run_both(3, 8, 8, 72, 128, seed=77 + res, bias=True, res=res, act=act)
    err = _rel_err(got, ref)
    assert err <= 2e-5, err


@pytest.mark.gpu
def test_2x2_shape_is_repeatable_and_batch_independent():
    """Twenty launches of one shape give the same bits, and a crop alone has the bits it has inside a batch of five: the shape never
    splits K, so a crop's sum does not depend on the batch."""
    from playaid_core_amd import wino

    rng = np.random.default_rng(5)
    dev = torch.device("cuda:0")
    n, hw, cin, cout = 5, 8, 72, 128
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    xp = torch.zeros((n, hw + 2, hw + 2, cin), dtype=torch.float32)
    xp[:, 1:-1, 1:-1] = torch.from_numpy(rng.standard_normal((n, hw, hw, cin)).astype(np.float32))
    ug = torch.from_numpy(wino.transform_weights(wt, bn=64)).to(dev)
    bd = torch.from_numpy(rng.standard_normal(cout).astype(np.float32)).to(dev)
    xd = xp.to(dev)
    first = wino.conv3x3(xd, ug, cin, cout, bias=bd, act=1, bn=64, shape=wino.WG_2X2).cpu()
    for _ in range(19):
        assert torch.equal(wino.conv3x3(xd, ug, cin, cout, bias=bd, act=1, bn=64, shape=wino.WG_2X2).cpu(), first)
    for i in (0, 2, 4):
        alone = wino.conv3x3(xd[i:i + 1].contiguous(), ug, cin, cout, bias=bd, act=1, bn=64, shape=wino.WG_2X2).cpu()
        assert alone.abs().max() > 0 and torch.equal(alone[0], first[i]), i


def test_shape_entry_refusals():
    """An unknown shape value, the 2 x 2 shape on the 32-channel filter layout, misaligned pointers and maps whose sides are not
    multiples of 4: PA_ERR_INVALID_ARG before any launch (non-null addresses that are never dereferenced, as tests/test_abi.py
    reaches the launchers' host checks)."""
    from playaid_core_amd import _lib

    lib = _lib.load()
    z, a16, a4 = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    bad = _lib.PA_ERR_INVALID_ARG

    def call(x=a16, ug=a16, bias=z, res=z, out=a16, h=8, w=8, cin=8, cout=64, bn=64, shape=1):
        return lib.pa_wino_conv3x3_shape(x, ug, bias, res, out, 1, h, w, cin, cout, bn, cin, cout, 1, 0, 0, shape, z)

    for shape in (2, 3, -1, 64):
        assert call(shape=shape) == bad, shape
    assert call(bn=32) == bad
    assert call(bn=32, cout=32) == bad
    assert call(bn=48) == bad
    for name in ("x", "ug", "out", "bias", "res"):
        assert call(**{name: a4}) == bad, name
        assert call(**{name: a4}, shape=0) == bad, name
    assert call(x=z) == bad and call(ug=z) == bad and call(out=z) == bad
    for h, w in ((6, 8), (8, 6), (2, 8), (8, 10)):
        assert call(h=h, w=w) == bad, (h, w)
        assert call(h=h, w=w, shape=0) == bad, (h, w)
