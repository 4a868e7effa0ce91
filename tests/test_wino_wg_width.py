"""The Winograd F(2x2, 3x3) kernel's launch width beside the filter layout (``csrc/wino.hip``, ``WinoParams::wg``, through
``pa_wino_conv3x3_wg``): width 32 on a 64-channel layout runs four-wave workgroups of 16 sub-blocks x 32 channels (``wino3x3_kernel<4, 1,
2, ABL, true>``), each copying its half of the 64-channel filter images. Per lane the arithmetic is the eight-wave workgroup's -- the
same chunk order, transform, accumulators and epilogue on the same values -- so the main test is bit for bit against the eight-wave
form (``wg=64``) on the same buffers; against torch's CPU ``conv2d`` in float64 the bar is ``tests/test_wino.py``'s own: 2e-5 of the
layer's largest output.

Shapes, the smallest that can still go wrong: 64 -> 64 on an 8 x 8 map with 1, 3 and 5 crops (4, 12 and 20 sub-blocks: a partial
workgroup alone, a full one plus a partial one; two workgroups per pixel tile, the lower and the upper half of one filter image);
64 -> 128 and 128 -> 128 on a 4 x 4 map with 5 crops (halves of more than one 64-channel group; 16 chunks: the ring wraps); 64 -> 64
on a 16 x 16 map with 2 crops (two full pixel tiles)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

SHAPES = [(1, 8, 8, 64, 64), (3, 8, 8, 64, 64), (5, 8, 8, 64, 64), (5, 4, 4, 64, 128), (5, 4, 4, 128, 128), (2, 16, 16, 64, 64)]
# (name, residual: None | "before" | "after", output channels beyond the layer's in a wider buffer)
EPILOGUES = [("bias_relu", None, 0), ("residual_before", "before", 0), ("residual_after", "after", 0), ("channel_slice", None, 64)]
TOL = 2e-5   # tests/test_wino.py: of the layer's largest output


def _ids(v):
    return "n{}_{}x{}_{}to{}".format(*v) if len(v) == 5 else v[0]


def _inputs(n, h, w, cin, cout, seed, res, out_extra):
    rng = np.random.default_rng(seed)
    x = rng.standard_normal((n, cin, h, w)).astype(np.float32)
    wt = (rng.standard_normal((cout, cin, 3, 3)) / np.sqrt(9 * cin)).astype(np.float32)
    b = rng.standard_normal(cout).astype(np.float32)
    r = rng.standard_normal((n, cout, h, w)).astype(np.float32) if res else None
    xp = torch.zeros((n, h + 2, w + 2, cin), dtype=torch.float32)
    xp[:, 1:-1, 1:-1] = torch.from_numpy(x).permute(0, 2, 3, 1)
    out0 = torch.full((n, h + 2, w + 2, cout + out_extra), -3.0, dtype=torch.float32)
    inner = (slice(None), slice(1, 1 + h), slice(1, 1 + w), slice(0, cout))
    resp = None
    if res:
        resp = torch.zeros_like(out0)
        resp[inner] = torch.from_numpy(r).permute(0, 2, 3, 1)
    ref = F.conv2d(torch.from_numpy(x).double(), torch.from_numpy(wt).double(), torch.from_numpy(b).double(), padding=1)
    if res == "before":
        ref = ref + torch.from_numpy(r).double()
    ref = F.relu(ref)
    if res == "after":
        ref = ref + torch.from_numpy(r).double()
    return xp, wt, b, resp, out0, inner, ref


@pytest.mark.gpu
@pytest.mark.parametrize("epi", EPILOGUES, ids=_ids)
@pytest.mark.parametrize("shape", SHAPES, ids=_ids)
def test_width_32_on_the_64_channel_layout_is_the_eight_wave_result(shape, epi):
    from playaid_core_amd import wino

    n, h, w, cin, cout = shape
    _, res, out_extra = epi
    xp, wt, b, resp, out0, inner, ref = _inputs(n, h, w, cin, cout, 100 * h + 10 * n + cout + len(epi[0]), res, out_extra)
    dev = torch.device("cuda:0")
    ug = torch.from_numpy(wino.transform_weights(wt, bn=64)).to(dev)
    xd, bd = xp.to(dev), torch.from_numpy(b).to(dev)
    rd = resp.to(dev) if resp is not None else None
    got = {}
    for key, wg in (("wide", 64), ("narrow", 32), ("again", 32)):
        o = out0.to(dev)
        wino.conv3x3(xd, ug, cin, cout, bias=bd, residual=rd, out=o, act=1, res_after=res == "after", bn=64, wg=wg)
        got[key] = o.cpu()
    mask = torch.ones_like(out0, dtype=torch.bool)
    mask[inner] = False
    for key, g in got.items():
        assert bool((g[mask] == -3.0).all()), f"{key}: the kernel wrote outside its output"
        err = float((g[inner].permute(0, 3, 1, 2).double() - ref).abs().max() / ref.abs().max())
        print(f"{key}: max|err| = {err:.3e} of the largest output (bar {TOL})")
        assert err <= TOL, (key, err)
    assert got["wide"][inner].abs().max() > 0
    assert torch.equal(got["narrow"], got["wide"]), float((got["narrow"] - got["wide"]).abs().max())
    assert torch.equal(got["again"], got["narrow"]), "width 32 is not bitwise repeatable"


@pytest.mark.gpu
def test_width_64_is_the_plain_launch():
    """wg = 64 is what pa_wino_conv3x3 launches on the 64-channel layout, and pa_wino_conv3x3_splitk with scratch."""
    from playaid_core_amd import wino

    n, h, w, cin, cout = 3, 8, 8, 128, 64
    xp, wt, b, _, _, _, _ = _inputs(n, h, w, cin, cout, 5, None, 0)
    dev = torch.device("cuda:0")
    xd, bd = xp.to(dev), torch.from_numpy(b).to(dev)
    ug = torch.from_numpy(wino.transform_weights(wt, bn=64)).to(dev)
    plain = wino.conv3x3(xd, ug, cin, cout, bias=bd, act=1, bn=64).cpu()
    assert plain.abs().max() > 0
    assert torch.equal(wino.conv3x3(xd, ug, cin, cout, bias=bd, act=1, bn=64, wg=64).cpu(), plain)
    sk = wino.SplitKScratch(dev, slab_floats=1 << 20, n_tickets=64)
    split = wino.conv3x3(xd, ug, cin, cout, bias=bd, act=1, bn=64, split_k=sk).cpu()   # 16 chunks: two splits
    assert torch.equal(wino.conv3x3(xd, ug, cin, cout, bias=bd, act=1, bn=64, wg=64, split_k=sk).cpu(), split)


@pytest.mark.gpu
def test_refusals_leave_the_output_untouched():
    """Width 32 with split-K scratch; width 32 on a 32-channel layout; cout not a multiple of 64 (96: no whole 64-channel groups to
    halve); width 64 on a 32-channel layout; a width other than 32 or 64."""
    from playaid_core_amd import wino

    n, h, w, cin = 2, 8, 8, 64
    dev = torch.device("cuda:0")
    sk = wino.SplitKScratch(dev, slab_floats=1 << 20, n_tickets=64)
    for cout, bn, wg, split in ((64, 64, 32, sk), (64, 32, 32, None), (96, 64, 32, None), (96, 32, 32, None), (96, 64, 64, None),
                                (64, 32, 64, None), (64, 64, 16, None), (64, 64, 0, None), (64, 48, 32, None)):
        xp, wt, b, _, out0, _, _ = _inputs(n, h, w, cin, cout, 7, None, 0)
        ug = torch.from_numpy(wino.transform_weights(wt, bn=32 if bn != 64 or cout % 64 else 64)).to(dev)
        o = out0.to(dev)
        with pytest.raises(ValueError):
            wino.conv3x3(xp.to(dev), ug, cin, cout, bias=torch.from_numpy(b).to(dev), out=o, act=1, bn=bn, wg=wg, split_k=split)
        torch.cuda.synchronize()
        assert bool((o.cpu() == -3.0).all()), (cout, bn, wg)
        assert int(sk.tickets.abs().sum()) == 0


def test_refusals_need_no_launch():
    """The same refusals through the C entry point with addresses that are never dereferenced, as tests/test_abi.py reaches the
    launchers' host checks: PA_ERR_INVALID_ARG before any launch."""
    import ctypes

    from playaid_core_amd import _lib

    lib = _lib.load()
    z, a16, a4 = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    bad = _lib.PA_ERR_INVALID_ARG

    def call(cout=64, bn=64, wg=32, slab=z, nf=0, tk=z, nt=0, ug=a16):
        return lib.pa_wino_conv3x3_wg(a16, ug, z, z, a16, 1, 8, 8, 8, cout, bn, 8, cout, 1, 0, 0, wg, slab, nf, tk, nt, z)

    assert call(slab=a16, nf=1 << 20, tk=a16, nt=64) == bad          # width 32 with split-K scratch
    assert call(slab=a16, nf=1 << 20) == bad and call(tk=a16, nt=64) == bad and call(slab=a4, nf=1 << 20, tk=a16, nt=64) == bad
    assert call(cout=96) == bad and call(cout=96, wg=64) == bad and call(cout=32) == bad   # no whole 64-channel groups
    assert call(bn=32, wg=32) == bad and call(bn=32, wg=64) == bad   # a width is named beside the 64-channel layout only
    for wg in (0, 16, 48, 128, -32):
        assert call(wg=wg) == bad, wg
    assert call(ug=a4) == bad and call(ug=z) == bad
