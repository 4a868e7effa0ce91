"""Every row of a ResNet-50 table of another input size than 128 (a kind-3 stem row, ``stem_pool_any.hip``; maps of
crop_size / 4, / 8, / 16, / 32 on the launchers the 128 table runs on) against float64, one row at a time. Walk, bars and
checks: tests/helpers/convnet_layers_sized.py (those of tests/helpers/convnet_layers.py).

Sizes: 64 (a stem row of 32 pixels: one partial column tile; maps 16, 8, 4, 2), 96 (48 pixels: a partial tile that is not a
power of two; maps 24, 12, 6, 3 -- the widths no tile divides) with n = 1 and 5 of 8 crops, and 256 (128 pixels: two column
tiles, the seam between them; maps 64, 32, 16, 8) with 2 of 2. The form of every row is compared with the written-down table
(``expected_forms``), the set of forms with the literal sets below.
"""
import pytest
import torch

from helpers import convnet_layers_sized as cls_

# the forms of the three tables under test: at these crop counts no implicit-GEMM row has the 512 tiles the
# 128-pixel tiles ask for; 2 x 2, 3 x 3 and 6 x 6 maps are taken by neither Winograd nor the patch kernel; psgemm has its 128 tiles
# only on the 64 x 64 maps' 256-channel rows of the 256 table
FORMS = {
    (64, "f32"): {"stem_pool_any", "wino", "patch", "igemm_64x64", "avgpool"},
    (64, "emulated_f32"): {"stem_pool_any", "wino", "patch", "igemm_64x64", "avgpool"},
    (96, "f32"): {"stem_pool_any", "wino", "igemm_64x64", "avgpool"},
    (96, "emulated_f32"): {"stem_pool_any", "wino", "igemm_64x64", "avgpool"},
    (256, "f32"): {"stem_pool_any", "wino", "igemm_64x64", "avgpool"},
    (256, "emulated_f32"): {"stem_pool_any", "wino", "psgemm", "igemm_64x64", "avgpool"},
}


@pytest.fixture(scope="module")
def rf_sd():
    from playaid_core_amd import synth

    return synth.make_resformer_state_dict(seed=2468)


@pytest.mark.gpu
@pytest.mark.parametrize("crop_size, max_crops, ns", [(64, 8, (1, 5)), (96, 8, (1, 5)), (256, 2, (2,))], ids=["64", "96", "256"])
@pytest.mark.parametrize("dtype", ["f32", "emulated_f32"])
def test_sized_convnet_rows_against_float64(rf_sd, dtype, crop_size, max_crops, ns):
    from playaid_core_amd.resnet_transformer_detector import ConvNet, build_resnet50_table

    descs, bufs, weights, dim = build_resnet50_table(rf_sd, crop_size=crop_size)
    for n in ns:
        net = ConvNet(descs, bufs, weights, dim, max_crops=max_crops, compute_dtype=dtype)
        try:
            assert net.in_hw == crop_size
            r = cls_.check_table(net, descs, weights, n, 7, f"{crop_size} {dtype} n={n}/{max_crops}")
            # trace(-1) returns the [S + 6]^2 x 4 input exactly (checked inside the walk against x; here: its size)
            assert net.trace(r["x"], -1, -1).numel() == max_crops * (crop_size + 6) ** 2 * 4
            with pytest.raises(ValueError):
                net.forward(torch.zeros((1, 3, 128, 128)))      # the table takes crop_size x crop_size crops
        finally:
            net.close()
        forms = r["forms"]
        print(f"{crop_size} {dtype} n={n}/{max_crops} forms: {sorted(set(forms))}")
        assert forms[0] == "stem_pool_any" and forms[-1] == "avgpool"
        want = cls_.expected_forms(descs, n, max_crops, dtype)
        assert forms == want, [(i, a, b) for i, (a, b) in enumerate(zip(forms, want)) if a != b]
        assert set(forms) == FORMS[(crop_size, dtype)]


@pytest.mark.gpu
def test_sized_forward_is_the_traced_last_row_and_repeats(rf_sd):
    """``forward`` in groups of max_crops (5 crops on a handle of 2) equals crop-by-crop calls, bit for bit, twice."""
    import numpy as np

    from playaid_core_amd.resnet_transformer_detector import ConvNet, build_resnet50_table

    descs, bufs, weights, dim = build_resnet50_table(rf_sd, crop_size=96)
    net = ConvNet(descs, bufs, weights, dim, max_crops=2)
    try:
        rng = np.random.default_rng(3)
        x = torch.from_numpy(rng.integers(0, 256, (5, 3, 96, 96)).astype(np.float32) / np.float32(255)).cuda()
        a = net.forward(x)
        b = net.forward(x)
        one = torch.cat([net.forward(x[i:i + 1]) for i in range(5)])
        assert a.shape == (5, 2048) and torch.equal(a, b)
        assert torch.equal(a, one)
    finally:
        net.close()
