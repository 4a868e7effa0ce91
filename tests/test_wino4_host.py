"""Winograd F(4x4, 3x3) taken apart (``csrc/wino4.hip``), host side only: the library's own filter transform and a numpy
restatement of the two device transforms -- the operation order ``w4_bt`` / ``w4_at`` document -- reproduce the direct 3x3
convolution in float64, and the filter image is ``U[36][cout][cin]``, the ``[N][K]`` image the grouped GEMM reads per position."""
import numpy as np

BT = np.array([[4, 0, -5, 0, 1, 0], [0, -4, -4, 1, 1, 0], [0, 4, -4, -1, 1, 0], [0, -2, -1, 2, 1, 0], [0, 2, -1, -2, 1, 0], [0, 4, 0, -5, 0, 1]],
              dtype=np.float64)
G = np.array([[1 / 4, 0, 0], [-1 / 6, -1 / 6, -1 / 6], [-1 / 6, 1 / 6, -1 / 6], [1 / 24, 1 / 12, 1 / 6], [1 / 24, -1 / 12, 1 / 6], [0, 0, 1]],
             dtype=np.float64)
AT = np.array([[1, 1, 1, 1, 1, 0], [0, 1, -1, 2, -2, 0], [0, 1, 1, 4, 4, 0], [0, 1, -1, 8, -8, 1]], dtype=np.float64)


def bt_line(d):
    """w4_bt: six values (leading axis) -> six, in the kernel's order."""
    a, b = d[4] - 4 * d[2], d[3] - 4 * d[1]
    c, e = d[4] - d[2], d[3] - d[1]
    return np.stack([4 * d[0] + (d[4] - 5 * d[2]), a + b, a - b, c + 2 * e, c - 2 * e, 4 * d[1] + (d[5] - 5 * d[3])])


def at_line(m):
    """w4_at: six values (leading axis) -> four, in the kernel's order."""
    s, d, u, v = m[1] + m[2], m[1] - m[2], m[3] + m[4], m[3] - m[4]
    return np.stack([(m[0] + s) + u, d + 2 * v, s + 4 * u, (d + 8 * v) + m[5]])


def input_transform(patch):
    """[6, 6, ...] -> B^T d B: along the columns (i) first, then along the rows (j), as wino4_input_kernel."""
    t = bt_line(patch)                                   # over i
    return np.moveaxis(bt_line(np.moveaxis(t, 1, 0)), 0, 1)   # over j


def output_transform(m):
    """[6, 6, ...] -> A^T M A, [4, 4, ...]: columns first, then rows, as wino4_output_kernel."""
    t = at_line(m)
    return np.moveaxis(at_line(np.moveaxis(t, 1, 0)), 0, 1)


def test_line_transforms_are_the_matrices():
    rng = np.random.default_rng(1)
    d = rng.standard_normal((6, 5))
    assert np.allclose(bt_line(d), BT @ d, rtol=0, atol=1e-13)
    assert np.allclose(at_line(d), AT @ d, rtol=0, atol=1e-13)
    p = rng.standard_normal((6, 6, 3))
    assert np.allclose(input_transform(p), np.einsum("ij,jkc,lk->ilc", BT, p, BT), rtol=0, atol=1e-12)
    assert np.allclose(output_transform(p), np.einsum("ij,jkc,lk->ilc", AT, p, AT), rtol=0, atol=1e-12)


def test_library_filter_transform_layout_and_values():
    from playaid_core_amd import wino

    rng = np.random.default_rng(2)
    for cin, cout in ((64, 64), (128, 64), (64, 128)):
        w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32)
        u = wino.transform_weights_f4(w)
        assert u.shape == (36, cout, cin) and u.dtype == np.float32
        # G g G^T in float64 in the transform's own order -- (G g) first, three-term sums left to right -- rounded once, at
        # position p = 6 i + j (sums of float32 values over 6 and 24 land near float32 rounding boundaries often enough that
        # another float64 order flips the last bit of some)
        g = w.astype(np.float64)
        tmp = [G[i, 0] * g[:, :, 0, :] + G[i, 1] * g[:, :, 1, :] + G[i, 2] * g[:, :, 2, :] for i in range(6)]
        ref = np.stack([tmp[i][:, :, 0] * G[j, 0] + tmp[i][:, :, 1] * G[j, 1] + tmp[i][:, :, 2] * G[j, 2] for i in range(6) for j in range(6)])
        assert np.array_equal(u, ref.astype(np.float32))
        assert np.abs(ref - np.einsum("ij,ocjk,lk->iloc", G, g, G).reshape(36, cout, cin)).max() <= 1e-15


def test_transform_rejects_bad_shapes():
    import ctypes

    from playaid_core_amd import _lib

    lib = _lib.load()
    assert lib.pa_wino4_weight_floats(64, 64) == 36 * 64 * 64
    assert lib.pa_wino4_weight_floats(32, 64) == 0 and lib.pa_wino4_weight_floats(64, 96) == 0 and lib.pa_wino4_weight_floats(0, 64) == 0
    buf = np.zeros(16, dtype=np.float32)
    p = buf.ctypes.data_as(ctypes.c_void_p)
    assert lib.pa_wino4_transform_weights(p, 32, 64, p) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_wino4_transform_weights(p, 64, 96, p) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_wino4_transform_weights(None, 64, 64, p) == _lib.PA_ERR_INVALID_ARG


def test_three_stages_equal_the_direct_convolution_in_float64():
    """A^T [(G g G^T) . (B^T d B)] A on random tiles, the products summed over cin in float64, against the direct convolution: 1e-12.
    The filter image is the library's (float32 values of float32 filters, so G g G^T is recomputed in float64 for the sum and the
    library's image is checked against it above)."""
    rng = np.random.default_rng(3)
    cin = cout = 64
    n = 3
    x = rng.standard_normal((n, cin, 4, 4))
    w = rng.standard_normal((cout, cin, 3, 3)).astype(np.float32).astype(np.float64)
    xp = np.zeros((n, cin, 6, 6))
    xp[:, :, 1:5, 1:5] = x
    u = np.einsum("ij,ocjk,lk->iloc", G, w, G)                      # [6][6][cout][cin]
    v = input_transform(np.ascontiguousarray(xp.transpose(2, 3, 0, 1)))   # [6][6][n][cin]
    m = np.einsum("ijnc,ijoc->ijno", v, u)                           # 36 independent products
    y = output_transform(m)                                          # [4][4][n][cout]
    ref = np.zeros((n, cout, 4, 4))
    for ky in range(3):
        for kx in range(3):
            ref += np.einsum("ncij,oc->noij", xp[:, :, ky:ky + 4, kx:kx + 4], w[:, :, ky, kx])
    err = np.abs(y.transpose(2, 3, 0, 1) - ref).max() / np.abs(ref).max()
    assert err <= 1e-12, err
