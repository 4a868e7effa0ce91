"""Crops and ResNet-50 tables of any size, the parts that need no GPU: the table ``build_resnet50_table(crop_size=...)`` builds
(at 128 exactly the table it always built; at other sizes a kind-3 stem row and maps of crop_size / 4, / 8, / 16, / 32), the
refused sizes, and the header / binding / export agreement of what the feature appends at ABI 15."""
import os
import re

import numpy as np
import pytest

from playaid_core_amd import synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def rf_sd():
    return synth.make_resformer_state_dict(seed=2468)


def test_table_at_128_is_the_table_without_the_argument(rf_sd):
    from playaid_core_amd.resnet_transformer_detector import build_resnet50_table

    a = build_resnet50_table(rf_sd)
    b = build_resnet50_table(rf_sd, crop_size=128)
    assert a[0] == b[0]                      # every row, field by field
    assert a[0][0]["kind"] == 1 and a[0][0]["in_hw"] == 128
    assert a[1] == b[1] and a[3] == b[3] == 2048
    assert a[1][:5] == [34 * 34 * 64, 32 * 32 * 256, 32 * 32 * 256, 32 * 32 * 64, 32 * 32 * 256]
    assert a[2].dtype == b[2].dtype == np.float32 and a[2].tobytes() == b[2].tobytes()


@pytest.mark.parametrize("crop_size", [64, 96, 160, 256, 512])
def test_table_geometry_at_other_sizes(rf_sd, crop_size):
    from playaid_core_amd.resnet_transformer_detector import RESNET50_BLOCKS, build_resnet50_table

    descs, bufs, weights, dim = build_resnet50_table(rf_sd, crop_size=crop_size)
    ref = build_resnet50_table(rf_sd)
    assert dim == 2048 and len(descs) == len(ref[0])
    assert weights.tobytes() == ref[2].tobytes()          # the blob does not depend on the size
    q = crop_size // 4
    d0 = descs[0]
    assert d0["kind"] == 3 and d0["in_hw"] == crop_size and d0["in_pad"] == 3 and d0["out_pad"] == 1 and (d0["cin"], d0["cout"]) == (3, 64)
    assert bufs[d0["out_buf"]] == (q + 2) * (q + 2) * 64
    assert all(d["kind"] == 0 for d in descs[1:-1]) and descs[-1]["kind"] == 2
    # every row but the stem's is the 128 table's row at another map size
    for d, r in zip(descs[1:], ref[0][1:]):
        assert {k: v for k, v in d.items() if k != "in_hw"} == {k: v for k, v in r.items() if k != "in_hw"}
        assert d["in_hw"] * 128 == r["in_hw"] * crop_size
    # the chain: layer l's blocks read maps of crop_size / 4, / 8, / 16, / 32 (its first block the map above when it strides)
    i = 1
    for li, blocks in enumerate(RESNET50_BLOCKS):
        hw = q >> li
        for b in range(blocks):
            first_strided = b == 0 and li > 0
            n_rows = 4 if b == 0 else 3
            rows = descs[i:i + n_rows]
            i += n_rows
            above = hw * 2 if first_strided else hw
            assert rows[0]["in_hw"] == above and rows[1]["in_hw"] == above and rows[1]["stride"] == (2 if first_strided else 1)
            assert rows[-1]["in_hw"] == hw and rows[-1]["ksize"] == 1          # conv3 on the block's output map
            if b == 0:
                assert rows[2]["in_hw"] == above and rows[2]["stride"] == rows[1]["stride"]   # the downsample branch
    assert i == len(descs) - 1
    assert descs[-1]["in_hw"] == crop_size // 32 and descs[-1]["cin"] == 2048 and bufs[descs[-1]["out_buf"]] == 2048
    # buffers: bordered ones hold (hw + 2)^2 * c, the others at least hw^2 * c of every row that uses them
    for d in descs[1:-1]:
        ohw = d["in_hw"] // d["stride"]
        need_in = (d["in_hw"] + 2 * d["in_pad"]) ** 2 * d["cin"]
        need_out = (ohw + 2 * d["out_pad"]) ** 2 * d["cout"]
        assert bufs[d["in_buf"]] == need_in if d["in_pad"] else bufs[d["in_buf"]] >= need_in
        assert bufs[d["out_buf"]] == need_out if d["out_pad"] else bufs[d["out_buf"]] >= need_out
        if d["ksize"] == 3:
            assert d["in_pad"] == 1
    assert bufs[1] == bufs[2] == bufs[4] == q * q * 256 and bufs[3] == q * q * 64


@pytest.mark.parametrize("crop_size", [100, 32, 544, 0, 96.5])
def test_table_refuses_other_sizes(rf_sd, crop_size):
    from playaid_core_amd.resnet_transformer_detector import build_resnet50_table

    with pytest.raises(ValueError, match="multiple of 32 in 64..512"):
        build_resnet50_table(rf_sd, crop_size=crop_size)


def test_header_binding_and_exports_agree():
    import ctypes

    from playaid_core_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "playaid_hip.h")).read()
    assert re.search(r"#define\s+PA_ABI_VERSION\s+15\b", hdr) and _lib.PA_ABI_VERSION == 15
    # the sized crop entry point: declared with twelve arguments, bound with twelve, exported
    decl = re.search(r"\bint\s+pa_square_crops_sized\s*\(([^)]*)\)\s*;", hdr)
    assert decl and len(decl.group(1).split(",")) == 12
    bound = {name: args for name, _, args in _lib.SYMBOLS}
    assert len(bound["pa_square_crops_sized"]) == 12
    assert bound["pa_square_crops_sized"][8] is ctypes.c_int32     # output_size, ahead of the crops pointer
    lo, hi = (int(re.search(r"#define\s+%s\s+(\d+)" % n, hdr).group(1)) for n in ("PA_CROP_SIZE_MIN", "PA_CROP_SIZE_MAX"))
    assert (lo, hi) == (_lib.PA_CROP_SIZE_MIN, _lib.PA_CROP_SIZE_MAX) == (16, 512)
    # the new form value, beside the enumeration whose list the ABI-15 tests pin
    assert int(re.search(r"#define\s+PA_CN_FORM_STEM_POOL_ANY\s+(\d+)", hdr).group(1)) == _lib.PA_CN_FORM_STEM_POOL_ANY == 12
    assert _lib.CN_FORM_NAMES[:12] == _lib.CN_FORMS and _lib.CN_FORM_NAMES[12] == "stem_pool_any" and len(_lib.CN_FORM_NAMES) == 13
    lib = _lib.load()
    assert lib.pa_abi_version() == 15
    assert lib.pa_square_crops_sized.argtypes == bound["pa_square_crops_sized"]
    # without an engine the call refuses before anything else (no GPU needed)
    assert lib.pa_square_crops_sized(None, None, 1, 8, 8, None, 0, 0, 64, None, None, None) == _lib.PA_ERR_INVALID_ARG


def test_create_refuses_bad_sized_stem_rows_without_gpu(rf_sd):
    """pa_convnet_create* validates a kind-3 row before it touches the device and names the row."""
    import ctypes as C

    from playaid_core_amd import _lib
    from playaid_core_amd.resnet_transformer_detector import build_resnet50_table

    lib = _lib.load()
    descs, bufs, weights, _ = build_resnet50_table(rf_sd, crop_size=96)

    def create(rows, dtype=_lib.PA_DTYPE_F32, buf_floats=bufs):
        arr = (_lib.pa_conv_desc * len(rows))()
        for i, d in enumerate(rows):
            for k, v in d.items():
                setattr(arr[i], k, int(v))
        b = (C.c_int64 * len(buf_floats))(*buf_floats)
        h = C.c_void_p()
        rc = lib.pa_convnet_create_dtype(0, arr, len(rows), b, len(buf_floats), weights.ctypes.data_as(C.c_void_p), weights.size, 2, dtype, C.byref(h))
        msg = lib.pa_convnet_last_error(h).decode() if h else ""
        lib.pa_convnet_destroy(h)
        return rc, msg

    for bad, word in ((dict(in_hw=100), "multiple of 32"), (dict(in_hw=32), "multiple of 32"), (dict(in_hw=544), "multiple of 32"),
                      (dict(out_pad=0), "out_pad 1"), (dict(w_off=weights.size - 100), "weights outside the blob")):
        rc, msg = create([dict(descs[0], **bad)] + descs[1:])
        assert rc in (_lib.PA_ERR_INVALID_ARG, _lib.PA_ERR_BAD_WEIGHTS) and msg.startswith("layer 0") and word in msg, (bad, rc, msg)
    rc, msg = create(descs, dtype=_lib.PA_DTYPE_BF16)
    assert rc == _lib.PA_ERR_INVALID_ARG and "layer 0" in msg and "bf16" in msg
    small = list(bufs)
    small[descs[0]["out_buf"]] -= 1
    rc, msg = create(descs, buf_floats=small)
    assert rc == _lib.PA_ERR_INVALID_ARG and "layer 0" in msg and "too small" in msg
    rc, msg = create([descs[0], descs[0]] + descs[1:])
    assert rc == _lib.PA_ERR_INVALID_ARG and "layer 1" in msg and "one stem row" in msg


def test_python_interfaces_refuse_bad_sizes_without_gpu():
    from playaid_core_amd.engine import Engine
    from playaid_core_amd.fighter import YoloCrop

    for bad in (8, 600, 15, 513, 64.5):
        with pytest.raises(ValueError):
            Engine._crop_size(bad)
        with pytest.raises(ValueError, match="16..512"):
            YoloCrop(0.5, 0.5, 0.2, 0.2).square_crop(np.zeros((64, 64, 3), np.uint8), output_size=bad)
    assert Engine._crop_size(16) == 16 and Engine._crop_size(512) == 512 and Engine._crop_size(128) == 128
