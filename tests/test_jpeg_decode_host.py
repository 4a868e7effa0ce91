"""The host half of the mixed-size JPEG decoder (no GPU): pa_jpegdec_plan on files written by live libjpeg-turbo behind
Pillow -- sizes, offsets, the block count -- the files it refuses, the argument checks of the new C ABI entries."""
import ctypes
import io
import os
import re

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from playaid_core_amd import _build, _lib

    _build.build()
    return _lib.load()


def pil_jpeg(rgb, quality=95, subsampling=0, **kw):
    from PIL import Image

    b = io.BytesIO()
    if rgb.ndim == 3:
        kw["subsampling"] = subsampling
    Image.fromarray(rgb).save(b, format="JPEG", quality=quality, **kw)
    return b.getvalue()


# (height, width, Pillow subsampling, (h, v) sampling factors of the luma component; chroma is 1 x 1)
CASES = [(1, 1, 0, (1, 1)), (7, 9, 0, (1, 1)), (16, 16, 1, (2, 1)), (37, 301, 0, (1, 1)), (128, 128, 2, (2, 2))]


def expected_blocks(h, w, hs, vs):
    """All components' 8x8 blocks padded to whole MCUs, from the sampling factors alone."""
    mcus = (-(-w // (8 * hs))) * (-(-h // (8 * vs)))
    return mcus * (hs * vs + 2)


def _plan(lib, blobs):
    from playaid_core_amd import _lib

    n = len(blobs)
    spans = np.zeros((n, 2), np.int64)
    off = 7   # the files need not start at the buffer's first byte
    parts = [b"\x00" * off]
    for i, b in enumerate(blobs):
        spans[i] = (off, off + len(b))
        parts.append(b)
        off += len(b)
    data = np.frombuffer(b"".join(parts), np.uint8)
    desc = (_lib.pa_crop_image * n)()
    total, blocks = ctypes.c_size_t(0), ctypes.c_int64(0)
    why = ctypes.create_string_buffer(256)
    rc = lib.pa_jpegdec_plan(data.ctypes.data_as(ctypes.c_void_p), spans.ctypes.data_as(ctypes.c_void_p), n, desc,
                             ctypes.byref(total), ctypes.byref(blocks), why, 256)
    return rc, desc, total.value, blocks.value, why.value.decode()


def test_plan_sizes_offsets_and_blocks(lib):
    from playaid_core_amd import _lib

    rng = np.random.default_rng(11)
    blobs, want_hw, want_blocks = [], [], 0
    for h, w, sub, (hs, vs) in CASES:
        blobs.append(pil_jpeg(rng.integers(0, 256, (h, w, 3), dtype=np.uint8), 95, sub))
        want_hw.append((h, w))
        want_blocks += expected_blocks(h, w, hs, vs)
    blobs.insert(2, b"")   # no file for this entry
    want_hw.insert(2, (0, 0))
    # a grey file: one component, 8 x 8 MCUs
    blobs.append(pil_jpeg(rng.integers(0, 256, (9, 17), dtype=np.uint8), 90))
    want_hw.append((9, 17))
    want_blocks += 2 * 3
    rc, desc, total, blocks, why = _plan(lib, blobs)
    assert rc == _lib.PA_OK, why
    off = 0
    for i, (h, w) in enumerate(want_hw):
        assert (desc[i].height, desc[i].width, desc[i].offset) == (h, w, off), i
        assert desc[i].offset % 16 == 0
        off += (h * w * 3 + 15) & ~15
    assert total == off
    assert blocks == want_blocks
    # the Python wrapper gives the same table
    from playaid_core_amd import jpeg_decode

    d2, t2, b2 = jpeg_decode.plan([b or None for b in blobs])
    assert (t2, b2) == (total, blocks)
    assert d2[:, 0].tolist() == [desc[i].offset for i in range(len(blobs))]
    assert (d2[:, 1] & 0xFFFFFFFF).tolist() == [h for h, _ in want_hw] and (d2[:, 1] >> 32).tolist() == [w for _, w in want_hw]
    assert all(jpeg_decode.blocks_bound(h, w) >= expected_blocks(h, w, hs, vs) for h, w, _, (hs, vs) in CASES)


def test_plan_refuses_what_is_not_baseline_and_names_the_image(lib):
    from playaid_core_amd import _lib, jpeg_decode

    rng = np.random.default_rng(12)
    good = pil_jpeg(rng.integers(0, 256, (24, 40, 3), dtype=np.uint8))
    progressive = pil_jpeg(rng.integers(0, 256, (24, 40, 3), dtype=np.uint8), progressive=True)
    cut = good[:100]
    rc, _, _, _, why = _plan(lib, [good, good, progressive])
    assert rc == _lib.PA_ERR_INVALID_ARG and "image 2" in why and "progressive" in why, why
    rc, _, _, _, why = _plan(lib, [good, cut, good])
    assert rc == _lib.PA_ERR_INVALID_ARG and "image 1" in why and "truncated" in why, why
    cmyk = io.BytesIO()
    from PIL import Image

    Image.fromarray(rng.integers(0, 256, (8, 8, 4), dtype=np.uint8), "CMYK").save(cmyk, format="JPEG")
    rc, _, _, _, why = _plan(lib, [cmyk.getvalue()])
    assert rc == _lib.PA_ERR_INVALID_ARG and "image 0" in why, why
    with pytest.raises(ValueError, match="image 1"):
        jpeg_decode.plan([good, cut])


def test_argument_checks_without_a_gpu(lib):
    from playaid_core_amd import _lib

    bad = _lib.PA_ERR_INVALID_ARG
    z, x = ctypes.c_void_p(0), ctypes.c_void_p(4096)   # never dereferenced: every call below is refused first
    why = ctypes.create_string_buffer(64)
    assert lib.pa_jpegdec_plan(z, x, 1, z, None, None, why, 64) == bad
    assert lib.pa_jpegdec_plan(x, z, 1, z, None, None, why, 64) == bad
    assert lib.pa_jpegdec_plan(x, x, 0, z, None, None, why, 64) == bad
    h = ctypes.c_void_p(0)
    assert lib.pa_jpegdec_create(0, 0, 1024, 1 << 20, ctypes.byref(h)) == bad and not h
    assert lib.pa_jpegdec_create(0, 4, 0, 1 << 20, ctypes.byref(h)) == bad and not h
    assert lib.pa_jpegdec_create(0, 4, 1024, 16, ctypes.byref(h)) == bad and not h
    assert lib.pa_jpegdec_create(0, 4, 1024, 1 << 20, None) == bad
    assert lib.pa_jpegdec_decode(z, x, x, 1, 1, x, 4096, x, x, z) == bad
    assert lib.pa_jpegdec_set_sync_rounds(z, 0) == bad
    assert lib.pa_jpegdec_last_error(z) == b"null handle"
    lib.pa_jpegdec_destroy(z)


def test_struct_sizes():
    from playaid_core_amd import _lib

    assert ctypes.sizeof(_lib.pa_crop_image) == 16
    assert _lib.pa_crop_image.offset.offset == 0 and _lib.pa_crop_image.height.offset == 8 and _lib.pa_crop_image.width.offset == 12
    assert _lib.PA_ABI_VERSION == 15


def test_the_package_never_imports_the_oracle():
    import playaid_core_amd

    root = os.path.dirname(playaid_core_amd.__file__)
    pat = re.compile(r"^\s*(from|import)\s+oracle\b", re.M)
    for dirpath, _, files in os.walk(root):
        for f in files:
            if f.endswith(".py"):
                assert not pat.search(open(os.path.join(dirpath, f)).read()), f
