"""The host half of the device's JPEG encoder (no GPU): the header bytes and the size bound against live libjpeg-turbo
behind Pillow, the argument checks of the new C ABI entries, and the cache directory's naming (playaid_core_amd/ai_cache.py)."""
import ctypes
import io
import os

import numpy as np
import pytest


@pytest.fixture(scope="module")
def lib():
    from playaid_core_amd import _build, _lib

    _build.build()
    return _lib.load()


def pil_jpeg(rgb, quality, subsampling):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(rgb).save(b, format="JPEG", quality=quality, subsampling=subsampling)
    return b.getvalue()


@pytest.mark.parametrize("subsampling", [0, 2])
@pytest.mark.parametrize("quality", [95, 100, 20])
@pytest.mark.parametrize("hw", [(1, 1), (17, 23), (1080, 1920)])
def test_header_equals_pillows_first_623_bytes(lib, hw, quality, subsampling):
    from playaid_core_amd import jpeg_encode

    h, w = hw
    want = pil_jpeg(np.zeros((h, w, 3), np.uint8), quality, subsampling)
    got = jpeg_encode.jpeg_header(h, w, quality, subsampling)
    assert len(got) == 623 == jpeg_encode.HEADER_BYTES
    assert got == want[:623]
    assert want[621:623] == b"\x3f\x00"   # the header really ends where the scan's parameters end


@pytest.mark.parametrize("subsampling", [0, 2])
@pytest.mark.parametrize("hw", [(64, 64), (17, 23)])
def test_file_bytes_bound_holds_for_noise_at_quality_100(lib, hw, subsampling):
    from playaid_core_amd import jpeg_encode

    h, w = hw
    rgb = np.random.default_rng(5).integers(0, 256, (h, w, 3), dtype=np.uint8)
    size = len(pil_jpeg(rgb, 100, subsampling))
    bound = jpeg_encode.file_bytes_bound(h, w, subsampling)
    assert bound == 623 + 2 * 209 * jpeg_encode.coded_blocks(h, w, subsampling) + 2
    assert bound >= size, (bound, size)


def test_argument_checks_without_a_gpu(lib):
    """Bad arguments come back as PA_ERR_INVALID_ARG before any device call."""
    from playaid_core_amd import _lib

    bad = _lib.PA_ERR_INVALID_ARG
    buf = (ctypes.c_uint8 * 700)()
    n = ctypes.c_int32(0)
    assert lib.pa_jpeg_header(8, 8, 95, 0, buf, 700, ctypes.byref(n)) == _lib.PA_OK and n.value == 623
    assert lib.pa_jpeg_header(8, 8, 95, 2, buf, 623, None) == _lib.PA_OK
    for h, w, q, s, cap in ((8, 8, 0, 0, 700), (8, 8, 101, 0, 700), (8, 8, 95, 1, 700), (0, 8, 95, 0, 700), (8, -1, 95, 0, 700),
                            (8, 8, 95, 0, 622), (65536, 8, 95, 0, 700)):
        assert lib.pa_jpeg_header(h, w, q, s, buf, cap, ctypes.byref(n)) == bad, (h, w, q, s, cap)
    assert lib.pa_jpeg_header(8, 8, 95, 0, None, 700, ctypes.byref(n)) == bad
    assert lib.pa_jpeg_file_bytes_bound(0, 8, 0) == 0 and lib.pa_jpeg_file_bytes_bound(8, 8, 1) == 0
    z, x = ctypes.c_void_p(0), ctypes.c_void_p(4096)   # never dereferenced: every call below is refused first
    h = ctypes.c_void_p(0)
    assert lib.pa_jpegenc_create(0, 0, 1024, 1 << 20, ctypes.byref(h)) == bad and not h
    assert lib.pa_jpegenc_create(0, 4, 0, 1 << 20, ctypes.byref(h)) == bad and not h
    assert lib.pa_jpegenc_create(0, 4, 1024, 16, ctypes.byref(h)) == bad and not h
    assert lib.pa_jpegenc_create(-1, 4, 1024, 1 << 20, ctypes.byref(h)) == bad and not h
    assert lib.pa_jpegenc_create(0, 4, 1024, 1 << 20, None) == bad
    assert lib.pa_jpegenc_encode(z, x, 64, x, 1, 8, 8, 1, 95, 0, x, 4096, x, z) == bad
    assert lib.pa_jpegenc_overflows(z, ctypes.byref(n), z) == bad
    assert lib.pa_jpegenc_last_error(z) == b"null handle"
    lib.pa_jpegenc_destroy(z)
    # a handle whose creation stopped at the device (or succeeded) still refuses bad arguments first
    rc = lib.pa_jpegenc_create(0, 4, 1024, 1 << 20, ctypes.byref(h))
    assert h, rc
    try:
        ok = (h, x, 64, x, 1, 8, 8, 1, 95, 0, x, 4096, x, z)
        for pos, val in ((1, z), (3, z), (4, -1), (5, 0), (6, 65536), (7, 2), (8, 0), (8, 101), (9, 1), (10, z), (12, z)):
            args = list(ok)
            args[pos] = val
            assert lib.pa_jpegenc_encode(*args) == bad, pos
            assert b"pa_jpegenc_encode" in lib.pa_jpegenc_last_error(h)
        assert lib.pa_jpegenc_encode(h, x, 64, x, 5, 8, 8, 1, 95, 0, x, 4096, x, z) == _lib.PA_ERR_CAPACITY   # n > max_images
        assert lib.pa_jpegenc_overflows(h, None, z) == bad
    finally:
        lib.pa_jpegenc_destroy(h)
    assert ctypes.sizeof(_lib.pa_jpeg_file) == 16


def test_cache_names_increment_rule_and_label_text():
    """ai_cache's layout on a hand-written detection table: 1-based label files only for frames with detections, '%g'
    text, crops under the class's name, and YOLOv5's increment_path name for a class's second detection in a frame."""
    from playaid_core_amd import ai_cache, constants
    from playaid_core_amd.ai_runner import read_fighter_yolo_crop_text

    F32 = np.float32
    dets = np.zeros((4, 3, 6), F32)
    counts = np.array([2, 0, 3, 1], np.int32)
    dets[0, 0] = [3, 0.5, 0.25, 0.125, 0.0625, 0.875]
    dets[0, 1] = [2, 0.1, 0.2, 0.3, 0.4, 0.5]
    dets[2, 0] = [2, 0.123456789, 0.5, 0.25, 0.25, 0.9]
    dets[2, 1] = [2, 0.75, 0.5, 0.25, 0.25, 0.8]
    dets[2, 2] = [2, 0.25, 0.5, 0.25, 0.25, 0.7]
    dets[3, 0] = [3, 1.0, 1.0, 1e-5, 0.5, 0.25]
    labels, crops = ai_cache.cache_layout(dets, counts, "vid", constants.CHAR_LIST)
    a, b = constants.CHAR_LIST[2], constants.CHAR_LIST[3]
    j = os.path.join
    assert [p for p, _ in labels] == [j("labels", "vid_1.txt"), j("labels", "vid_3.txt"), j("labels", "vid_4.txt")]
    assert labels[0][1] == "3 0.5 0.25 0.125 0.0625 0.875\n2 0.1 0.2 0.3 0.4 0.5\n"
    assert labels[1][1].splitlines()[0] == "2 0.123457 0.5 0.25 0.25 0.9" and len(labels[1][1].splitlines()) == 3
    assert labels[2][1] == "3 1 1 1e-05 0.5 0.25\n"
    assert crops == [(0, 0, j("crops", b, "vid_1.jpg")), (0, 1, j("crops", a, "vid_1.jpg")),
                     (2, 0, j("crops", a, "vid_3.jpg")), (2, 1, j("crops", a, "vid_32.jpg")), (2, 2, j("crops", a, "vid_33.jpg")),
                     (3, 0, j("crops", b, "vid_4.jpg"))]
    assert ai_cache.label_path("clip", 7) == j("labels", "clip_7.txt")
    assert ai_cache.crop_path("Joker", "clip", 12) == j("crops", "Joker", "clip_12.jpg")
    assert ai_cache.crop_path("Joker", "clip", 12, 1) == j("crops", "Joker", "clip_122.jpg")
    # the text parses back to the table's rows with the runner's own reader
    c = read_fighter_yolo_crop_text(labels[0][1], b)
    assert (c.center_x, c.center_y, c.crop_width, c.crop_height, c.confidence, c.class_id) == (0.5, 0.25, 0.125, 0.0625, 0.875, 3)
    with pytest.raises(ValueError):
        ai_cache.cache_layout(np.array([[[99, 0.5, 0.5, 0.1, 0.1, 0.9]]], F32), np.array([1], np.int32), "vid", constants.CHAR_LIST)


def test_clip_source_from_cache_reads_labels_and_crop_files(tmp_path):
    """ClipSource.from_cache on a directory written by hand with Pillow: labels per frame ('' where there is no file),
    crop images decoded like cv2.imread (BGR), None where the detector saved none; the clip is as long as its last label."""
    from PIL import Image

    from playaid_core_amd import constants
    from playaid_core_amd.ai_runner import ClipSource

    a, b = constants.CHAR_LIST[2], constants.CHAR_LIST[3]
    root = tmp_path / "cache"
    (root / "labels").mkdir(parents=True)
    for f in (a, b):
        (root / "crops" / f).mkdir(parents=True)
    rgb = np.random.default_rng(1).integers(0, 256, (21, 34, 3), dtype=np.uint8)
    (root / "labels" / "v_1.txt").write_text("2 0.5 0.5 0.1 0.1 0.9\n3 0.25 0.5 0.1 0.1 0.8\n")
    (root / "labels" / "v_3.txt").write_text("2 0.5 0.5 0.1 0.1 0.9\n")
    (root / "labels" / "other_9.txt").write_text("2 0.5 0.5 0.1 0.1 0.9\n")
    Image.fromarray(rgb).save(str(root / "crops" / a / "v_1.jpg"), quality=95, subsampling=0)
    Image.fromarray(rgb[:8, :8]).save(str(root / "crops" / b / "v_1.jpg"), quality=95, subsampling=0)
    Image.fromarray(rgb).save(str(root / "crops" / a / "v_3.jpg"), quality=95, subsampling=0)
    clip = ClipSource.from_cache("/somewhere/v.avi", str(root))
    assert clip.name == "v" and clip.frames.shape == (3, 0, 0, 3)
    assert clip.labels == ["2 0.5 0.5 0.1 0.1 0.9\n3 0.25 0.5 0.1 0.1 0.8\n", "", "2 0.5 0.5 0.1 0.1 0.9\n"]
    want = np.asarray(Image.open(str(root / "crops" / a / "v_1.jpg")).convert("RGB"))[..., ::-1]
    assert np.array_equal(clip.crop_images[0][0], want) and clip.crop_images[0][1].shape == (8, 8, 3)
    assert clip.crop_images[1] == [None, None] and clip.crop_images[2][1] is None and np.array_equal(clip.crop_images[2][0], want)
    frames = np.zeros((2, 4, 4, 3), np.uint8)
    clip2 = ClipSource.from_cache(frames, str(root), name="v")
    assert clip2.frames is frames and len(clip2.labels) == 2 and len(clip2.crop_images) == 2
    with pytest.raises(FileNotFoundError):
        ClipSource.from_cache("nothing.avi", str(root))
