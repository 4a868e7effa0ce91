"""The crop stage's reference arithmetic (csrc/crop_math.h) against the oracle, on the CPU.

Every kernel of csrc/preprocess.hip and csrc/crop_sized.hip takes its slice / contain / paste geometry, its INTER_AREA branch and
destination pixel, its Pillow coefficient rows and bicubic output values and its base-256 digit form from that one header.
tests/helpers/crop_math_table.cpp includes nothing else and runs the same functions over plain host buffers in the multi-pass form
(plan -> horizontal pass -> vertical pass -> INTER_AREA); it is compiled with the host C++ compiler alone ($CXX, else g++), with
``-ffp-contract=off`` like the kernels. Everything here is byte equality with ``oracle.yolo_crop`` / ``oracle.resample``: no tolerance.
"""
import importlib.util
import os
import shutil
import struct
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import frame_geometry as fg  # noqa: E402
from oracle import resample, yolo_crop  # noqa: E402

SRC = os.path.join(ROOT, "tests", "helpers", "crop_math_table.cpp")

# (h, w) of a crop image per branch cv2.resize(INTER_AREA) takes to width 128: copy, 2 x 2, integer, fractional, enlarging
NON_SQUARE_SOURCES = [(96, 128), (200, 256), (300, 384), (150, 200), (48, 64)]


@pytest.fixture(scope="module")
def run(tmp_path_factory):
    cxx = os.environ.get("CXX") or "g++"
    if not shutil.which(cxx.split()[0]):
        pytest.skip(f"no host C++ compiler ({cxx})")
    tmp = tmp_path_factory.mktemp("crop_math")
    exe = str(tmp / "crop_math_table")
    subprocess.run(cxx.split() + ["-std=c++17", "-O1", "-ffp-contract=off", "-o", exe, SRC], check=True)
    count = [0]

    def call(*parts):
        count[0] += 1
        src, dst = str(tmp / f"in{count[0]}.bin"), str(tmp / f"out{count[0]}.bin")
        with open(src, "wb") as f:
            for p in parts:
                f.write(p)
        subprocess.run([exe, src, dst], check=True)
        with open(dst, "rb") as f:
            out = f.read()
        os.remove(src)
        os.remove(dst)
        return out

    return call


def square_crops(run, frames, cases, size):
    """cases [(frame index, box, padding)] -> (status int32[k], crops uint8[k, size, size, 3]) of the host program."""
    n, h, w, _ = frames.shape
    recs = b"".join(struct.pack("<ii4d", int(f), int(pad), *[float(v) for v in box]) for f, box, pad in cases)
    out = run(struct.pack("<6i", 1, n, h, w, len(cases), size), np.ascontiguousarray(frames).tobytes(), recs)
    k = len(cases)
    assert len(out) == 4 * k + k * size * size * 3
    return np.frombuffer(out, np.int32, k), np.frombuffer(out, np.uint8, offset=4 * k).reshape(k, size, size, 3)


def images(run, imgs, out_w, swap_rb=True):
    """imgs through the runner's input branch (out_w 0) or imutils.resize(width=out_w) -> (status, [output])."""
    head = struct.pack("<3i", 2, len(imgs), int(swap_rb)) + b"".join(struct.pack("<3i", im.shape[0], im.shape[1], out_w) for im in imgs)
    out = run(head, *[np.ascontiguousarray(im).tobytes() for im in imgs])
    status = np.frombuffer(out, np.int32, len(imgs))
    at, res = 4 * len(imgs), []
    for im in imgs:
        shape = (128, 128, 3) if out_w == 0 else (int(im.shape[0] * (out_w / float(im.shape[1]))), out_w, 3)
        res.append(np.frombuffer(out, np.uint8, int(np.prod(shape)), offset=at).reshape(shape))
        at += int(np.prod(shape))
    assert at == len(out)
    return status, res


@pytest.mark.parametrize("fi", range(len(fg.FRAMES)), ids=[f"{h}x{w}" for h, w in fg.FRAMES])
def test_every_case_of_a_frame_size_equals_the_oracle(run, fi):
    """Every case of ``fg.crop_cases(fi)`` -- every slice shape x INTER_AREA branch, the 127-row sides, the three paddings --
    against ``fg.expected(fi)``: status and all 128 x 128 x 3 bytes."""
    where = fg.slot_of(fi)
    cases = [(where[i][1], box, pad) for i, (box, pad) in enumerate(fg.crop_cases(fi))]
    status, crops = square_crops(run, fg.frames(fi), cases, 128)
    bad = fg.first_mismatch(fi, crops, status, "crop_math.h on the host")
    assert bad is None, bad


def test_refused_geometry_has_its_status(run):
    for fi, box, pad in fg.refused_cases():
        H, W = fg.FRAMES[fi]
        status, crops = square_crops(run, fg.frames(fi)[:1], [(0, box, pad)], 128)
        assert status[0] == fg.expected_refusal(box, H, W, pad), (fi, box, pad, int(status[0]))
        assert not crops.any()


def _any_size():
    spec = importlib.util.spec_from_file_location("crop_any_size_cases", os.path.join(ROOT, "tests", "test_crop_any_size.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("size", [16, 96, 512])
def test_other_output_sizes_equal_the_oracle(run, size):
    """tests/test_crop_any_size.py's boxes (those of S = 96 and of S = 256: sides 45 .. 640 at its five centres, the off-screen box)
    on one 720p frame, cut at S = 16, 96 and 512."""
    cas = _any_size()
    frame = cas.frames_720()[:1]
    for pad in (30, 0):
        boxes = np.concatenate([cas.cases(96, pad).reshape(-1, 4), cas.cases(256, pad).reshape(-1, 4)])
        status, crops = square_crops(run, frame, [(0, tuple(b), pad) for b in boxes], size)
        made = 0
        for k, box in enumerate(boxes):
            ok, want = yolo_crop.square_crop(frame[0], tuple(box), size, padding=pad)
            assert (status[k] == 0) == bool(ok), (size, pad, k, int(status[k]))
            if ok:
                made += 1
                assert np.array_equal(crops[k], want), (size, pad, k, int((crops[k] != want).sum()))
            else:
                assert not crops[k].any()
        assert made >= len(boxes) - 2


def test_runner_inputs_from_non_square_sources(run):
    """One source per INTER_AREA branch with sw != sh, then ImageOps.pad's bicubic pass and paste: ``runner_input_from_crop``."""
    rng = np.random.default_rng(5)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in NON_SQUARE_SOURCES]
    status, got = images(run, imgs, 0)
    assert (status == 0).all(), status
    for im, g in zip(imgs, got):
        assert np.array_equal(g, yolo_crop.runner_input_from_crop(im)), im.shape


def test_rectangles_resized_to_a_width(run):
    """``imutils.resize(width=256)`` of rectangles (the damage HUD crops), every branch: enlarging, copy, 2 x 2, integer, fractional."""
    rng = np.random.default_rng(6)
    imgs = [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in [(37, 101), (64, 256), (100, 512), (90, 768), (75, 300)]]
    status, got = images(run, imgs, 256)
    assert (status == 0).all(), status
    for im, g in zip(imgs, got):
        assert np.array_equal(g, resample.imutils_resize_width(im, 256)), im.shape


def _digit_passes():
    """The passes tests/test_crop_mfma.py::test_digit_split_is_exact_* enumerate: every unclipped (2 * (d / 2) + 60 -> d), d = 1 ..
    1024, then its clipped and enlarging pairs (the same seed)."""
    rng = np.random.default_rng(7)
    pairs = [(40, 160), (161, 160), (150, 188), (160, 200), (3, 7), (7, 3), (250, 167), (188, 129), (64, 64 + 1), (299, 200)]
    pairs += [(int(a), int(b)) for a, b in zip(rng.integers(2, 700, 40), rng.integers(2, 700, 40)) if a / b <= 1.5]
    return [(2 * (d // 2) + 60, d) for d in range(1, 1025)] + pairs


def test_digit_split_and_row_constant(run):
    """``coef_digits`` and ``coef_row_constant`` for every coefficient of those passes: d0 + 256 d1 + 65536 d2 == k with d0 and d1 in
    [-128, 127], the constant 2^21 + 128 * (sum of the row's first seven taps); the coefficients themselves are the oracle's."""
    passes = _digit_passes()
    out = run(struct.pack("<2i", 3, len(passes)), b"".join(struct.pack("<2i", a, b) for a, b in passes))
    n_rows, n_coef = struct.unpack_from("<2i", out)
    assert n_rows == sum(b for _, b in passes) and len(out) == 8 + 8 * n_rows + 16 * n_coef
    rows = np.frombuffer(out, np.int32, 2 * n_rows, offset=8).reshape(n_rows, 2).astype(np.int64)
    quads = np.frombuffer(out, np.int32, 4 * n_coef, offset=8 + 8 * n_rows).reshape(n_coef, 4).astype(np.int64)
    k, d0, d1, d2 = quads.T
    assert np.array_equal(d0 + 256 * d1 + 65536 * d2, k)
    for d in (d0, d1):
        assert d.min() >= -128 and d.max() <= 127
    taps = rows[:, 0]
    cnt = np.minimum(taps, fg.MAX_TAPS)      # what a table row holds; a pass of more taps is refused (d < 18 of the unclipped ones)
    assert cnt.sum() == n_coef and cnt.min() >= 1
    first = np.cumsum(cnt) - cnt
    tap = np.arange(7)[None, :]
    taken = np.where(tap < cnt[:, None], k[np.minimum(first[:, None] + tap, n_coef - 1)], 0)
    assert np.array_equal(rows[:, 1], 128 * taken.sum(axis=1) + (1 << 21))
    # the table is Pillow's: a few of the passes against the oracle's coefficients
    at = 0
    for i, (a, b) in enumerate(passes):
        n = int(cnt[at:at + b].sum())
        if i % 97 == 0 or i >= 1024:
            ksize, bounds, kk = resample.pil_bicubic_coeffs(a, b)
            want = np.concatenate([kk[r, :int(bounds[r, 1])] for r in range(b)]).astype(np.int64)
            lo = int(first[at])
            assert np.array_equal(taps[at:at + b], bounds[:, 1]), (a, b)
            if ksize <= fg.MAX_TAPS:
                assert np.array_equal(k[lo:lo + n], want), (a, b)
        at += b
