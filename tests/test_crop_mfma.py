"""The crop stage's vertical bicubic pass on the int8 matrix instruction (csrc/preprocess.hip, ``CropPlan::mfma_v``).

CPU: the arithmetic the kernel relies on, against ``oracle/resample.py``'s own coefficients and integer sums -- every 22-bit
coefficient splits into three base-256 digits that fit int8, pixels offset to p - 128, and
``2^21 + sum p k == D0 + (D1 << 8) + (D2 << 16) + 128 sum k + 2^21`` with ``D_j = sum (p - 128) d_j``; the source rows of 32
consecutive outputs of a 7-tap pass span at most 64.

GPU: ``Engine.square_crops`` bit for bit against ``oracle.yolo_crop.square_crop`` and against the same engine with
``PA_CROP_MFMA=0`` (the vector form, read once per process: a child, tests/helpers/crop_mfma_worker.py) on boxes that reach
every branch of the new path; the boxes' geometry is asserted here on the CPU, so a case cannot silently stop being one.
"""
import math
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import resample  # noqa: E402

sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import crop_mfma_cases as cm  # noqa: E402


# =====================================================================================================================
# CPU: digits, offset identity, K span
# =====================================================================================================================
def _digits(k):
    """k = d0 + 256 d1 + 65536 d2 with d0, d1 in [-128, 127] (the kernel's split, on int64 arrays)."""
    d0 = ((k & 0xFF) ^ 0x80) - 0x80
    k1 = (k - d0) >> 8
    d1 = ((k1 & 0xFF) ^ 0x80) - 0x80
    d2 = (k1 - d1) >> 8
    return d0, d1, d2


def _check_pass(in_size, out_size, rng):
    ksize, bounds, kk = resample.pil_bicubic_coeffs(in_size, out_size)
    cnt = bounds[:, 1].astype(np.int64)
    valid = np.arange(ksize)[None, :] < cnt[:, None]
    k = np.where(valid, kk, 0).astype(np.int64)
    d0, d1, d2 = _digits(k)
    assert np.array_equal(d0 + 256 * d1 + 65536 * d2, k)
    for d in (d0, d1, d2):
        assert d.min() >= -128 and d.max() <= 127, (in_size, out_size, int(d.min()), int(d.max()))
    # pixel rows: random, all 0, all 255, and the two that push a sum furthest (255 under the positive / negative taps)
    px = [rng.integers(0, 256, size=k.shape, dtype=np.int64), np.zeros_like(k), np.full_like(k, 255), np.where(k > 0, 255, 0),
          np.where(k < 0, 255, 0)]
    for p in px:
        want = (1 << 21) + (p * k).sum(axis=1)  # the oracle's accumulator (resample._resample_axis1), before >> 22
        q = p - 128
        s0, s1, s2 = (q * d0).sum(axis=1), (q * d1).sum(axis=1), (q * d2).sum(axis=1)
        for s in (s0, s1, s2, want):
            assert np.abs(s).max() < 2 ** 31
        # the kernel's order: Horner in wrapping int32, constant added with the middle digit
        cst = 128 * k.sum(axis=1) + (1 << 21)
        acc = s2.astype(np.int32)
        acc = (acc.astype(np.uint32) << np.uint32(8)).astype(np.uint32) + s1.astype(np.int32).astype(np.uint32)
        acc = ((acc << np.uint32(8)).astype(np.uint32) + cst.astype(np.int32).astype(np.uint32)).astype(np.uint32)
        acc = (acc + s0.astype(np.int32).astype(np.uint32)).astype(np.uint32).astype(np.int32)
        assert np.array_equal(acc.astype(np.int64), want), (in_size, out_size)
    return ksize, bounds


@pytest.mark.parametrize("lo,hi", [(1, 400), (401, 640), (641, 850), (851, 1024)])
def test_digit_split_is_exact_for_every_unclipped_pass(lo, hi):
    """Every pass ``2 * (d / 2) + 60 -> d`` (the slice of a crop no frame edge clips), d = lo .. hi: digits in int8, the
    offset identity equal to the oracle's integer sum on five pixel patterns per output, and -- for the passes of at most 7
    taps, the only ones the matrix form takes -- at most 64 source rows under any 32 consecutive outputs (the oracle alone
    says so; the plan kernel checks each sub-band of a crop against the kernel's own 32 x 32 tile)."""
    rng = np.random.default_rng(1000 + lo)
    for d in range(lo, hi + 1):
        in_size = 2 * (d // 2) + 60
        ksize, bounds = _check_pass(in_size, d, rng)
        lo_row = bounds[:, 0].astype(np.int64)
        hi_row = lo_row + bounds[:, 1]
        n = len(lo_row)
        w = min(32, n)
        span = hi_row[w - 1:] - lo_row[: n - w + 1]
        if d >= 120:
            assert ksize <= 7, (d, ksize)
        if ksize <= 7:   # (the wider filters of d < 120 never take the matrix form; d = 6 spans 66 rows)
            assert span.max() <= 64, (d, int(span.max()))


def test_digit_split_is_exact_for_clipped_and_enlarging_passes():
    """Passes the cache does not hold -- clipped slices, enlarging ones, both ends of the <= 7-tap range: the digits still fit
    int8 (normalised coefficients stay below 2^23) and the identity holds."""
    rng = np.random.default_rng(7)
    pairs = [(40, 160), (161, 160), (150, 188), (160, 200), (3, 7), (7, 3), (250, 167), (188, 129), (64, 64 + 1), (299, 200)]
    pairs += [(int(a), int(b)) for a, b in zip(rng.integers(2, 700, 40), rng.integers(2, 700, 40)) if a / b <= 1.5]
    for in_size, out_size in pairs:
        _check_pass(in_size, out_size, rng)


# =====================================================================================================================
# CPU: the GPU cases are what their names say
# =====================================================================================================================
def test_cases_reach_every_branch():
    plans = {name: cm.plan(box, cm.H, cm.W, pad) for name, pad, box in cm.CASES}
    both = [p for p in plans.values() if p["need_h"] and p["need_v"] and p["ksize_v"] <= 7 and not p["fallback"]]
    assert {p["d"] for p in both} >= {129, 160, 191}
    assert {(p["rw"] * 3) % 4 == 0 for p in both} == {True, False}
    assert {(p["rw"] * 3) % 32 == 0 for p in both} == {True, False}          # a full and a partial last 32-byte column block
    assert {(p["sx0"] * 3) % 4 for p in both} == {0, 1, 2, 3}                # every byte misalignment of the slice start
    assert all(0 < p["n2_max"] <= 32 and p["n0_max"] <= 32 for p in both)
    assert any(p["n2_max"] % 32 for p in both)                               # the 32-row block is partial
    v = plans["vertical_only"]
    assert v["need_v"] and not v["need_h"] and v["sy0"] == 0                  # clipped by the top edge
    h = plans["horizontal_only"]
    assert h["need_h"] and not h["need_v"] and h["sx0"] == 0                  # clipped by the left edge
    e = plans["enlarging"]
    assert e["need_h"] and e["need_v"] and e["rw"] > e["sw"] and e["rh"] > e["sh"] and e["b2_over_b0"] and not e["fallback"]
    for name in ("wide_filter_a", "wide_filter_b"):
        assert plans[name]["need_v"] and plans[name]["ksize_v"] > 7 and plans[name]["ksize_v"] <= 15 and not plans[name]["fallback"]
    assert plans["fallback"]["fallback"] and plans["fallback"]["need_h"] and plans["fallback"]["need_v"]


# =====================================================================================================================
# GPU
# =====================================================================================================================
_WANT = {}


def _want():
    """The oracle's crops of every case, once per module: (ok bool[n], crops uint8[n,128,128,3] BGR)."""
    if not _WANT:
        from oracle import yolo_crop

        frames = cm.frames()
        ok, crops = [], []
        for i, (name, pad, box) in enumerate(cm.CASES):
            good, c = yolo_crop.square_crop(frames[cm.frame_of(i)], box, 128, padding=pad)
            ok.append(bool(good))
            crops.append(c if good else np.zeros((128, 128, 3), np.uint8))
        _WANT["v"] = (np.array(ok), np.stack(crops))
    return _WANT["v"]


def _run_child(tmp_path, name, mfma):
    env = dict(os.environ)
    env.pop("PA_CROP_MFMA", None)
    if mfma is not None:
        env["PA_CROP_MFMA"] = mfma
    path = str(tmp_path / name)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "crop_mfma_worker.py"), path], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, (mfma, r.returncode, r.stderr[-2000:])
    return np.load(path)


@pytest.mark.gpu
def test_matrix_form_is_bit_exact(tmp_path):
    """Default build (matrix form on) against the oracle, against a second call on the same inputs, and against the vector
    form (``PA_CROP_MFMA=0``, a fresh child) -- every byte and every status."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    ok, want = _want()
    assert ok.all()
    got = _run_child(tmp_path, "mfma.npz", None)
    old = _run_child(tmp_path, "vector.npz", "0")
    names = [c[0] for c in cm.CASES]
    for label, res in (("matrix form", got), ("vector form", old)):
        assert np.array_equal(res["status"], np.zeros(len(names), np.int64)), (label, res["status"])
        for i, nm in enumerate(names):
            assert np.array_equal(res["crops"][i], want[i]), f"{label}: case {nm} differs from the oracle in {int((res['crops'][i] != want[i]).sum())} bytes"
    assert np.array_equal(got["crops"], got["crops_again"]) and np.array_equal(got["status"], got["status_again"])
    assert np.array_equal(got["crops"], old["crops"])
