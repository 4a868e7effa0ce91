"""The crop stage's horizontal bicubic pass on the int8 matrix instruction (csrc/preprocess.hip, ``CropPlan::mfma_h``).

CPU: the facts the form rests on, from ``oracle/resample.py``'s own coefficients -- the taps of ten output pixels of every
unclipped 7-tap pass span at most 60 bytes (so they fit the 64-byte window behind any misalignment), and a numpy
restatement of the per-crop operand (``crop_hop_kernel``: digit planes in fragment order, tap positions shifted by the
slice's misalignment) run the way the kernel runs it (int8 products with pixels - 128, Horner in wrapping int32, constant
with the middle digit) reproduces ``resample``'s accumulator ``2^21 + sum p k`` exactly. The GPU cases' geometry is asserted
through a host mirror of the plan (helpers/crop_mfma_h_cases.py), so a case cannot stop being one.

GPU: ``Engine.square_crops`` byte for byte, statuses included, against ``oracle.yolo_crop.square_crop``, against children
with ``PA_CROP_MFMA_H=0`` and ``PA_CROP_MFMA=0`` (helpers/crop_mfma_h_worker.py), and against repeated calls.
"""
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
from helpers import crop_mfma_h_cases as ch  # noqa: E402


# =====================================================================================================================
# CPU: window, operand, partial sums
# =====================================================================================================================
@pytest.mark.parametrize("lo,hi", [(119, 400), (401, 700), (701, 1024)])
def test_ten_pixel_blocks_span_at_most_60_bytes(lo, hi):
    """Every pass ``2 * (d / 2) + 60 -> d`` of at most 7 taps (d = 119 .. 1024 are all of them in that range): the taps of any
    block of ten output pixels span at most 20 source pixels = 60 bytes; with the 3 bytes of alignment slack that is the
    64-byte window."""
    for d in range(lo, hi + 1):
        in_size = 2 * (d // 2) + 60
        ksize, bounds, _ = resample.pil_bicubic_coeffs(in_size, d)
        assert ksize <= 7, (d, ksize)
        lo_px = bounds[:, 0].astype(np.int64)
        hi_px = lo_px + bounds[:, 1]
        for x0 in range(0, d, ch.HOP_PIXELS):
            x1 = min(x0 + ch.HOP_PIXELS, d)
            span = 3 * int(hi_px[x0:x1].max() - lo_px[x0:x1].min())
            assert span <= 60, (d, x0, span)
        # and the host mirror's shortcut (first pixel's first tap, last pixel's end) is the same span (every eighth d, one
        # misalignment each: the shortcut rests on the bounds being monotone, which does not depend on d)
        for mis in ([d & 3] if d % 8 == 7 else []):
            wins = ch.block_windows(in_size, d, mis)
            for b, (first, w) in enumerate(wins):
                x0, x1 = b * ch.HOP_PIXELS, min((b + 1) * ch.HOP_PIXELS, d)
                assert first == lo_px[x0:x1].min()
                assert w == ((mis + 3 * first) & 3) + 3 * int(hi_px[x0:x1].max() - first) <= ch.HOP_WINDOW


def _pixel_rows(k_full, rng):
    """Source rows [3 + 2 * picked outputs][in_size * 3] for a pass whose dense coefficient matrix is k_full [out][in]: random, all 0, all
    255, then for every output (of a pass wider than 200: for 96 outputs spread over it, both ends included) one row with 255
    under its positive taps and one with 255 under its negative taps (the two that push that output's sum furthest; every row
    is checked at every output all the same)."""
    in_size = k_full.shape[1]
    rows = [rng.integers(0, 256, in_size * 3), np.zeros(in_size * 3, np.int64), np.full(in_size * 3, 255)]
    rows = np.stack(rows)
    pick = np.arange(k_full.shape[0]) if k_full.shape[0] <= 200 else np.linspace(0, k_full.shape[0] - 1, 96).astype(np.int64)
    pos = np.repeat(np.where(k_full[pick] > 0, 255, 0), 3, axis=1)
    neg = np.repeat(np.where(k_full[pick] < 0, 255, 0), 3, axis=1)
    return np.concatenate([rows, pos, neg]).astype(np.uint8)


def _check_operand(in_size, out_size, rng):
    ksize, bounds, kk = resample.pil_bicubic_coeffs(in_size, out_size)
    assert ksize <= 7
    k_full = np.zeros((out_size, in_size), np.int64)
    for xx in range(out_size):
        k_full[xx, bounds[xx, 0]:bounds[xx, 0] + bounds[xx, 1]] = kk[xx, :bounds[xx, 1]]
    px = _pixel_rows(k_full, rng)
    # the oracle's accumulator (resample._resample_axis1), before >> 22: per channel 2^21 + sum p k
    m = px.shape[0]
    p3 = px.reshape(m, in_size, 3).astype(np.int64)
    want = ((1 << 21) + np.einsum("mic,oi->moc", p3, k_full)).reshape(m, out_size * 3)
    worst = 0
    for mis in range(4):
        if not all(w <= ch.HOP_WINDOW for _, w in ch.block_windows(in_size, out_size, mis)):
            continue
        op = ch.build_operand(bounds, kk, out_size, mis)
        assert op.shape == ((out_size + 9) // 10, ch.HOP_BLOCK_BYTES)
        # the staged row: ``mis`` bytes of whatever precedes the slice in the frame, then the slice
        staged = np.concatenate([rng.integers(0, 256, (m, mis)).astype(np.uint8), px], axis=1)
        got, biggest = ch.run_operand(op, staged, out_size)
        assert np.array_equal(got, want), (in_size, out_size, mis)
        worst = max(worst, biggest, int(np.abs(want).max()))
    assert worst < 2 ** 31
    return worst


def test_operand_reproduces_the_oracle_accumulator():
    """Unclipped passes over the range of d, the clipped passes of the GPU cases, and passes at both ends of the 7-tap range:
    every misalignment the window admits, the five kinds of pixel rows, every partial sum below 2^31."""
    rng = np.random.default_rng(11)
    pairs = [(2 * (d // 2) + 60, d) for d in (119, 120, 128, 129, 130, 131, 160, 191, 240, 283, 356, 640, 1024)]
    pairs += [(190, 146), (180, 137), (330, 295), (161, 160), (150, 149)]
    worst = max(_check_operand(i, o, rng) for i, o in pairs)
    assert worst < 2 ** 31


def test_cases_are_what_they_say():
    plans = {c[0]: ch.plan_of(i) for i, c in enumerate(ch.CASES)}
    on = {n: p for n, p in plans.items() if p["mfma_h"]}
    assert set(on) == {"d128_m0", "d129_m3", "d130_m2", "d131_m1", "d160_m1", "d191_m0", "d240_m2", "clip_left", "clip_right"}
    assert all(p["mfma_v"] and p["rb"] == 8 for p in on.values())
    assert {p["d"] for p in on.values()} >= {128, 129, 130, 131, 160, 191}
    assert {p["h_mis"] for p in on.values()} == {0, 1, 2, 3}
    assert {p["rw"] % ch.HOP_PIXELS == 0 for p in on.values()} == {True, False}
    assert plans["d191_m0"]["rw"] % ch.HOP_PIXELS == 1 and plans["d129_m3"]["rw"] % ch.HOP_PIXELS == 9   # partial last blocks
    for p in on.values():
        top, bottom = p["bands8"][0], p["bands8"][-1]
        assert 0 < top[0] < 32 and 0 < bottom[0] < 32 and max(b[0] for b in p["bands8"]) <= 32
        assert p["window_fits"] and max(w for _, w in p["windows"]) <= ch.HOP_WINDOW
    # clipped at an edge: not a cached pass, own coefficient rows; the window check decides the form either way
    left, right = plans["clip_left"], plans["clip_right"]
    assert left["sx0"] == 0 and left["sw"] != 2 * (left["rw"] // 2) + 60 and left["mfma_h"] == left["window_fits"]
    assert right["sx0"] + right["sw"] == ch.SETS["main"][1] and right["sw"] != 2 * (right["rw"] // 2) + 60
    assert right["mfma_h"] == right["window_fits"]
    # rows of 1914 bytes: matrix vertical pass, vector horizontal pass
    for n in ("odd_pitch", "odd_pitch_b"):
        assert plans[n]["mfma_v"] and not plans[n]["mfma_h"] and plans[n]["window_fits"] and (ch.SETS["odd"][1] * 3) % 4 == 2
    # more than 32 source rows in a sub-band whose vector form fits at the same height: neither matrix form
    o = plans["over_32_rows"]
    assert o["rb"] == 8 and max(b[0] for b in o["bands8"]) > 32 and not o["mfma_v"] and not o["mfma_h"] and o["ksize_h"] <= 7
    # the knobs on the host mirror: both off under PA_CROP_MFMA=0, the horizontal one alone under PA_CROP_MFMA_H=0,
    # and the sub-band height never falls for the matrix forms' sake
    for i, c in enumerate(ch.CASES):
        a, b, v = ch.plan_of(i), ch.plan_of(i, mfma_h=0), ch.plan_of(i, mfma=0)
        assert not b["mfma_h"] and b["mfma_v"] == a["mfma_v"] and not v["mfma_h"] and not v["mfma_v"]
        assert a["rb"] >= b["rb"] >= v["rb"], c[0]


# =====================================================================================================================
# GPU
# =====================================================================================================================
_ORACLE = {}


def _oracle_crop(fs, frame, bx):
    key = (fs, frame, tuple(bx))
    if key not in _ORACLE:
        from oracle import yolo_crop

        if ("frames", fs) not in _ORACLE:
            _ORACLE[("frames", fs)] = ch.frames(fs)
        good, c = yolo_crop.square_crop(_ORACLE[("frames", fs)][frame], bx, 128, padding=30)
        assert good
        _ORACLE[key] = c
    return _ORACLE[key]


SETTINGS = {"default": {}, "h_off": {"PA_CROP_MFMA_H": "0"}, "vector": {"PA_CROP_MFMA": "0"}}


@pytest.fixture(scope="module")
def runs(tmp_path_factory):
    """The three children, started together, once per module."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    tmp = tmp_path_factory.mktemp("crop_mfma_h")
    procs = {}
    for name, extra in SETTINGS.items():
        env = dict(os.environ)
        for k in ("PA_CROP_MFMA", "PA_CROP_MFMA_H", "PA_CROP_XCD", "PA_PRE_ABLATE"):
            env.pop(k, None)
        env.update(extra)
        path = str(tmp / (name + ".npz"))
        procs[name] = (path, subprocess.Popen([sys.executable, os.path.join(ROOT, "tests", "helpers", "crop_mfma_h_worker.py"), path],
                                              stdout=subprocess.PIPE, stderr=subprocess.PIPE, text=True, env=env))
    res = {}
    for name, (path, pr) in procs.items():
        _, err = pr.communicate(timeout=600)
        assert pr.returncode == 0, (name, pr.returncode, err[-2000:])
        res[name] = dict(np.load(path))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("setting", list(SETTINGS))
def test_cases_match_the_oracle(runs, setting):
    """Every case, every byte and status, in all three settings; the second call and the reversed order as well."""
    r = runs[setting]
    for key, st in (("crops", "status"), ("crops_again", "status_again"), ("crops_rev", "status_rev")):
        assert np.array_equal(r[st], np.zeros(len(ch.CASES), np.int64)), (setting, key, r[st])
        for i, (name, fs, fr, bx) in enumerate(ch.CASES):
            want = _oracle_crop(fs, fr, bx)
            assert np.array_equal(r[key][i], want), f"{setting} / {key}: case {name} differs from the oracle in {int((r[key][i] != want).sum())} bytes"


@pytest.mark.gpu
def test_settings_agree_byte_for_byte(runs):
    d = runs["default"]
    for other in ("h_off", "vector"):
        for key in d:
            assert np.array_equal(d[key], runs[other][key]), (other, key)


@pytest.mark.gpu
@pytest.mark.parametrize("nf,slots", ch.COUNTS)
def test_crop_counts(runs, nf, slots):
    """1, 5 (six slots), 12 and 80 crops a call -- the last two fill whole groups of 8 rows of the crop kernel's grid, which it
    deals to the XCDs crop by crop."""
    r = runs["default"]
    _, idx = ch.mixed_boxes(nf, slots)
    got, st = r[f"count_{nf}"], r[f"count_status_{nf}"]
    assert got.shape == (nf, slots, 128, 128, 3) and not st.any()
    used = nf * slots if nf != 3 else 5
    for s in range(used):
        f, q = divmod(s, slots)
        want = _oracle_crop("main", f & 1, ch.CASES[idx[f, q]][3])
        assert np.array_equal(got[f, q], want), (nf, f, q, ch.CASES[idx[f, q]][0])


@pytest.mark.gpu
def test_twenty_launches_and_a_long_clip(runs):
    from oracle import pipeline

    r = runs["default"]
    assert bool(r["twenty_equal"])
    bx, _ = ch.mixed_boxes(ch.CLIP_FRAMES, 2)
    want, ok = pipeline.crops_for_clip(ch.mixed_frames(ch.CLIP_FRAMES), bx)
    assert ok.all() and ch.CLIP_FRAMES > 2 * ch.CLIP_BATCH
    assert np.array_equal(r["clip_rgb"], want)
