"""The temporal head's inference path -- ``pa_head_frames``: ``window_gather_kernel`` (csrc/misc.hip), the Conv1d as a gathered
split-K igemm (``run_head`` in csrc/pa_api.hip, ``igemm_f32_kernel<.., GATHER>``) and ``head_mlp_kernel`` (the deferred slab sum, the
MLP, log-softmax, argmax and the records) -- against float64 on features the tests import (``clip_begin`` + ``features_import`` +
``head_frames``: no backbone runs except where a test says so). Reference, features and the bar (|logp - ref| <= 1e-5 absolute):
tests/helpers/head_windows.py.

What the cases reach: S = 1 (no reach, A = 1: one live lane, logp exactly 0), 3, 5, 7, 9 and 15 (reach 49 of a 70-frame clip);
one to four fighters with four distinct class ids; A = 1, 2, 37, 63 and 64 (every lane a class); passes that start above ``lo``;
a pass of exactly 64 windows and one of 65 (a second 64-row tile); clip batches down to the two-frame minimum against the
reference sampler per clip, seam rows included; the cached window table (re-use, invalidation by ``pa_infer_windows``, batched
against plain clips of equal length); the first-index tie break on bit-equal logits; the record's status as the crop status of the
window's middle row, and as 0 after ``pa_features_import``; ``PA_HEAD_SPLITK`` = 1 (the igemm's own bias + ReLU epilogue and
``head_mlp_kernel``'s ``h1`` branch), 3 (uneven runs: 75 / 75 / 74 k-steps at S = 7) and 32, each in a child process.

Measured on an MI355X (max |dlogp| over the case's ranges; share of windows left out of the action_id comparison as near-ties):
  S1 A1 F1 0 (logp exactly 0.0, prob exactly 1.0) | S3 A2 F2 5.4e-7 | S5 A37 F3 9.4e-7 | S7 A63 F2 1.21e-6, the same on emulated_f32
  and bf16 | S9 A64 F4 1.46e-6 | S15 A64 F1 1.33e-6
  clip batches: 3 x 20 frames 1.25e-6 (plain clip of 60: 1.22e-6; the two differ by 1.71 next to a seam), 5 x 2 frames 3.3e-7
  (plain clip of 10: 2.9e-7; differ by 0.93)
  tied pairs (5, 40) 2.7e-6, (62, 63) 2.6e-6: equal bits, the lower index in all 20 windows
  PA_HEAD_SPLITK (S = 7 / S = 1): unset 1.21e-6 / 5.6e-7, 1: 3.57e-6 / 1.32e-6, 3: 1.93e-6 / 7.6e-7, 32: 1.02e-6 / 4.3e-7; every
  setting's log-probabilities differ from the default's in some bit on both engines
  max |prob - exp(max ref logp)| 1.7e-7 over all cases; near-ties left out of the action_id comparison: 0 of the windows in every case
  records with a non-zero status after ``features_import`` that follows a clip with a failed crop: 1 before ``pa_features_import``
  set the status of the rows it writes (the stale PA_CROP_BAD_BOX of that clip's row), 0 since
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

from helpers import head_windows as hw

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

BATCHES = {  # name: (grid row, clip frames, clips in the batch, feature seed, a one-pass range across a seam)
    "S7 3x20": (hw.SERVED, 60, 3, 201, (18, 23)),
    "S3 5x2": ("S3 A2 F2", 10, 5, 202, (4, 7)),
}
TIE_PAIRS = ((5, 40), (62, 63))
TIE_CASE = (3, 64, 2, 1, 4, 11, ((1, 11),), 301)   # S, A, F, D, max_batch_frames, clip, ranges, feature seed
TIE_RAISE = 20.0


def _need_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


@pytest.fixture(scope="module")
def eng7():
    """The served head with both fighters (S = 7, A = 63, frame_delta 3, 8 frames per pass, clips of up to 64 frames)."""
    _need_gpu()
    eng = hw.make_engine(hw.GRID[hw.SERVED])
    yield eng
    eng.close()


# -- 1. the grid ------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("name", list(hw.GRID))
def test_head_grid_against_float64(name):
    _need_gpu()
    ms, _ = hw.run_case(hw.GRID[name])
    if hw.GRID[name][1] == 1:  # one class: log-softmax of a single logit
        for m in ms:
            assert m["logp_min"] == 0.0 and m["logp_max"] == 0.0, (m["logp_min"], m["logp_max"])
            assert m["prob_min"] == 1.0 and m["prob_max"] == 1.0, (m["prob_min"], m["prob_max"])
            assert m["action_max"] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("dtype", ["emulated_f32", "bf16"])
def test_served_head_on_the_other_dtypes(dtype):
    """The head is fp32 on all three compute dtypes: the same bar."""
    _need_gpu()
    hw.run_case(hw.GRID[hw.SERVED], dtype)


# -- 2. clip batches --------------------------------------------------------------------------------
def _near_seam(n_frames, L):
    """bool[n_frames - 1]: frame numbers 1 .. n_frames - 1 within 3 of a seam (a multiple of L below n_frames)."""
    f = np.arange(1, n_frames)
    seams = np.arange(L, n_frames, L)
    return (np.abs(f[:, None] - seams[None, :]) <= 3).any(axis=1)


def _batch_case(eng, name):
    row, clip, k, seed, (lo1, hi1) = BATCHES[name]
    S, A, F, D = hw.GRID[row][:4]
    sd = hw.state_dict(S, A)
    feats = hw.make_feats(clip, F, seed)
    ref_b = hw.reference(sd, feats, hw.window_rows(1, clip, S, D, clip, F, batch_of=k))
    ref_p = hw.reference(sd, feats, hw.window_rows(1, clip, S, D, clip, F))
    lp_b, rec_b = hw.import_and_run(eng, feats, 1, clip, batch_of=k)
    hw.check(hw.measure(lp_b, rec_b, ref_b), f"{name}: {k} clips of {clip // k}")
    lp_p, rec_p = hw.import_and_run(eng, feats, 1, clip)
    hw.check(hw.measure(lp_p, rec_p, ref_p), f"{name}: one clip of {clip}")
    near = _near_seam(clip, clip // k)
    d = float(np.abs(lp_b - lp_p)[near].max())
    print(f"{name}: batched and plain differ by {d:.3g} within 3 rows of a seam")
    assert d > 1e-3
    # one pass, same (first frame, count, clip length): only the table key's sub_frames entry tells the two clips apart
    lp_b1, rec_b1 = hw.import_and_run(eng, feats, lo1, hi1, batch_of=k)
    lp_p1, rec_p1 = hw.import_and_run(eng, feats, lo1, hi1)
    lp_b2, rec_b2 = hw.import_and_run(eng, feats, lo1, hi1, batch_of=k)
    for what, lp, rec, ref in (("batched", lp_b1, rec_b1, ref_b), ("plain after batched", lp_p1, rec_p1, ref_p),
                               ("batched after plain", lp_b2, rec_b2, ref_b)):
        hw.check(hw.measure(lp, rec, ref[lo1 - 1:hi1 - 1]), f"{name} [{lo1}, {hi1}) {what}")
    assert float(np.abs(lp_b1 - lp_p1).max()) > 1e-3


@pytest.mark.gpu
def test_clip_batch_of_short_clips_against_the_sampler(eng7):
    """Three clips of 20 frames, shorter than the reach of 27: both clamps of every window are its own clip's."""
    _batch_case(eng7, "S7 3x20")


@pytest.mark.gpu
def test_clip_batch_of_two_frame_clips_against_the_sampler():
    """Five clips of 2 frames, the smallest ``pa_clip_begin_batch`` accepts."""
    _need_gpu()
    eng = hw.make_engine(hw.GRID["S3 A2 F2"])
    try:
        _batch_case(eng, "S3 5x2")
    finally:
        eng.close()


# -- 3. the cached window table ---------------------------------------------------------------------
def _same(a, b):
    return np.array_equal(a[0].view(np.int32), b[0].view(np.int32)) and all(np.array_equal(a[1][k].view(np.int32), b[1][k].view(np.int32))
                                                                            for k in a[1])


@pytest.mark.gpu
def test_cached_window_table(eng7):
    S, A, F, D, _, clip, _, seed = hw.GRID[hw.SERVED]
    feats = hw.make_feats(clip, F, seed)
    first = hw.import_and_run(eng7, feats, 1, clip)
    assert _same(hw.head_range(eng7, 1, clip), first)
    # one pass (3 of the 8 frames a pass holds): the second call finds its own table
    small = hw.head_range(eng7, 30, 33)
    ref = hw.reference(hw.state_dict(S, A), feats, hw.window_rows(30, 33, S, D, clip, F))
    hw.check(hw.measure(*small, ref), "table built for [30, 33)")
    assert _same(hw.head_range(eng7, 30, 33), small)
    # pa_infer_windows writes an identity table into the same buffer and must drop the key
    x = torch.from_numpy(np.random.default_rng(7).integers(0, 256, (1, S, 3, 128, 128)).astype(np.float32) / np.float32(255.0))
    lw = eng7.infer_windows(x).cpu().numpy()
    assert lw.shape == (1, A) and np.isfinite(lw).all()
    assert _same(hw.head_range(eng7, 30, 33), small)
    eng7.infer_windows(x)
    assert _same(hw.head_range(eng7, 1, clip), first)
    assert _same(hw.head_range(eng7, 30, 33), small)
    assert _same(hw.head_range(eng7, 1, clip), first)


# -- 4. ties and records ----------------------------------------------------------------------------
def _tied_state_dict(pair):
    S, A = TIE_CASE[:2]
    sd = dict(hw.state_dict(S, A))
    w, b = sd["model.classifier.2.weight"].copy(), sd["model.classifier.2.bias"].copy()
    lo, hi = pair
    w[hi] = w[lo]
    b[lo] = b[hi] = b[lo] + np.float32(TIE_RAISE)
    sd["model.classifier.2.weight"], sd["model.classifier.2.bias"] = w, b
    return sd


def _tie_reference(pair):
    S, A, F, D, _, clip, ((lo, hi),), seed = TIE_CASE
    feats = hw.make_feats(clip, F, seed)
    sd = _tied_state_dict(pair)
    return sd, feats, hw.reference(sd, feats, hw.window_rows(lo, hi, S, D, clip, F))


@pytest.mark.gpu
@pytest.mark.parametrize("pair", TIE_PAIRS, ids=lambda p: f"{p[0]}-{p[1]}")
def test_equal_logits_take_the_lower_index(pair):
    """Two classes with identical ``classifier.2`` rows and biases, raised above every other class: their device logits are the
    same bits, so are their log-probabilities, and ``action_id`` is the lower index in every window."""
    _need_gpu()
    sd, feats, ref = _tie_reference(pair)
    (lo, hi), = TIE_CASE[6]
    eng = hw.make_engine(TIE_CASE, sd=sd)
    try:
        lp, rec = hw.import_and_run(eng, feats, lo, hi)
    finally:
        eng.close()
    err = float(np.abs(lp.astype(np.float64) - ref).max())
    print(f"tie {pair}: max |dlogp| = {err:.3g}")
    assert err <= hw.BAR
    assert np.array_equal(lp[..., pair[0]].view(np.int32), lp[..., pair[1]].view(np.int32))
    assert (lp.argmax(axis=-1) == pair[0]).all() and (lp.max(axis=-1) == lp[..., pair[0]]).all()
    assert (rec["action_id"] == pair[0]).all(), rec["action_id"]
    assert float(np.abs(rec["prob"].astype(np.float64) - np.exp(ref.max(axis=-1))).max()) <= hw.PROB_BAR


def _status_clip():
    """12 frames of 128 x 128 with 64-pixel boxes that the padded square crop keeps inside the frame; the box of (frame 5,
    fighter 1) is not a box."""
    from playaid_core_amd import synth

    n = 12
    frames = synth.make_frames(n, 128, 128, seed=9)
    boxes = np.zeros((n, 2, 4))
    for i in range(n):
        boxes[i, 0] = (0.5, 0.5, 0.5 + i / 1024.0, 0.5)
        boxes[i, 1] = (0.5, 0.5, 0.5, 0.5 - i / 1024.0)
    boxes[5, 1] = np.nan
    return frames, boxes


@pytest.mark.gpu
def test_record_status_is_the_middle_frames_and_zero_after_an_import(eng7):
    """The record of frame number i + 1 carries the crop status of cache row i (the window's middle slot), not of a side slot;
    rows that ``pa_features_import`` writes carry no crop and report 0, whatever an earlier clip left in the cache."""
    from playaid_core_amd import _lib

    frames, boxes = _status_clip()
    n = frames.shape[0]
    out = eng7.infer_clip(frames, boxes)
    want = np.zeros((n, 2), np.int32)
    want[5, 1] = _lib.PA_CROP_BAD_BOX
    assert np.array_equal(out["crop_status"], want), out["crop_status"]
    assert np.array_equal(out["status"], out["crop_status"][:n - 1])
    # frame numbers 3 and 9 read row 5 in a side slot (their +-3 slots) only
    assert out["status"][2, 1] == 0 and out["status"][8, 1] == 0 and out["status"][5, 1] != 0
    feats = hw.make_feats(n, 2, 401)
    lp, rec = hw.import_and_run(eng7, feats, 1, n)
    stale = int((rec["status"] != 0).sum())
    print(f"records with a non-zero status after features_import: {stale}")
    S, A, F, D = hw.GRID[hw.SERVED][:4]
    hw.check(hw.measure(lp, rec, hw.reference(hw.state_dict(S, A), feats, hw.window_rows(1, n, S, D, n, F))), "after an import")


# -- 5. PA_HEAD_SPLITK (children) -------------------------------------------------------------------
_CHILDREN = {"dead": None, "results": {}}


def _child(setting):
    """One child per setting, run once; after a child that ended badly nothing further is started."""
    if setting in _CHILDREN["results"]:
        return _CHILDREN["results"][setting]
    if _CHILDREN["dead"] is not None:
        pytest.fail(f"not started: the PA_HEAD_SPLITK={_CHILDREN['dead']} child ended badly before")
    env = dict(os.environ)
    env.pop("PA_HEAD_SPLITK", None)
    if setting != "unset":
        env["PA_HEAD_SPLITK"] = setting
    _CHILDREN["dead"] = setting  # until it has come back clean
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "head_splitk_worker.py")],
                       capture_output=True, text=True, env=env, timeout=600)
    assert r.returncode == 0, f"PA_HEAD_SPLITK={setting}: exit {r.returncode}\n{r.stdout[-3000:]}\n{r.stderr[-3000:]}"
    _CHILDREN["dead"] = None
    res = json.loads(r.stdout.strip().splitlines()[-1])
    _CHILDREN["results"][setting] = res
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("setting", ["unset", "1", "3", "32"])
def test_head_splitk_settings_against_float64(setting):
    """1: no split, the igemm's direct bias + ReLU epilogue and ``head_mlp_kernel``'s ``h1`` branch; 3: 75 / 75 / 74 k-steps at
    S = 7 and 11 / 11 / 10 at S = 1; 32: 7 k-steps per split at S = 7, one at S = 1. Each meets the bar, and each sums in another
    order than the default (16 splits at S = 7, 4 at S = 1), so its log-probabilities differ from the default's in some bit."""
    _need_gpu()
    base = _child("unset")
    res = _child(setting)
    for name, v in res.items():
        print(f"PA_HEAD_SPLITK={setting} {name}: {v['windows']} windows, max |dlogp| = {v['err']:.3g}, near-ties {v['skipped']:.4f}, "
              f"{'same bits as' if v['sha256'] == base[name]['sha256'] else 'differs from'} the default")
        assert v["err"] <= hw.BAR and v["prob_err"] <= hw.PROB_BAR and v["skipped"] <= hw.TIE_CAP
        if setting != "unset":
            assert v["sha256"] != base[name]["sha256"], f"PA_HEAD_SPLITK={setting} {name}: the same bits as the default"


# -- 6. the comparator itself (CPU) -----------------------------------------------------------------
def _frames_with(f, S, D, lo_clamp, hi_clamp, late_slot=None):
    mid = S // 2
    out = [max(f - D * (mid - t) ** 2, lo_clamp) if t <= mid else min(f + D * (mid - t) ** 2, hi_clamp) for t in range(S)]
    if late_slot is not None:
        out[late_slot] += 1
    return out


def _rows_with(lo, hi, S, D, F, **kw):
    fn = np.array([_frames_with(f, S, D, **kw) for f in range(lo, hi)])
    return (fn[:, None, :] - 1) * F + np.arange(F)[None, :, None]


def test_bar_rejects_named_faults():
    """On the served case's inputs every named fault, computed in float64, moves some log-probability by at least 3 x the bar."""
    S, A, F, D, _, clip, _, seed = hw.GRID[hw.SERVED]
    sd = hw.state_dict(S, A)
    feats = hw.make_feats(clip, F, seed)
    rows = hw.window_rows(1, clip, S, D, clip, F)
    assert np.array_equal(rows, _rows_with(1, clip, S, D, F, lo_clamp=1, hi_clamp=clip - 1))
    ref = hw.reference(sd, feats, rows)
    x = hw.gather_x(feats, rows)

    # the Conv1d's K axis is (slot, 1024 columns) in steps of 32; 16 splits of 14 steps
    step = np.arange(S)[:, None] * 32 + np.arange(1000)[None, :] // 32
    x_drop = x * torch.from_numpy(((step < 9 * 14) | (step >= 10 * 14)).astype(np.float64))[None]
    sd_b1 = dict(sd)
    sd_b1["model.cnn1d.0.bias"] = sd["model.cnn1d.0.bias"] * np.float32(16)
    with torch.no_grad():
        logits = hw.cnn.head_logits(x, sd).numpy()
    mx = logits.max(axis=1, keepdims=True)
    lane_out = logits - mx - np.log(np.exp(logits - mx)[:, :A - 1].sum(axis=1, keepdims=True))   # the 63rd class's lane

    _, bclip, k, bseed, _ = BATCHES["S7 3x20"]
    bfeats = hw.make_feats(bclip, F, bseed)
    bref = hw.reference(sd, bfeats, hw.window_rows(1, bclip, S, D, bclip, F, batch_of=k))

    faults = {
        "fighter rows swapped": (hw.reference(sd, feats, rows ^ 1), ref),
        "upper clamp at max_frames": (hw.reference(sd, feats, _rows_with(1, clip, S, D, F, lo_clamp=1, hi_clamp=clip)), ref),
        "lower clamp at 0": (hw.reference(sd, feats, _rows_with(1, clip, S, D, F, lo_clamp=0, hi_clamp=clip - 1)), ref),
        "slot 1 read one frame late": (hw.reference(sd, feats, _rows_with(1, clip, S, D, F, lo_clamp=1, hi_clamp=clip - 1, late_slot=1)),
                                       ref),
        "batched clip clamped to the whole clip": (hw.reference(sd, bfeats, hw.window_rows(1, bclip, S, D, bclip, F)), bref),
        "split 9 of 16 left out of the reduce": (hw.logp_of_x(x_drop, sd).reshape(ref.shape), ref),
        "b1 added once per split": (hw.logp_of_x(x, sd_b1).reshape(ref.shape), ref),
        "last class's lane left out of the softmax sum": (lane_out.reshape(ref.shape), ref),
    }
    for what, (bad, good) in faults.items():
        d = float(np.abs(bad - good).max())
        print(f"{what}: moves logp by {d:.3g} = {d / hw.BAR:.3g} x the bar")
        assert d >= 3 * hw.BAR, f"{what}: only {d / hw.BAR:.2f} x the bar"


def test_first_argmax_and_decided():
    """The helper's own argmax rule is the first index among equal maxima, at either end of the row and in the middle; a pair
    closer than 2 x the bar is left out of the action comparison, a clear one is not."""
    lp = np.log(np.array([[0.3, 0.3, 0.2, 0.2], [0.1, 0.4, 0.1, 0.4], [0.1, 0.2, 0.35, 0.35], [0.25, 0.25, 0.25, 0.25]]))
    assert hw.first_argmax(lp).tolist() == [0, 1, 2, 0]
    assert hw.first_argmax(lp.reshape(2, 2, 4)).tolist() == [[0, 1], [2, 0]]
    assert hw.first_argmax(np.zeros((3, 1))).tolist() == [0, 0, 0]
    near = np.array([[-1.0, -1.0 - 1.9e-5, -3.0], [-1.0, -1.0 - 2.1e-5, -3.0]])
    assert hw.decided(near).tolist() == [False, True]
    assert hw.decided(np.zeros((2, 1))).all()
    rec = {"action_id": np.array([[1], [0]]), "char_id": np.full((2, 1), hw.CLASS_IDS[0]), "prob": np.exp(near.max(axis=1))[:, None],
           "status": np.zeros((2, 1), np.int32)}
    m = hw.measure(near[:, None, :].astype(np.float32), rec, near[:, None, :])
    assert m["action_wrong"] == 0 and m["skipped"] == 0.5   # the near-tie's other index passes, the clear row is compared
    rec["action_id"] = np.array([[0], [1]])
    assert hw.measure(near[:, None, :].astype(np.float32), rec, near[:, None, :])["action_wrong"] == 1


def test_sampler_per_clip_is_the_kernels_arithmetic():
    """``window_rows`` (the reference sampler, per clip of a batch, seam rows ``j = L`` included) equals a line-by-line model of
    ``window_gather_kernel`` for every S the engine accepts a test runs, frame_delta 1..3, one to four fighters, whole clips and
    passes that start inside them."""
    windows = 0
    for si, S in enumerate((1, 3, 5, 7, 9, 15)):
        for D in (1, 2, 3):
            F = 1 + (si + D) % 4
            for clip, k, f0, cnt in ((23, 0, 1, 22), (23, 0, 9, 5), (70, 0, 1, 69), (10, 5, 1, 9), (60, 3, 1, 59), (60, 3, 18, 5),
                                     (28, 4, 1, 27), (2, 1, 1, 1)):
                got = hw.kernel_rows(f0, cnt, F, S, D, clip, clip // k if k else 0)
                want = hw.window_rows(f0, f0 + cnt, S, D, clip, F, batch_of=k)
                assert np.array_equal(got, want.reshape(-1)), (S, D, F, clip, k, f0, cnt)
                assert want.min() >= 0 and want.max() < clip * F
                windows += cnt * F
    print(f"{windows} windows, no mismatch")


def test_seeds_stay_under_the_tie_cap_and_fp32_under_the_bar():
    """For every case a GPU test runs: the share of windows whose reference top two are closer than 2 x the bar is under the cap,
    and torch's own fp32 head is within a third of the bar of float64 (a correct fp32 kernel that sums in another order keeps the
    other two thirds)."""
    cases = {name: (c, 0, c[5], c[6]) for name, c in hw.GRID.items()}
    cases["knob child S1"] = (hw.SPLITK_S1, 0, hw.SPLITK_S1[5], hw.SPLITK_S1[6])
    for name, (row, clip, k, seed, _) in BATCHES.items():
        cases[name] = (hw.GRID[row][:7] + (seed,), k, clip, ((1, clip),))
    for name, (case, k, clip, ranges) in cases.items():
        S, A, F, D = case[:4]
        sd = hw.state_dict(S, A)
        feats = hw.make_feats(clip, F, case[7])
        for lo, hi in ranges:
            rows = hw.window_rows(lo, hi, S, D, clip, F, batch_of=k)
            ref = hw.reference(sd, feats, rows)
            skipped = float(1.0 - hw.decided(ref).mean())
            with torch.no_grad():
                lp32 = torch.log_softmax(hw.cnn.head_logits(hw.gather_x(feats, rows).float(), sd), dim=1).numpy().reshape(ref.shape)
            e32 = float(np.abs(lp32.astype(np.float64) - ref).max())
            print(f"{name} [{lo}, {hi}): near-ties {skipped:.4f}, torch fp32 within {e32:.3g}")
            assert skipped <= hw.TIE_CAP
            assert e32 <= hw.BAR / 3
    for pair in TIE_PAIRS:
        _, _, ref = _tie_reference(pair)
        assert float(np.abs(ref[..., pair[0]] - ref[..., pair[1]]).max()) <= 1e-12
        rest = np.delete(ref, pair, axis=-1).max()
        print(f"tie {pair}: the pair at {ref[..., pair[0]].max():.4f}, the best other class at {rest:.3f}")
        assert rest < -1.0
