"""Every kernel that reads frames, on frames that are not 16:9 landscape with a width that is a multiple of 16.

The other GPU tests hand the library 270 x 480, 360 x 640, 720 x 1280 or 1080 x 1920 frames; with a width that is a multiple of
4 every row of a slice starts at the same byte offset inside its dword and every frame of a batch starts dword-aligned, a 16:9
frame is letter-boxed with top and bottom borders only, and ``scale_boxes`` never subtracts a horizontal pad. Here:

1. the crop stage (``crop_plan_kernel`` / ``crop_fused_kernel`` / the multi-pass fallback, ``slice_upload_kernel``) on the case
   lists of tests/helpers/frame_geometry.py -- seven frame sizes whose row pitch takes every residue mod 4, batches of seven
   different frames -- bit-exact against ``oracle.yolo_crop.square_crop``, status included; what the lists cover is asserted on
   the CPU (classes of the classifier there, the 16 (pitch, first column) shift pairs, edges and corners, the end of the frame
   buffer), and the geometry the library refuses is an explicit list with the status derived from the class;
2. the fused kernel's LDS tiers: the same lists in a child process per ``PA_FUSED_LDS`` budget, bit-identical to the default;
3. ``letterbox_kernel``: the detector's model input, bitwise ``oracle.yolov5.letterbox``, over left / right and unequal borders,
   enlarging, the copy branch, on the three compute dtypes;
4. ``detect_nms_kernel`` and its 80-class twin with ``pad_x != 0`` against ``oracle.detect.detect_frame``, rows compared as
   uint32 and label text byte for byte, boxes inside the grey border included (they clip to zero width and stay);
5. ``pa_save_one_box_crops`` and ``pa_crop_resize_width`` on 719 x 1277 and 853 x 481 frames;
6. ``infer_clip`` on a 481 x 854 and on a portrait 853 x 481 clip against ``oracle.pipeline``.

Every bar is bit-exactness, or one the project already states (LOGP_TOL = 1e-4 on log-probabilities).
"""
import collections
import os
import subprocess
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import detector_layers as dl  # noqa: E402
from helpers import frame_geometry as fg  # noqa: E402

from oracle import detect as odet  # noqa: E402
from oracle import resample  # noqa: E402
from oracle import yolo_crop  # noqa: E402
from playaid_core_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOGP_TOL = 1e-4
F32 = np.float32


# =====================================================================================================================
# CPU: what the case lists cover
# =====================================================================================================================
def _classes():
    out = collections.Counter()
    for fi, (H, W) in enumerate(fg.FRAMES):
        for box, pad in fg.crop_cases(fi):
            out[fg.classify(box, H, W, pad)] += 1
    return out


def test_frame_sizes_take_every_row_and_frame_alignment():
    assert set(fg.FRAMES) >= {(1080, 1920), (719, 1277), (481, 854), (853, 481), (480, 640), (360, 643), (203, 317)}
    assert {(3 * w) % 4 for _, w in fg.FRAMES} == {0, 1, 2, 3}
    assert sum((3 * h * w) % 4 != 0 for h, w in fg.FRAMES) >= 2
    assert any(h > w for h, w in fg.FRAMES)
    # a batch of BATCH_FRAMES frames has a size that is not a multiple of 4 wherever one frame's is not
    assert all((fg.BATCH_FRAMES * 3 * h * w) % 4 != 0 for h, w in fg.FRAMES if (3 * h * w) % 4 != 0) and fg.BATCH_FRAMES >= 4


def test_sides_that_give_127_rows():
    sides = fg.rows127_sides()
    assert len(sides) == 96
    assert sides[:16] == [49, 98, 103, 107, 161, 187, 196, 197, 206, 214, 237, 239, 249, 253, 322, 347]


def test_case_list_covers_every_class():
    """Every (slice shape, INTER_AREA branch) pair at least twice, 127-row crops in every slice shape, the three paddings.
    Prints the classes with their case counts."""
    cnt = _classes()
    assert all(len(c) == 3 for c in cnt), [c for c in cnt if len(c) != 3]
    pairs, rows127 = collections.Counter(), collections.Counter()
    for (shape, branch, rows), v in cnt.items():
        assert rows in (127, 128)
        pairs[(shape, branch)] += v
        rows127[shape] += v * (rows == 127)
    for (shape, branch, rows), v in sorted(cnt.items()):
        print(f"{shape:7s} {branch:9s} {rows}: {v}")
    print("cases:", sum(cnt.values()))
    for shape in fg.SHAPES:
        for branch in fg.BRANCHES:
            assert pairs[(shape, branch)] >= 2, (shape, branch, pairs[(shape, branch)])
        assert rows127[shape] >= 1, shape
    pads = collections.Counter(pad for fi in range(len(fg.FRAMES)) for _, pad in fg.crop_cases(fi))
    assert set(pads) == {30, 0, 7} and min(pads.values()) >= 100
    # the list is the same list every time it is built
    fg._CASES.clear()
    assert _classes() == cnt


def test_case_list_covers_every_row_shift():
    """All 16 pairs ((3 W) mod 4, (3 x0) mod 4): the shift of a slice's first row, and how it moves from row to row."""
    seen = collections.Counter()
    for fi, (H, W) in enumerate(fg.FRAMES):
        for box, pad in fg.crop_cases(fi):
            seen[fg.row_shifts(box, H, W, pad)] += 1
    assert set(seen) == {(a, b) for a in range(4) for b in range(4)}, sorted(seen)
    print(sorted(seen.items()))


def test_case_list_covers_edges_corners_and_the_end_of_the_buffer():
    for fi, (H, W) in enumerate(fg.FRAMES):
        cases = fg.crop_cases(fi)
        clips = collections.Counter("".join(sorted(fg.geometry(box, H, W, pad)["clip"])) for box, pad in cases)
        for edge in ("L", "R", "T", "B", "LT", "RT", "BL", "BR", ""):
            assert clips[edge] >= 1, (H, W, edge, dict(clips))
        # every case has exactly one slot; in every padding's first call the last frame holds a slice that ends on the last
        # row and the last column of the frame: the last bytes of the frame buffer
        where = fg.slot_of(fi)
        assert sorted(where) == list(range(len(cases)))
        enders = collections.Counter()
        for i, (box, pad) in enumerate(cases):
            if fg._ends_on_last_byte(box, H, W, pad) and where[i][1] == fg.BATCH_FRAMES - 1:
                enders[pad] += 1
        assert all(enders[pad] >= 1 for pad in fg.PADDINGS), (H, W, dict(enders))
        for pad, slots in fg.batches(fi):
            assert slots.shape == (fg.BATCH_FRAMES, fg.FIGHTERS)
            assert all(cases[int(i)][1] == pad for i in slots.reshape(-1) if i >= 0)


def test_the_oracle_accepts_every_case():
    """The cap: no case of the list is refused (those are the explicit list below), so none can drop out at run time."""
    n = 0
    for fi in range(len(fg.FRAMES)):
        ok, crops = fg.expected(fi)
        assert ok.all(), (fg.FRAMES[fi], np.flatnonzero(~ok)[:5])
        assert crops.reshape(len(ok), -1).any(axis=1).mean() > 0.95   # crops of pixels, not black canvases
        n += len(ok)
    assert n >= 900


def test_refused_list():
    """At most 40 refused cases, every stated refusal among them, the expected status from the class; the oracle makes no crop
    of those it can be asked about (the reference raises on a non-finite box)."""
    ref = fg.refused_cases()
    assert 0 < len(ref) <= 40
    seen = collections.Counter()
    for fi, box, pad in ref:
        H, W = fg.FRAMES[fi]
        st = fg.expected_refusal(box, H, W, pad)
        seen[st] += 1
        g = fg.geometry(box, H, W, pad)
        if st == fg.PA_CROP_FILTER_TOO_WIDE:
            # the rule of tests/test_reference_kats.py (_too_wide) agrees; the reference itself would make a crop here
            from test_reference_kats import _too_wide

            assert _too_wide(np.zeros((H, W, 3), np.uint8), box, pad) and g["wrap"]
        elif all(np.isfinite(box)):
            assert not yolo_crop.square_crop(synth.make_frame(0, H, W), box, 128, padding=pad)[0], (fi, box, pad)
    assert set(seen) == {fg.PA_CROP_EMPTY, fg.PA_CROP_BAD_BOX, fg.PA_CROP_FILTER_TOO_WIDE} and min(seen.values()) >= 5


def test_classifier_follows_the_oracle_on_known_slices():
    """The classifier's slice is the oracle's: shape of ``square_crop_pil_stage``'s result, hand-worked classes."""
    H, W = 480, 640
    box = lambda cx, cy, d: fg._box(cx, cy, d, H, W, 2)   # noqa: E731
    assert fg.classify(box(300, 200, 128), H, W, 0) == ("square", "copy", 128)
    assert fg.classify(box(300, 200, 256), H, W, 0) == ("square", "2x2", 128)
    assert fg.classify(box(300, 200, 129), H, W, 0) == ("HV+", "frac", 128)          # 128 x 128 slice enlarged to 129
    assert fg.classify(box(300, 200, 161), H, W, 30) == ("HV-", "frac", 127)         # 220 x 220 shrunk to 161
    assert fg.classify(box(20, 200, 128), H, W, 0) == ("paste", "copy", 128)          # 128 rows x 84 columns: pasted
    assert fg.classify(box(300, 200, 98), H, W, 0) == ("square", "bilinear", 127)
    assert fg.classify(box(900, 200, 98), H, W, 7) == ("empty",)                     # (112 x 0)
    assert fg.classify(box(900, 200, 98), H, W, 0) == ("blank",)                     # (d x 0): a black crop, not a refusal
    assert fg.classify((np.nan, 0.5, 0.1, 0.1), H, W, 0) == ("bad",)
    fr = synth.make_frame(1, H, W)
    for b, pad in [(box(20, 200, 128), 0), (box(300, 200, 161), 30), (box(630, 470, 150), 7), (box(5, 3, 90), 30)]:
        g = fg.geometry(b, H, W, pad)
        cx, cy, cw, ch = yolo_crop.yolo_pixels(*b, W, H)
        half = max(cw, ch) // 2
        raw = fr[max(cy - half - pad, 0): min(cy + half + pad, H), max(cx - half - pad, 0): min(cx + half + pad, W)]
        assert raw.shape[:2] == (g["sh"], g["sw"]) and np.array_equal(raw, fr[g["y0"]:g["y0"] + g["sh"], g["x0"]:g["x0"] + g["sw"]])


def test_letterbox_table_is_the_oracles():
    """The un-padded sizes and borders of the (frame, network input) pairs of part 3, measured on the oracle's output."""
    for frame_hw, net_hw, size, top_left, bottom_right in fg.LETTERBOX:
        assert fg.letterbox_borders(frame_hw, net_hw) == (size, top_left, bottom_right), (frame_hw, net_hw)
    assert fg.letterbox_borders((97, 131), (384, 640))[0][1] > 131   # enlarging
    assert fg.scale_geometry((384, 640), (720, 1280)) == (0.5, 0.0, 12.0)
    gain, pad_x, pad_y = fg.scale_geometry((384, 640), (600, 800))
    assert (gain, pad_x, pad_y) == (0.64, 64.0, 0.0)


def test_oracle_keeps_a_box_inside_the_border_at_zero_width():
    """A candidate right of a 640 x 360 image in the 384 x 640 input (216 columns of image between two 212-column borders)
    clips to x1 = x2 = 360: the label row stays, with zero width."""
    pred = np.zeros((1, 11), F32)
    pred[0, :5] = (500.0, 374.4, 40.0, 19.2, 0.9)
    pred[0, 5 + 3] = 0.8
    rows, text = odet.detect_frame(pred, (384, 640), (640, 360))
    assert text == "3 1 0.975 0 0.05 0.72\n", text


# =====================================================================================================================
# GPU 1: the crop stage
# =====================================================================================================================
_DEV_FRAMES = {}


def _frames_dev(engine, fi):
    import torch

    key = (fi, str(engine.device))
    if key not in _DEV_FRAMES:
        _DEV_FRAMES.clear()     # one frame size at a time on the device
        _DEV_FRAMES[key] = torch.from_numpy(fg.frames(fi)).to(engine.device)
    return _DEV_FRAMES[key]


def _batched(engine, fi, swap_rb=False):
    """Every case of a frame size through ``square_crops``, one call per batch of the layout -> (crops, status) in case order."""
    cases = fg.crop_cases(fi)
    fr = _frames_dev(engine, fi)
    crops = np.zeros((len(cases), 128, 128, 3), np.uint8)
    status = np.full(len(cases), -9, np.int64)
    for pad, slots in fg.batches(fi):
        c, s = engine.square_crops(fr, fg.call_boxes(fi, slots), padding=pad, swap_rb=swap_rb)
        sel = slots >= 0
        crops[slots[sel]] = c[sel]
        status[slots[sel]] = s[sel]
    return crops, status


@pytest.mark.gpu
@pytest.mark.parametrize("fi", range(len(fg.FRAMES)), ids=[f"{h}x{w}" for h, w in fg.FRAMES])
def test_square_crops_batched(engine, fi):
    """``Engine.square_crops``: batches of seven different frames, two boxes each, bit-exact against the oracle."""
    crops, status = _batched(engine, fi)
    bad = fg.first_mismatch(fi, crops, status, "square_crops")
    assert bad is None, bad


def _by_src(engine, fi, order_of):
    """Every case through ``square_crops_src_device``, ONE call per padding, the crops in the order ``order_of(ids)`` and each
    cut from the frame its slot names -> (crops, status) in case order."""
    import torch

    cases, where = fg.crop_cases(fi), fg.slot_of(fi)
    fr = _frames_dev(engine, fi)
    F = engine.F
    crops = np.zeros((len(cases), 128, 128, 3), np.uint8)
    status = np.full(len(cases), -9, np.int64)
    for pad in fg.PADDINGS:
        ids = order_of([i for i, (_, p) in enumerate(cases) if p == pad])
        k = -(-len(ids) // F) * F
        use = list(ids) + [ids[0]] * (k - len(ids))
        boxes = torch.from_numpy(np.array([cases[i][0] for i in use], np.float64)).to(engine.device)
        src = torch.from_numpy(np.array([where[i][1] for i in use], np.int32)).to(engine.device)
        out = torch.empty((k, 128, 128, 3), dtype=torch.uint8, device=engine.device)
        st = engine.square_crops_src_device(fr, boxes, src, k, out, padding=pad, swap_rb=False)
        torch.cuda.synchronize()
        crops[ids] = out.cpu().numpy()[:len(ids)]
        status[ids] = st.cpu().numpy()[:len(ids)]
    return crops, status


@pytest.mark.gpu
@pytest.mark.parametrize("fi", range(len(fg.FRAMES)), ids=[f"{h}x{w}" for h, w in fg.FRAMES])
def test_square_crops_src_shuffled(engine, fi):
    """``Engine.square_crops_src_device`` with a shuffled source index: the same cases, the same bytes."""
    shuffle = lambda ids: list(np.random.default_rng(77 + fi).permutation(ids))   # noqa: E731
    crops, status = _by_src(engine, fi, shuffle)
    bad = fg.first_mismatch(fi, crops, status, "square_crops_src_device (shuffled)")
    assert bad is None, bad


@pytest.mark.gpu
@pytest.mark.parametrize("fi", range(len(fg.FRAMES)), ids=[f"{h}x{w}" for h, w in fg.FRAMES])
def test_square_crops_whole_list_equals_one_by_one(engine, fi):
    """The whole list of a frame size and padding in ONE call equals the same boxes cut one call each (what a crop gives must
    not depend on what shares its launch: LDS left behind, the fallback list, the per-crop scratch)."""
    import torch

    cases, where = fg.crop_cases(fi), fg.slot_of(fi)
    fr = _frames_dev(engine, fi)
    F = engine.F
    crops, status = _by_src(engine, fi, list)
    one = np.zeros_like(crops)
    one_st = np.full(len(cases), -9, np.int64)
    src0 = torch.zeros(F, dtype=torch.int32, device=engine.device)
    out = torch.empty((len(cases), F, 128, 128, 3), dtype=torch.uint8, device=engine.device)
    sts = []
    for i, (box, pad) in enumerate(cases):
        f = where[i][1]
        bx = torch.from_numpy(np.array([box] * F, np.float64)).to(engine.device)
        sts.append(engine.square_crops_src_device(fr[f:f + 1], bx, src0, F, out[i], padding=pad, swap_rb=False))
    torch.cuda.synchronize()
    one[:] = out.cpu().numpy()[:, 0]
    one_st[:] = torch.stack(sts).cpu().numpy()[:, 0]
    bad = fg.first_mismatch(fi, crops, status, "one call for the whole list vs one call per box", want=(one_st, one))
    assert bad is None, bad


@pytest.mark.gpu
def test_refused_geometry_is_refused_with_its_status(engine):
    """The explicit list: the stated status, an all-zero crop, alone and next to a crop that is made."""
    import torch

    for fi, box, pad in fg.refused_cases():
        H, W = fg.FRAMES[fi]
        fr = _frames_dev(engine, fi)
        want = fg.expected_refusal(box, H, W, pad)
        good = fg._box(W // 2, H // 2, 64, H, W, 2)
        boxes = np.array([[box, good], [good, box]], np.float64)
        crops, status = engine.square_crops(fr[-2:], boxes, padding=pad)
        torch.cuda.synchronize()
        assert status[0, 0] == want and status[1, 1] == want, (fi, box, pad, status, want)
        assert not crops[0, 0].any() and not crops[1, 1].any(), (fi, box, pad)
        assert status[0, 1] == 0 and status[1, 0] == 0 and crops[0, 1].any() and crops[1, 0].any()


@pytest.mark.gpu
@pytest.mark.parametrize("fi", [5, 2, 6], ids=["360x643", "481x854", "203x317"])
def test_window_ingest_on_unaligned_frames(engine, fi):
    """``upload_crop_windows`` + ``preprocess_windows`` from pinned host frames of exactly n * H * W * 3 bytes, for the frame
    sizes with (3 W) mod 4 = 1, 2 and 3: crops and status equal the whole-frame call and the oracle. (The ingest runs at the
    engine's own padding and writes RGB: the padding-30 calls, against the oracle's crop with its channels reversed.)"""
    import torch

    from playaid_core_amd import constants

    H, W = fg.FRAMES[fi]
    assert (3 * W) % 4 == {5: 1, 2: 2, 6: 3}[fi] and constants.CROP_PADDING == 30
    cases = fg.crop_cases(fi)
    host = torch.from_numpy(fg.frames(fi)).pin_memory()
    assert host.is_pinned() and host.numel() == fg.BATCH_FRAMES * H * W * 3 and host.is_contiguous()
    n = fg.BATCH_FRAMES
    stage = engine.make_window_stage(n, bytes_per_crop=(3 * W + 16) * H)
    whole_c, whole_s = _batched(engine, fi, swap_rb=True)
    crops = np.zeros((len(cases), 128, 128, 3), np.uint8)
    status = np.full(len(cases), -9, np.int64)
    done = np.zeros(len(cases), bool)
    out = torch.empty((n, engine.F, 128, 128, 3), dtype=torch.uint8, device=engine.device)
    st = torch.empty((n, engine.F), dtype=torch.int32, device=engine.device)
    for pad, slots in fg.batches(fi):
        if pad != constants.CROP_PADDING:
            continue
        boxes = fg.call_boxes(fi, slots)
        engine.upload_crop_windows(host, boxes, stage, padding=pad)
        engine.preprocess_windows(stage, n, H, W, torch.from_numpy(boxes).to(engine.device), 0, out, st)
        torch.cuda.synchronize()
        sel = slots >= 0
        crops[slots[sel]] = out.cpu().numpy()[sel]
        status[slots[sel]] = st.cpu().numpy()[sel]
        done[slots[sel]] = True
    assert done.sum() >= 40
    ok, want = fg.expected(fi)
    rgb = np.ascontiguousarray(want[..., ::-1])
    # the cases of the other paddings are not part of this test: hand them through as equal
    crops[~done], status[~done] = rgb[~done], 0
    bad = fg.first_mismatch(fi, crops, status, "window ingest vs the oracle", want=(np.where(ok, 0, -1), rgb))
    assert bad is None, bad
    whole_c[~done], whole_s[~done] = rgb[~done], 0
    bad = fg.first_mismatch(fi, crops, status, "window ingest vs the whole-frame call", want=(whole_s, whole_c))
    assert bad is None, bad


# =====================================================================================================================
# GPU 2: the fused kernel's LDS tiers
# =====================================================================================================================
LDS_FRAMES = (0, 1)                     # 1080 x 1920 and 719 x 1277 (unaligned rows and frames)
LDS_BUDGETS = ("49152", "24576", "8192", "0")


@pytest.mark.gpu
def test_fused_lds_budgets_give_the_same_bytes(tmp_path):
    """``PA_FUSED_LDS`` moves crops between the fused kernel's sub-band heights (8 / 4 / 2 / 1 output rows) and the multi-pass
    fallback; the budget is read once per process, so every setting is a child of its own (tests/helpers/crop_lds_worker.py),
    one after the other, and the first that ends abnormally ends the test. Every budget gives the default's bytes, and the
    default gives the oracle's.

    Tiers, from ``band_lds`` (csrc/preprocess.hip: B0 source rows + B1 resized rows of the worst sub-band), for an unclipped
    padding-30 slice, as (324-pixel slice, d = 264 | 900-pixel slice, d = 840):
        default 77824: 8 rows (44304 B) | 1 row (62736 B)       49152: 8 rows | fallback
        24576: 2 rows (17728 B) | fallback                        8192: fallback (14176 B for one row) | fallback
        0: every crop on the fallback (sides under 128 pixels are on it under every budget).
    Over the two frame sizes' 402 cases the same arithmetic gives (8 / 4 / 2 / 1 rows / fallback), the 101 sides under 128
    aside: 271 / 16 / 14 / 0 / 0 by default, 229 / 48 / 13 / 11 / 0 at 49152, 181 / 46 / 37 / 21 / 16 at 24576,
    39 / 71 / 53 / 44 / 94 at 8192, 0 / 0 / 0 / 0 / 301 at 0: no two budgets pick the same tiers.
    The fallback's per-crop scratch (t1, t2: ``t_stride`` = a whole frame of the engine's maximum size, one stride per crop of
    ``max_batch_frames * fighters``) holds every crop of a call -- the plan refuses a pass larger than t_stride, and the entry
    refuses a call of more frames than the engine's -- so budget 0 is within the design."""
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")

    def run(budget, name):
        env = dict(os.environ)
        env.pop("PA_FUSED_LDS", None)
        if budget is not None:
            env["PA_FUSED_LDS"] = budget
        path = str(tmp_path / name)
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "crop_lds_worker.py"), path] + [str(f) for f in LDS_FRAMES],
                           capture_output=True, text=True, env=env, timeout=600)
        assert r.returncode == 0, (budget, r.returncode, r.stderr[-2000:])
        return np.load(path)

    default = run(None, "default.npz")
    for fi in LDS_FRAMES:
        bad = fg.first_mismatch(fi, default[f"crops_{fi}"], default[f"status_{fi}"], "default LDS budget vs the oracle")
        assert bad is None, bad
    for budget in LDS_BUDGETS:
        got = run(budget, f"lds_{budget}.npz")
        for fi in LDS_FRAMES:
            bad = fg.first_mismatch(fi, got[f"crops_{fi}"], got[f"status_{fi}"], f"PA_FUSED_LDS={budget} vs the default",
                                    want=(default[f"status_{fi}"], default[f"crops_{fi}"]))
            assert bad is None, bad


# =====================================================================================================================
# GPU 3: the letterbox
# =====================================================================================================================
_LETTERBOX_WANT = {}


def _letterbox_want(k):
    """Three different frames of LETTERBOX[k]'s size and the oracle's letterbox of them, once per module."""
    from oracle import yolov5 as oy

    if k not in _LETTERBOX_WANT:
        (h, w), net = fg.LETTERBOX[k][:2]
        frames = synth.make_frames(3, h, w, seed=50 + k)
        _LETTERBOX_WANT[k] = (frames, np.stack([oy.letterbox(f, net) for f in frames]))
    return _LETTERBOX_WANT[k]


@pytest.mark.gpu
@pytest.mark.parametrize("k", range(len(fg.LETTERBOX)), ids=[f"{f[0]}x{f[1]}_in_{n[0]}x{n[1]}" for f, n, *_ in fg.LETTERBOX])
@pytest.mark.parametrize("dtype", ["f32", "emulated_f32", "bf16"])
def test_letterbox_model_input(dtype, k):
    """The detector's model input (``check_detector``'s first check) on three different frames: border and channel 3 zero, the
    interior bitwise the oracle's letterbox."""
    from playaid_core_amd.yolov5 import YoloV5Detector

    frames, want = _letterbox_want(k)
    net = fg.LETTERBOX[k][1]
    det = YoloV5Detector(synth.make_yolov5s_state_dict(), 6, net, max_images=3, compute_dtype=dtype)
    try:
        dl.check_model_input(det, frames, f"{dtype} {frames.shape[1]}x{frames.shape[2]} in {net[0]}x{net[1]}", idx=np.arange(3), want=want)
    finally:
        det.close()


# =====================================================================================================================
# GPU 4: NMS with pad_x != 0
# =====================================================================================================================
NMS_PAIRS = [((384, 640), (480, 640)), ((384, 640), (640, 360)), ((640, 384), (853, 481)), ((384, 640), (719, 1277)),
             ((384, 640), (97, 131)), ((320, 320), (600, 600))]
_NMS = {}


def _nms_pred(net, img, nc):
    """``tests/test_detect.py``'s random head rows with the centres scaled to the network input, plus, in every frame but the
    last, candidates of the kept classes inside the grey border and across the image's edges (both sides of the clip)."""
    from test_detect import _random_pred

    key = (net, img, nc)
    if key in _NMS:
        return _NMS[key]
    rng = np.random.default_rng(1000 + net[0] + img[1] + nc)
    n, rows = 12, 400
    pred = _random_pred(rng, n, rows, nc=nc)
    pred[..., 0] *= net[1] / 640.0
    pred[..., 1] *= net[0] / 384.0
    gain, pad_x, pad_y = fg.scale_geometry(net, img)
    kept = (2, 3) if nc == 6 else (2, 3, 40, 77)
    for f in range(n - 1):
        x_lo, x_hi, y_lo, y_hi = pad_x, net[1] - pad_x, pad_y, net[0] - pad_y       # the image inside the network input
        cands = [
            (x_hi + pad_x / 2, net[0] * 0.4, max(pad_x * 0.5, 4.0), 30.0),           # inside the right border (or across the right edge)
            (x_lo - pad_x / 2, net[0] * 0.6, max(pad_x * 0.5, 4.0), 24.0),           # inside the left border (or across the left edge)
            (net[1] * 0.3, y_lo - pad_y / 2, 40.0, max(pad_y * 0.5, 4.0)),           # top
            (net[1] * 0.7, y_hi + pad_y / 2, 36.0, max(pad_y * 0.5, 4.0)),           # bottom
            (x_hi - 10.0, y_hi - 8.0, 60.0, 50.0),                                   # across the bottom-right corner
            (x_lo + 6.0, y_lo + 5.0, 44.0, 38.0),                                    # across the top-left corner
        ]
        for j, (cx, cy, w, h) in enumerate(cands):
            r = 20 * j + f
            pred[f, r] = 0
            pred[f, r, :5] = (cx + f, cy + 0.5 * f, w, h, 0.99 - 0.01 * ((j + f) % 6))
            pred[f, r, 5 + kept[(j + f) % len(kept)]] = 0.99
    _NMS[key] = pred
    return pred


@pytest.mark.gpu
@pytest.mark.parametrize("net,img", NMS_PAIRS, ids=[f"{i[0]}x{i[1]}_in_{n[0]}x{n[1]}" for n, i in NMS_PAIRS])
@pytest.mark.parametrize("nc", [6, 80], ids=["pa_detect_postprocess", "pa_detect_postprocess_classes"])
@pytest.mark.parametrize("max_det", [1, 2, 8])
def test_nms_scales_boxes_with_a_horizontal_pad(engine, max_det, nc, net, img):
    """Both NMS entries against ``oracle.detect.detect_frame``: rows as uint32, label text byte for byte. Rows whose box lies in
    the border clip to zero width or height and are kept. At least 10 detections survive and at least one was clipped."""
    from playaid_core_amd import detect as pdet

    pred = _nms_pred(net, img, nc)
    classes = (2, 3) if nc == 6 else (2, 3, 40, 77)     # (80 classes: one in each of the three mask words, two in the first)
    dets, counts = engine.detect_postprocess(pred, net, img, classes=classes, max_det=max_det)
    dets, counts = dets.cpu().numpy(), counts.cpu().numpy()
    gain, pad_x, pad_y = fg.scale_geometry(net, img)
    some = clipped = 0
    for f in range(pred.shape[0]):
        want, text = odet.detect_frame(pred[f], net, img, classes=classes, max_det=max_det)
        assert counts[f] == want.shape[0], (f, counts[f], want.shape[0])
        got = dets[f, : counts[f]]
        assert np.array_equal(got.view(np.uint32), want.view(np.uint32)), (f, got, want)
        assert pdet.label_lines(got) == text
        some += want.shape[0]
        raw = odet.non_max_suppression(pred[f], classes=classes, max_det=max_det)
        x = (raw[:, [0, 2]].astype(np.float64) - pad_x) / gain
        y = (raw[:, [1, 3]].astype(np.float64) - pad_y) / gain
        clipped += int(((x < 0) | (x > img[1])).any(axis=1).sum() + ((y < 0) | (y > img[0])).any(axis=1).sum())
    assert some >= 10 and clipped >= 1, (some, clipped)
    assert counts[-1] == 0


# =====================================================================================================================
# GPU 5: the other frame readers
# =====================================================================================================================
@pytest.mark.gpu
@pytest.mark.parametrize("h,w", [(719, 1277), (853, 481)])
def test_save_one_box_crops_on_unaligned_frames(engine, h, w):
    """``pa_save_one_box_crops`` == ``oracle.detect.save_one_box`` (quality 95) / the raw rectangle (quality 0), the way
    tests/test_savebox.py checks 720p; rows over the right and bottom edges among them."""
    import torch

    from test_savebox import _label_rows

    n = 12
    rng = np.random.default_rng(h)
    frames = synth.make_frames(n, h, w, seed=21)
    dets, counts = _label_rows(rng, n, h, w)
    # boxes over the right and the bottom edge, and over the corner
    for i, (cx, cy, bw, bh) in enumerate([(0.99, 0.98, 0.101, 0.1015), (0.995, 0.4, 0.2, 0.1), (0.3, 0.99, 0.1, 0.15)]):
        dets[i, 0, 1:5] = (cx, cy, bw, bh)
        counts[i] = max(counts[i], 1)
    if (h, w) == (719, 1277):
        assert odet.save_one_box_rect(dets[0, 0], (h, w)) == (1193, 662, 1277, 719)
    fd = torch.from_numpy(frames).to(engine.device)
    dd, cd = torch.from_numpy(dets).to(engine.device), torch.from_numpy(counts).to(engine.device)
    for quality in (95, 0):
        images, desc = engine.save_one_box_crops(fd, dd, cd, jpeg_quality=quality)
        engine.check_device_errors()
        got = engine.unpack_crop_images(images, desc)
        assert len(got) == n * 2
        seen = edge = 0
        for i in range(n):
            for p, cls in enumerate((2, 3)):
                ks = [k for k in range(counts[i]) if int(dets[i, k, 0]) == cls]
                g = got[i * 2 + p]
                if not ks:
                    assert g is None
                    continue
                row = dets[i, ks[0]]
                x1, y1, x2, y2 = odet.save_one_box_rect(row, (h, w))
                if quality:
                    want = odet.save_one_box(row, frames[i], quality)
                else:
                    want = frames[i][y1:y2, x1:x2] if x2 > x1 and y2 > y1 else None
                if want is None:
                    assert g is None
                    continue
                assert g is not None and g.shape == want.shape, (i, p, None if g is None else g.shape, want.shape)
                assert np.array_equal(g, want), (quality, i, p, int(np.abs(g.astype(int) - want).max()))
                seen += 1
                edge += x2 == w or y2 == h
        assert seen > n and edge >= 3


@pytest.mark.gpu
def test_crop_resize_width_on_an_unaligned_frame(engine):
    """``pa_crop_resize_width`` (rect_resize_kernel) on 719 x 1277 frames: rectangles at every x1 mod 4, every INTER_AREA
    branch, one ending on the last pixel of the last frame, against ``oracle.resample.imutils_resize_width``."""
    h, w = 719, 1277
    frames = synth.make_frames(3, h, w, seed=13)
    groups = [
        [(101, 50, 101 + 133, 50 + 60), (102, 300, 102 + 700, 300 + 301), (103, 8, 103 + 512, 8 + 200), (104, 400, 104 + 768, 400 + 99)],
        [(641, 300, 641 + 256, 300 + 64), (w - 133, h - 60, w, h), (w - 601, h - 250, w, h), (0, 0, 255, 77)],
    ]
    assert {r[0] % 4 for g in groups for r in g} == {0, 1, 2, 3}
    branches = set()
    for rects in groups:
        got = engine.crop_resize_width(frames, rects, 256)
        for j, (x1, y1, x2, y2) in enumerate(rects):
            sw = x2 - x1
            branches.add("enlarge" if sw < 256 else "copy" if sw == 256 else "2x2" if sw == 512 else "int" if sw % 256 == 0 else "frac")
            for i in range(3):
                want = resample.imutils_resize_width(frames[i, y1:y2, x1:x2], 256)
                assert got[j][i].shape == want.shape, (rects[j], i)
                assert np.array_equal(got[j][i], want), (rects[j], i)
    assert branches == {"enlarge", "frac", "2x2", "int", "copy"}


# =====================================================================================================================
# GPU 6: end to end
# =====================================================================================================================
_CLIPS = {}


def _clip(n, h, w, state_dict):
    from oracle import pipeline

    if (n, h, w) not in _CLIPS:
        frames, boxes = synth.make_frames(n, h, w), synth.make_boxes(n, h, w)
        _CLIPS[(n, h, w)] = (frames, boxes, pipeline.run_action_recognition(frames, boxes, state_dict, mode="cached"))
    return _CLIPS[(n, h, w)]


@pytest.mark.gpu
@pytest.mark.parametrize("n,h,w", [(30, 481, 854), (20, 853, 481)], ids=["481x854", "853x481_portrait"])
def test_infer_clip_on_unaligned_frames(engine, state_dict, n, h, w):
    frames, boxes, ref = _clip(n, h, w, state_dict)
    got = engine.infer_clip(frames, boxes, want_crops=True)
    assert not got["crop_status"].any()
    assert np.array_equal(got["crops_rgb"], ref["crops_rgb"]), "crop stage is not bit-exact"
    err = float(np.abs(got["logp"].astype(np.float64) - ref["logp"]).max())
    print(f"{h}x{w}: max |dlogp| = {err:.3e}")
    assert err <= LOGP_TOL, err
    assert np.array_equal(got["action_id"], ref["action_id"])
