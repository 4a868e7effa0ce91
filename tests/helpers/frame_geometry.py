"""Case lists and the branch classifier behind tests/test_frame_geometry.py (and its child, tests/helpers/crop_lds_worker.py).

Everything here is derived from the oracle (``oracle/yolo_crop.py``, ``oracle/resample.py``, ``oracle/yolov5.py``), never from
the kernels' plan: the slice of a box (numpy's slice semantics included), Pillow's contain size and bicubic support, and the
INTER_AREA branch ``cv2.resize`` takes for the side ``d``. The lists are deterministic (seeded generators, no clock, no global
RNG): the CPU half of the test asserts what they cover, the GPU half runs them as they stand.

A crop case is ``(box, padding)`` on one frame size. Classes (``classify``):
  * slice shape: ``square`` (the slice is d x d: no Pillow stage), ``paste`` (ImageOps.pad pastes without resizing), and the
    resized ones ``H-  H+  V-  V+  HV-  HV+``: horizontal pass only, vertical only or both, ``+`` when it enlarges
    (``rw > sw or rh > sh``), ``-`` otherwise;
  * INTER_AREA branch: ``copy`` (d == 128), ``2x2`` (d == 256), ``int`` (d in 384, 512, ...), ``frac``, ``bilinear`` (d < 128:
    OpenCV's bilinear emulation);
  * rows: ``int(d * (128 / float(d)))``, 128 or 127 (the second black pad runs only for 127).
Every one of the 8 x 5 (shape, branch) pairs is permitted by the geometry on a frame of at least 512 pixels a side: a frame edge
can clip a slice to any width and height up to ``2 * (d // 2) + 2 * padding``, ``square`` needs (d, d), ``paste`` (s, d) or
(d, s) with s < d, ``H-`` / ``H+`` a wide slice of width d + 1 / d - 1 whose height Pillow's rounding keeps (less than half the
width), ``V-`` / ``V+`` the transpose, ``HV-`` / ``HV+`` anything else, and none of that constrains d.
"""
from __future__ import annotations

import math

import numpy as np

from oracle import resample as R
from oracle import yolo_crop

PA_CROP_OK, PA_CROP_EMPTY, PA_CROP_BAD_BOX, PA_CROP_FILTER_TOO_WIDE = 0, 1, 2, 4

# (3 W) mod 4 = 0, 3, 2, 3, 0, 1, 3; (3 H W) mod 4 = 0, 1, 2, 3, 0, 0, 1; 853 x 481 is portrait
FRAMES = [(1080, 1920), (719, 1277), (481, 854), (853, 481), (480, 640), (360, 643), (203, 317)]
PADDINGS = (30, 0, 7)
FIGHTERS = 2
BATCH_FRAMES = 7          # different frames per call; odd, so that n * H * W * 3 keeps the frame size's residue mod 4
SHAPES = ("square", "paste", "H-", "H+", "V-", "V+", "HV-", "HV+")
BRANCHES = ("copy", "2x2", "int", "frac", "bilinear")
MAX_TAPS = 15             # the library's stated bicubic table (PA_CROP_FILTER_TOO_WIDE beyond it)


def rows127_sides(limit=1200):
    """Sides d whose imutils.resize(width=128) comes out 127 rows high: int(d * (128 / float(d))) == 127."""
    return [d for d in range(1, limit) if int(d * (128 / float(d))) == 127]


def area_branch(d):
    if d < 128:
        return "bilinear"
    if d == 128:
        return "copy"
    if d == 256:
        return "2x2"
    return "int" if d % 128 == 0 else "frac"


def geometry(box, H, W, pad):
    """The slice ``YoloCrop.square_crop`` takes, statement by statement as ``oracle.yolo_crop.square_crop_pil_stage``, or None
    for a box the reference cannot turn into pixels (non-finite) or whose side is not positive."""
    if not all(math.isfinite(float(v)) for v in box):
        return None
    cx, cy, cw, ch = yolo_crop.yolo_pixels(*box, W, H)
    d = max(cw, ch)
    if d <= 0:
        return None
    half = int(d / 2)
    lo_y, hi_y, lo_x, hi_x = cy - half - pad, cy + half + pad, cx - half - pad, cx + half + pad
    ys = range(*slice(max(lo_y, 0), min(hi_y, H)).indices(H))
    xs = range(*slice(max(lo_x, 0), min(hi_x, W)).indices(W))
    sh, sw = len(ys), len(xs)
    return {"d": d, "sh": sh, "sw": sw, "y0": ys.start if sh else 0, "x0": xs.start if sw else 0,
            "wrap": min(hi_y, H) < 0 or min(hi_x, W) < 0,
            "clip": frozenset(e for e, c in (("L", lo_x < 0), ("R", hi_x > W), ("T", lo_y < 0), ("B", hi_y > H)) if c)}


def classify(box, H, W, pad):
    """-> ("bad",) | ("empty",) | ("blank",) | ("too_wide",) | (shape, branch, rows)."""
    g = geometry(box, H, W, pad)
    if g is None:
        return ("bad",)
    d, sh, sw = g["d"], g["sh"], g["sw"]
    if sh == 0 or sw == 0:
        # a (d x 0) slice is pasted as a black canvas (Pillow skips the resize); every other empty slice has no crop
        return ("blank",) if (sw == 0 and sh == d) else ("empty",)
    if (sh, sw) == (d, d):
        shape = "square"
    else:
        rw, rh = R.pil_contain_size(sw, sh, (d, d))
        if rw <= 0 or rh <= 0:
            return ("empty",)
        ks = [2 * math.ceil(2 * max(i / o, 1.0)) + 1 for i, o, need in ((sw, rw, rw != sw), (sh, rh, rh != sh)) if need]
        if max(ks, default=0) > MAX_TAPS:
            return ("too_wide",)
        if rw == sw and rh == sh:
            shape = "paste"
        else:
            shape = "H" * (rw != sw) + "V" * (rh != sh) + ("+" if (rw > sw or rh > sh) else "-")
    return (shape, area_branch(d), int(d * (128 / float(d))))


def expected_refusal(box, H, W, pad):
    """The status the library states for a geometry it refuses (include/playaid_hip.h), from the class alone."""
    return {"bad": PA_CROP_BAD_BOX, "empty": PA_CROP_EMPTY, "too_wide": PA_CROP_FILTER_TOO_WIDE}[classify(box, H, W, pad)[0]]


def row_shifts(box, H, W, pad):
    """((3 W) mod 4, (3 x0) mod 4): how the byte address of a slice row moves from row to row, and where its first row starts."""
    return (3 * W) % 4, (3 * geometry(box, H, W, pad)["x0"]) % 4


# -- building boxes from pixels ---------------------------------------------------------------------------------------
def _norm(c, size):
    """A normalised coordinate whose ``int(c * size)`` is the pixel c (int() truncates towards zero)."""
    return (c + 0.4) / size if c >= 0 else (c - 0.4) / size


def _box(cx, cy, d, H, W, k):
    """Centre pixel (cx, cy), larger side d; the shorter side and which one it is follow the counter k."""
    other = max(int(d * (0.6, 0.75, 1.0)[k % 3]), 1)
    bw, bh = (other, d) if k % 2 else (d, other)
    return (_norm(cx, W), _norm(cy, H), (bw + 0.5) / W, (bh + 0.5) / H)


def _centre(span, d, pad, size, high, inside_at):
    """The centre pixel whose slice along an axis of ``size`` pixels is ``span`` long: the unclipped length when it fits
    (placed at ``inside_at``), else clipped at the high or the low end of the axis. None when impossible."""
    half = d // 2
    full = 2 * half + 2 * pad
    if span > min(full, size) or span < 1:
        return None
    if span == full:
        return half + pad + min(inside_at, size - full)
    return size - span + half + pad if high else span - half - pad


def _targets(shape, d, full):
    """(sw, sh) candidates that give the slice shape for side d (checked with ``classify`` by the caller)."""
    thin = lambda s: max((s // 2) - 2, 1)   # noqa: E731  Pillow's rounding keeps the short side: |short / long| < 1 / 2
    return {
        "square": [(d, d)],
        "paste": [(d - max(d // 3, 1), d), (d, d - max(d // 4, 1))],
        "H-": [(d + 1, thin(d + 1))],
        "H+": [(d - 1, thin(d - 1))],
        "V-": [(thin(d + 1), d + 1)],
        "V+": [(thin(d - 1), d - 1)],
        "HV-": [(full, full), (d + 5, d + 9)],
        "HV+": [(d - 3, d - 2), (d - 7, d - 1)],
    }[shape]


_BRANCH_SIDES = {"copy": [128], "2x2": [256], "int": [384, 512], "frac": [200, 333, 161, 140], "bilinear": [64, 100, 98, 33]}


def _aimed(H, W, k0):
    """One case per (shape, branch) the frame can hold, and one 127-row case per shape."""
    out, k = [], k0
    r127 = set(rows127_sides())
    wanted = [(s, b, False) for s in SHAPES for b in BRANCHES] + [(s, None, True) for s in SHAPES]
    for shape, branch, want127 in wanted:
        sides = [d for d in (196, 98, 322, 161, 206, 103)] if want127 else _BRANCH_SIDES[branch]
        found = False
        for d in sides:
            if d > min(H, W) or found:
                continue
            for j in range(3):
                pad = PADDINGS[(k + j) % 3]
                full = 2 * (d // 2) + 2 * pad
                for sw, sh in _targets(shape, d, full):
                    cx = _centre(sw, d, pad, W, high=bool((k >> 1) & 1), inside_at=37 + k % 4)
                    cy = _centre(sh, d, pad, H, high=bool(k & 1), inside_at=11 + k % 5)
                    if cx is None or cy is None:
                        continue
                    box = _box(cx, cy, d, H, W, k)
                    cl = classify(box, H, W, pad)
                    if cl[0] == shape and (cl[2] == 127 and d in r127 if want127 else cl[1] == branch):
                        out.append((box, pad))
                        k += 1
                        found = True
                        break
                if found:
                    break
    return out


def _swept(H, W, rng):
    """Sides x places: the centre, the four edges, the four corners and a random place, the first column of the slice walked
    through every residue mod 4, the three paddings and three aspect ratios in turn."""
    out = []
    sides = [24, 64, 127, 128, 129, 256, 384, 512, 49, 98, 103, 107, 161, 187, 196, 197, 322, 347]
    sides += [int(rng.uniform(130, 0.9 * min(H, W))) for _ in range(3)]
    spots = [(0.5, 0.5), (0.0, 0.5), (1.0, 0.5), (0.5, 0.0), (0.5, 1.0), (0.01, 0.02), (0.99, 0.985), (0.03, 0.97), (0.98, 0.02)]
    k = 0
    for side in sides:
        if side > min(H, W):
            continue
        for (px, py) in spots[: 9 if side in (64, 128, 129, 161, 256) else 4] + [(float(rng.random()), float(rng.random()))]:
            asp = (0.6, 0.75, 1.0)[k % 3]
            bw, bh = ((int(side * asp) + 0.5), side + 0.5) if k % 2 else (side + 0.5, int(side * asp) + 0.5)
            cxp = px * W + (k % 4) + 0.3
            out.append(((cxp / W, (py * H + 0.4) / H, bw / W, bh / H), PADDINGS[k % 3]))
            k += 1
    # the untouched squares: padding 0, even side, inside the frame (copy and 2x2 among them), at every column residue
    for j, d in enumerate([128, 256, 128, 256, 384, 200, 98, 196]):
        if d + 8 <= min(H, W):
            out.append((_box(d // 2 + 5 + j, d // 2 + 3 + j, d, H, W, 2), 0))
    # slices that end on the frame's last row and last column, at the three paddings
    for j, d in enumerate([150, 129, 90]):
        out.append((_box(W - d // 2 + j, H - d // 2 + 1, d, H, W, 2), PADDINGS[j]))
    return out


def _random(H, W, rng, count):
    out = []
    while len(out) < count:
        d = int(rng.integers(20, min(H, W)))
        box = _box(int(rng.integers(-d // 3, W + d // 3)), int(rng.integers(-d // 3, H + d // 3)), d, H, W, int(rng.integers(0, 6)))
        pad = PADDINGS[int(rng.integers(0, 3))]
        if len(classify(box, H, W, pad)) == 3:
            out.append((box, pad))
    return out


_CASES = {}


def crop_cases(fi):
    """The accepted crop cases of frame size FRAMES[fi]: [(box, padding)], every one a crop the oracle makes."""
    if fi not in _CASES:
        H, W = FRAMES[fi]
        rng = np.random.default_rng(2024 + fi)
        cases = _swept(H, W, rng)
        cases += _aimed(H, W, len(cases))
        cases += _random(H, W, rng, 12)
        _CASES[fi] = cases
    return _CASES[fi]


def refused_cases():
    """[(frame size index, box, padding)]: geometry the library refuses, at most 40 cases; the expected status comes from
    ``expected_refusal``. Empty slices (off the frame to the right and below, a (0 x d) slice), boxes that are not
    finite or have no side, slices that a Pillow pass would shrink by more than its 15 taps allow (most of them the
    negative-stop wraps of a box above or left of the frame, which keep nearly the whole frame column or row)."""
    out = []
    for fi in (0, 1, 3, 5, 6):
        H, W = FRAMES[fi]
        d = min(H, W) // 4
        out += [
            (fi, _box(W + d + 40, H // 2, d, H, W, 0), 30),                    # right of the frame: (sh x 0), sh != d
            (fi, _box(W // 2, H + d + 40, d, H, W, 1), 7),                     # below the frame: (0 x sw)
            (fi, _box(W // 2 + 1, H + d // 2 + 1, d - d % 2, H, W, 2), 0),     # (0 x d): Pillow divides by zero
            (fi, (float("nan"), 0.5, 0.2, 0.3), 30),
            (fi, (0.5, 0.5, float("inf"), 0.3), 0),
            (fi, (0.5, 0.5, 0.0, 0.0), 30),                                    # no side
            (fi, _box(W // 2, -(d // 2) - 40, d, H, W, 0), 30),                # above: the stop wraps, nearly every row kept
            (fi, _box(-(d // 2) - 12, H // 2, d, H, W, 1), 7),                 # left: nearly every column kept
        ]
    return out


# -- batches ----------------------------------------------------------------------------------------------------------
def batches(fi):
    """The cases of a frame size as calls of BATCH_FRAMES frames x FIGHTERS boxes: [(padding, slots)], slots an int array
    [BATCH_FRAMES, FIGHTERS] of case indices (-1: unused, filled with the call's first case). A case keeps its slot in every
    test, so its oracle crop is computed once. Slices that end on the frame's last row and last column go to the LAST frame of
    a call first (one call after the other), so that the last bytes of the frame buffer are read at several widths."""
    H, W = FRAMES[fi]
    cases = crop_cases(fi)
    per = BATCH_FRAMES * FIGHTERS
    out = []
    for pad in PADDINGS:
        ids = [i for i, (_, p) in enumerate(cases) if p == pad]
        enders = [i for i in ids if _ends_on_last_byte(cases[i][0], H, W, pad)]
        calls = -(-len(ids) // per)
        slots = np.full((calls, BATCH_FRAMES, FIGHTERS), -1, np.int64)
        tail = enders[:calls * FIGHTERS]
        for j, i in enumerate(tail):
            slots[j % calls, BATCH_FRAMES - 1, j // calls] = i
        rest = iter([i for i in ids if i not in set(tail)])
        flat = slots.reshape(-1)
        for j in range(flat.size):
            if flat[j] < 0:
                flat[j] = next(rest, -1)
        out += [(pad, slots[c]) for c in range(calls)]
    return out


def _ends_on_last_byte(box, H, W, pad):
    g = geometry(box, H, W, pad)
    return g is not None and g["sh"] > 0 and g["sw"] > 0 and not g["wrap"] and g["y0"] + g["sh"] == H and g["x0"] + g["sw"] == W


def slot_of(fi):
    """case index -> (call, frame of the batch, fighter)."""
    out = {}
    for c, (_, slots) in enumerate(batches(fi)):
        for f in range(BATCH_FRAMES):
            for p in range(FIGHTERS):
                if slots[f, p] >= 0:
                    out[int(slots[f, p])] = (c, f, p)
    return out


_FRAMES, _EXPECTED = {}, {}


def frames(fi):
    """The BATCH_FRAMES different frames of a frame size (uint8[BATCH_FRAMES, H, W, 3])."""
    from playaid_core_amd import synth

    if fi not in _FRAMES:
        H, W = FRAMES[fi]
        _FRAMES[fi] = synth.make_frames(BATCH_FRAMES, H, W, seed=31 + fi)
    return _FRAMES[fi]


def expected(fi):
    """(ok bool[k], crops uint8[k, 128, 128, 3]) of ``oracle.yolo_crop.square_crop`` for every case, each on the frame of
    the batch its slot names. Computed once per process."""
    if fi not in _EXPECTED:
        cases, where, fr = crop_cases(fi), slot_of(fi), frames(fi)
        ok = np.zeros(len(cases), bool)
        crops = np.zeros((len(cases), 128, 128, 3), np.uint8)
        for i, (box, pad) in enumerate(cases):
            good, crop = yolo_crop.square_crop(fr[where[i][1]], box, 128, padding=pad)
            ok[i] = bool(good)
            if good:
                crops[i] = crop
        _EXPECTED[fi] = (ok, crops)
    return _EXPECTED[fi]


def call_boxes(fi, slots):
    """float64[BATCH_FRAMES, FIGHTERS, 4] of one call (unused slots repeat the call's first case)."""
    cases = crop_cases(fi)
    first = int(slots[slots >= 0][0])
    return np.array([[cases[int(i) if i >= 0 else first][0] for i in row] for row in slots], np.float64)


def first_mismatch(fi, got_crops, got_status, what, want=None):
    """None when every case's status and bytes equal ``want`` = (status, crops) (default: the oracle's), else a description of the first case
    that differs: its class, both row shifts, its frame of the batch, and the largest byte difference and where it is.
    got_crops uint8[k, 128, 128, 3], got_status int[k], in case order."""
    H, W = FRAMES[fi]
    cases, where = crop_cases(fi), slot_of(fi)
    if want is None:
        ok, crops = expected(fi)
        want_status = np.where(ok, PA_CROP_OK, -1)
    else:
        want_status, crops = want
    for i, (box, pad) in enumerate(cases):
        same = np.array_equal(got_crops[i], crops[i])
        if got_status[i] == want_status[i] and same:
            continue
        g = geometry(box, H, W, pad)
        diff = np.abs(got_crops[i].astype(np.int16) - crops[i].astype(np.int16))
        at = np.unravel_index(int(diff.argmax()), diff.shape)
        return (f"{what}: frame size {H}x{W}, case {i} (padding {pad}, class {classify(box, H, W, pad)}, d {g['d']}, slice "
                f"{g['sh']}x{g['sw']} at y0 {g['y0']} x0 {g['x0']}, clipped {''.join(sorted(g['clip'])) or '-'}), shifts (3W mod 4, 3x0 mod 4) = "
                f"{row_shifts(box, H, W, pad)}, call {where[i][0]} frame {where[i][1]} of {BATCH_FRAMES} fighter {where[i][2]}: status "
                f"{int(got_status[i])} (want {int(want_status[i])}), {int((diff > 0).sum())} bytes differ, largest {int(diff.max())} at "
                f"(row, column, channel) {tuple(int(v) for v in at)}")
    return None


# -- letterbox ----------------------------------------------------------------------------------------------------------
# (frame, network input) -> the un-padded size and the borders (top, left), (bottom, right) ``oracle.yolov5.letterbox`` gives
LETTERBOX = [
    ((480, 640), (384, 640), (384, 512), (0, 64), (0, 64)),
    ((640, 360), (384, 640), (384, 216), (0, 212), (0, 212)),
    ((853, 481), (640, 384), (640, 361), (0, 11), (0, 12)),
    ((719, 1277), (384, 640), (360, 640), (12, 0), (12, 0)),
    ((97, 131), (384, 640), (384, 519), (0, 60), (0, 61)),        # enlarging
    ((384, 640), (384, 640), (384, 640), (0, 0), (0, 0)),         # the copy branch
    ((600, 600), (320, 320), (320, 320), (0, 0), (0, 0)),         # no border, scale 1.875
    ((333, 517), (64, 96), (62, 96), (1, 0), (1, 0)),
]


def letterbox_borders(frame_hw, net_hw):
    """(un-padded (h, w), (top, left), (bottom, right)) measured on ``oracle.yolov5.letterbox``'s own output: a frame whose
    pixels are all 7 comes back 7 / 255 inside and 114 / 255 on the border."""
    from oracle import yolov5 as oy

    out = oy.letterbox(np.full(frame_hw + (3,), 7, np.uint8), net_hw)
    inside = out[0] == np.float32(7) / np.float32(255)
    assert np.array_equal(out[0][~inside], np.full((~inside).sum(), np.float32(114) / np.float32(255)))
    rows, cols = np.flatnonzero(inside.any(axis=1)), np.flatnonzero(inside.any(axis=0))
    assert inside[rows[0]:rows[-1] + 1, cols[0]:cols[-1] + 1].all()
    return ((len(rows), len(cols)), (int(rows[0]), int(cols[0])), (net_hw[0] - int(rows[-1]) - 1, net_hw[1] - int(cols[-1]) - 1))


def scale_geometry(net_hw, img_hw):
    """``scale_boxes``' (gain, pad_x, pad_y) as ``oracle.detect.scale_and_normalise`` computes them."""
    gain = min(net_hw[0] / img_hw[0], net_hw[1] / img_hw[1])
    return gain, (net_hw[1] - img_hw[1] * gain) / 2, (net_hw[0] - img_hw[0] * gain) / 2
