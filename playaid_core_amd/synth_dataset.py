"""The reference's second source of labelled data: synthetic windows (``get_synth``, ``simple_dataset`` and
``load_and_augment_frame_to_stage_crop``, ``playaid/ult_action_dataset.py:97-136, 373-427, 569-689``), composed on the device.

``get_synth`` picks a character and a body, strings animations together until the timeline is at least one window long, cuts S
consecutive frames with their per-frame action labels, and for every frame resizes the RGBA character render to the side of a
square stage crop (``imutils.resize``, INTER_AREA) and pastes it over that crop through its own alpha. Here the renders and the
stage pictures are uploaded ONCE (``SpriteBank``, ``StageBank``: ``pa_synth_bank_create``) and every frame of every window of
a batch is one record of one launch (``csrc/synth_composite.hip``, ``pa_synth_composite``) that writes the
backbone's input layout; no frame exists on the host.

* ``sample_synth`` draws, on the host, what ``get_synth`` draws -- one ``pa_synth_params`` record per frame and the labels;
* ``composite`` checks the records (``pa_synth_params_check``), uploads them and launches;
* ``composite_reference`` is the NUMPY TWIN of the kernel: the same arithmetic, and the contract the kernel is tested against
  bit for bit. It is self-contained: tests pin it, on the CPU, to Pillow's own ``Image.paste`` and to the INTER_AREA
  restatement the crop path is pinned to. Neither cv2 nor imutils is a dependency, so "equals cv2" rests on that restatement
  (DESIGN.md 5.15 lists what is unverified);
* ``SynthWindowDataset`` hands out the reference's 4-tuple per item and whole batches in the model layout from one launch.

``augment_synth_char_crop`` (``dataset_utils.py``), the RGBA chain the reference runs on the sprite BEFORE the paste when
``synth_difficulty`` is 1 or 2, is ``sprite_augment.py``: one launch from the sprite bank into a bank of augmented 128 x 128
sprites, which ``pa_synth_composite`` takes through the same bank handle. ``SynthWindowDataset(sprite_augment=level,
paste_jitter=40)`` is the reference's level; the argument ``synth_difficulty`` itself still raises (it may become sugar for the pair).

The order of the draws in ``sample_synth`` is fixed (scalars, from one ``numpy.random.Generator``; ``choice(seq)`` stands for
``seq[integers(0, len(seq))]``):

 1. the character: ``choice(characters)``
 2. a stand-in action for the body: ``choice([a for a in animations if a != "Unknown"])``, then ``choice(bodies of it)``
 3. per pass of the ``while i < 2 or len(timeline) < S`` loop: ``choice(animations)`` until one is usable -- "Unknown" draws
    ``choice(sorted(the character's actions outside animations))`` at once, an action the character has is taken, any other is
    drawn again -- then ``choice(raw animations)`` and ``choice(cameras)`` of that action and the body
 4. ``last_frame = integers(S, len(timeline) - 1, endpoint=True)``; the window is ``timeline[last_frame - S : last_frame]``
 5. the stage: ``choice(stages)``, then ``x = integers(0, W - D)``, ``y = integers(0, H - D)`` (upper bounds exclusive)
 6. per frame of the window: with ``randomize_stage_background`` step 5 again; else with ``move_stage_background``
    ``integers(-10, 10)`` for x then y (exclusive), added and clamped to ``[0, W - D]`` / ``[0, H - D]``; then with
    ``paste_jitter = k > 0`` ``integers(-k, k, endpoint=True)`` for x then y

The reference draws from Python's global ``random``; the distributions are the same, the streams are not. Where the reference
iterates a ``set`` (the "Unknown" complement) this module sorts it, and ``from_directory`` sorts what ``os.listdir`` and
``glob`` return, so that a draw is a function of the seed alone.
"""
from __future__ import annotations

import ctypes as C
import glob as _glob
import os
from pathlib import Path
from typing import Dict, Optional, Sequence

import numpy as np

from . import _lib

PARAMS_DTYPE = np.dtype([("sprite", "<i4"), ("stage", "<i4"), ("stage_x", "<i4"), ("stage_y", "<i4"), ("paste_dx", "<i4"),
                         ("paste_dy", "<i4"), ("reserved", "<i4", (2,))])
assert PARAMS_DTYPE.itemsize == 32
FORMATS = {"uint8": _lib.PA_SYNTH_U8, "model": _lib.PA_SYNTH_MODEL}
SYNTH_DIFFICULTY_JITTER = 40   # load_and_augment_frame_to_stage_crop:130-132, when synth_difficulty is on


# ---- banks -----------------------------------------------------------------------------------------------------------------------

class _Bank:
    """Images uploaded once into one device allocation (``pa_synth_bank_create``). ``engine=None`` makes a bank of sizes alone:
    ``check_params`` takes it, ``composite`` does not."""
    KIND = None
    CHANNELS = None

    def __init__(self, engine, arrays: Sequence[np.ndarray]):
        arrays = [np.ascontiguousarray(a) for a in arrays]
        for k, a in enumerate(arrays):
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != self.CHANNELS:
                raise ValueError(f"image {k} is uint8[h, w, {self.CHANNELS}], got {a.dtype}{tuple(a.shape)}")
        n = len(arrays)
        self.shapes = [(int(a.shape[0]), int(a.shape[1])) for a in arrays]   # (h, w)
        self.engine = engine
        self._lib = _lib.load()
        ptrs = (C.c_void_p * max(n, 1))(*[a.ctypes.data for a in arrays])
        widths = (C.c_int32 * max(n, 1))(*[s[1] for s in self.shapes])
        heights = (C.c_int32 * max(n, 1))(*[s[0] for s in self.shapes])
        h = C.c_void_p()
        rc = self._lib.pa_synth_bank_create(engine._h if engine is not None else None, self.KIND, ptrs, widths, heights, n, C.byref(h))
        if rc == _lib.PA_ERR_INVALID_ARG:
            msg = self._lib.pa_last_error(engine._h).decode() if engine is not None else self._refusal()
            raise ValueError(msg)
        if rc != _lib.PA_OK:
            engine._check(rc)
        self._h = h

    def _refusal(self) -> str:
        return (f"pa_synth_bank_create refused the images: at least one; sprite sides 1..{_lib.PA_SYNTH_SPRITE_MAX}, none so thin "
                f"that it resizes to an empty image at every dim; stage sides 1..{_lib.PA_SYNTH_STAGE_MAX}")

    def __len__(self):
        return len(self.shapes)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pa_synth_bank_destroy(self._h)
            self._h = None

    def __del__(self):
        self.close()

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()


def frame_number(path: str) -> int:
    """The reference's sort key of a render (``dataset_utils.py:501-504``): the number behind the last underscore."""
    return int(Path(path).stem.split("_")[-1])


class SpriteBank(_Bank):
    """The character renders, RGBA. ``tree[char][action][body][raw_anim][cam]`` lists the bank's image numbers in frame order;
    ``paths[number]`` is the render's file (or a name of the reference's pattern for arrays)."""
    KIND = _lib.PA_SYNTH_SPRITES
    CHANNELS = 4

    def __init__(self, engine, arrays, tree, paths):
        super().__init__(engine, arrays)
        self.tree, self.paths = tree, list(paths)

    @classmethod
    def from_arrays(cls, engine, tree: Dict) -> "SpriteBank":
        """``tree[char][action][body][raw_anim][cam] = [uint8[h, w, 4] RGBA, ...]`` in frame order."""
        arrays, paths, index = [], [], {}
        for char, actions in tree.items():
            index[char] = {}
            for action, bodies in actions.items():
                index[char][action] = {}
                for body, raws in bodies.items():
                    index[char][action][body] = {}
                    for raw, cams in raws.items():
                        index[char][action][body][raw] = {}
                        for cam, frames in cams.items():
                            index[char][action][body][raw][cam] = list(range(len(arrays), len(arrays) + len(frames)))
                            paths += [f"{char}_{body}_{raw}_{cam}_{k}.png" for k in range(len(frames))]
                            arrays += list(frames)
        return cls(engine, arrays, index, paths)

    @classmethod
    def from_directory(cls, engine, root: str) -> "SpriteBank":
        """``root/<char>/<action>/<char>_<body>_<raw anim>_<cam>_<frame>.png``: the layout
        ``get_character_actions_animations_dict`` walks (``dataset_utils.py:429-506``), split at underscores as there (the raw
        animation's name is everything between the body and the camera, ``c05attackairn_frame`` say), frames sorted by number.
        Every PNG is read once, with Pillow, as RGBA (cv2 would read BGRA and swap after the resize: the same bytes)."""
        from PIL import Image

        files: Dict = {}
        for fighter in sorted(os.listdir(root)):
            fighter_dir = os.path.join(root, fighter)
            if not os.path.isdir(fighter_dir):
                continue
            files[fighter] = {}
            for move in sorted(os.listdir(fighter_dir)):
                move_dir = os.path.join(fighter_dir, move)
                if not os.path.isdir(move_dir):
                    continue
                files[fighter][move] = {}
                for f in sorted(_glob.glob(os.path.join(move_dir, "*.png"))):
                    attrs = Path(f).stem.split("_")
                    body, cam, raw = attrs[1], attrs[-2], "_".join(attrs[2:-2])
                    files[fighter][move].setdefault(body, {}).setdefault(raw, {}).setdefault(cam, []).append(f)
        arrays, paths, index = [], [], {}
        for char, actions in files.items():
            index[char] = {}
            for action, bodies in actions.items():
                index[char][action] = {}
                for body, raws in bodies.items():
                    index[char][action][body] = {}
                    for raw, cams in raws.items():
                        index[char][action][body][raw] = {}
                        for cam, fs in cams.items():
                            fs = sorted(fs, key=frame_number)
                            index[char][action][body][raw][cam] = list(range(len(arrays), len(arrays) + len(fs)))
                            paths += fs
                            for f in fs:
                                with Image.open(f) as im:
                                    arrays.append(np.array(im.convert("RGBA")))
        return cls(engine, arrays, index, paths)


class StageBank(_Bank):
    """The stage pictures, RGB."""
    KIND = _lib.PA_SYNTH_STAGES
    CHANNELS = 3

    def __init__(self, engine, arrays, paths=None):
        super().__init__(engine, arrays)
        self.paths = list(paths) if paths is not None else [f"stage_{k}.jpg" for k in range(len(self.shapes))]

    @classmethod
    def from_arrays(cls, engine, arrays: Sequence[np.ndarray]) -> "StageBank":
        return cls(engine, arrays)

    @classmethod
    def from_directory(cls, engine, root: str) -> "StageBank":
        """Every ``**/*.jpg`` under ``root`` (sorted), read once with Pillow as RGB."""
        from PIL import Image

        paths = sorted(_glob.glob(os.path.join(root, "**", "*.jpg"), recursive=True))
        arrays = []
        for f in paths:
            with Image.open(f) as im:
                arrays.append(np.array(im.convert("RGB")))
        return cls(engine, arrays, paths)


# ---- the sampler -----------------------------------------------------------------------------------------------------------------

def _choice(rng: np.random.Generator, seq):
    if len(seq) == 0:
        raise IndexError("Cannot choose from an empty sequence")   # random.choice's
    return seq[int(rng.integers(0, len(seq)))]


def _randrange(rng: np.random.Generator, lo: int, hi: int) -> int:
    if hi <= lo:
        raise ValueError(f"empty range for randrange() ({lo}, {hi}, {hi - lo})")   # random.randrange's
    return int(rng.integers(lo, hi))


def sample_synth(rng: np.random.Generator, bank_tree: Dict, animations: Sequence[str], characters: Sequence[str],
                 num_frames_per_sample: int, dim: int, stage_sizes: Sequence, randomize_stage_background: bool = False,
                 move_stage_background: bool = False, paste_jitter: int = 0):
    """``get_synth`` (``ult_action_dataset.py:570-672``) up to the pixels, in the draw order of this module's docstring.
    ``bank_tree``: ``SpriteBank.tree``; ``stage_sizes``: ``StageBank.shapes`` ((h, w) per stage).
    -> ``(params, char_label, clip_actions, meta)``: S ``pa_synth_params`` records (``PARAMS_DTYPE``), the character's index in
    ``characters``, the S action strings as drawn ("Unknown" stays "Unknown"), and a dict with ``char``, ``body``,
    ``segments`` (per pass ``(drawn action, action used, raw animation, camera, frames)``), ``timeline`` (the bank's image
    numbers, concatenated) and ``last_frame``. Raises the reference's exceptions, with its messages, for a level of the tree
    with nothing under it, and ``ValueError`` for a stage that is not strictly larger than ``dim``."""
    S, D = int(num_frames_per_sample), int(dim)
    animations = list(animations)
    char = _choice(rng, list(characters))
    char_label = list(characters).index(char)
    temp_action = _choice(rng, [a for a in animations if a != "Unknown"])
    if not bank_tree[char][temp_action].keys():
        raise Exception(f"Requested action {temp_action} for {char} has no associated body")
    body = _choice(rng, list(bank_tree[char][temp_action].keys()))
    if not bank_tree[char][temp_action][body].keys():
        raise Exception(f"Requested action {temp_action} for {char} and body {body} has no raw anim")
    if "Unknown" not in animations and not any(a in bank_tree[char] for a in animations):
        raise Exception(f"None of the requested actions is available for {char}")   # (the reference draws for ever)

    timeline, actions, segments = [], [], []
    i = 0
    while i < 2 or len(timeline) < S:
        action = None
        while not action:
            selected = _choice(rng, animations)
            if selected == "Unknown":
                action = _choice(rng, sorted(set(bank_tree[char].keys()) - set(animations)))
            elif selected in bank_tree[char]:
                action = selected
        raw = _choice(rng, list(bank_tree[char][action][body].keys()))
        if not bank_tree[char][action][body][raw].keys():
            raise Exception(f"Requested raw action {raw} for {char} and body {body} has no cam")
        cam = _choice(rng, list(bank_tree[char][action][body][raw].keys()))
        if not bank_tree[char][action][body][raw][cam]:
            raise Exception(f"Requested cam for {char} {body} {raw} {cam} has no anim")
        frames = bank_tree[char][action][body][raw][cam]
        timeline.extend(frames)
        actions.extend([selected] * len(frames))
        segments.append((selected, action, raw, cam, len(frames)))
        i += 1

    last_frame = int(rng.integers(S, len(timeline) - 1, endpoint=True))
    clip = timeline[last_frame - S:last_frame]
    clip_actions = actions[last_frame - S:last_frame]

    def draw_stage():
        s = int(rng.integers(0, len(stage_sizes)))
        h, w = stage_sizes[s]
        return s, _randrange(rng, 0, w - D), _randrange(rng, 0, h - D)

    stage, x, y = draw_stage()
    params = np.zeros(S, dtype=PARAMS_DTYPE)
    for k, sprite in enumerate(clip):
        if randomize_stage_background:
            stage, x, y = draw_stage()
        elif move_stage_background:
            h, w = stage_sizes[stage]
            x_off, y_off = _randrange(rng, -10, 10), _randrange(rng, -10, 10)
            x, y = max(0, min(x + x_off, w - D)), max(0, min(y + y_off, h - D))
        dx = dy = 0
        if paste_jitter:
            dx = int(rng.integers(-paste_jitter, paste_jitter, endpoint=True))
            dy = int(rng.integers(-paste_jitter, paste_jitter, endpoint=True))
        params[k] = (sprite, stage, x, y, dx, dy, (0, 0))
    meta = {"char": char, "body": body, "segments": segments, "timeline": timeline, "last_frame": last_frame}
    return params, char_label, clip_actions, meta


# ---- the records -----------------------------------------------------------------------------------------------------------------

def _as_params(params) -> np.ndarray:
    params = np.ascontiguousarray(params)
    if params.dtype != PARAMS_DTYPE or params.ndim != 1 or len(params) < 1:
        raise ValueError("params is a non-empty 1-d array of synth_dataset.PARAMS_DTYPE (sample_synth)")
    return params


def check_params(params: np.ndarray, sprites: _Bank, stages: _Bank, dim: int) -> bool:
    """``pa_synth_params_check`` (host code of the library; no device call): True when the kernel takes every record without
    clamping anything, every record's stage holds a ``dim`` x ``dim`` crop and no sprite of the bank is too thin for ``dim``."""
    params = _as_params(params)
    rc = _lib.load().pa_synth_params_check(params.ctypes.data_as(C.c_void_p), len(params), sprites._h, stages._h, int(dim))
    return rc == _lib.PA_OK


def clamp_params(params: np.ndarray, sprite_shapes: Sequence, stage_shapes: Sequence, dim: int) -> np.ndarray:
    """The records as the kernel reads them (include/playaid_hip.h): ``sprite`` and ``stage`` clamped into their banks, the
    origin into ``[0, W - dim] x [0, H - dim]`` of the (clamped) stage, the paste offsets to +-4096, the reserved words
    ignored (zero here). A record that passes ``check_params`` comes back unchanged. ``*_shapes``: ``(h, w)`` per image."""
    p = _as_params(params).copy()
    p["sprite"] = np.clip(p["sprite"], 0, len(sprite_shapes) - 1)
    p["stage"] = np.clip(p["stage"], 0, len(stage_shapes) - 1)
    hw = np.asarray([tuple(s[:2]) for s in stage_shapes], dtype=np.int64)[p["stage"]]
    p["stage_x"] = np.clip(p["stage_x"], 0, np.maximum(hw[:, 1] - dim, 0))
    p["stage_y"] = np.clip(p["stage_y"], 0, np.maximum(hw[:, 0] - dim, 0))
    p["paste_dx"] = np.clip(p["paste_dx"], -_lib.PA_SYNTH_PASTE_MAX, _lib.PA_SYNTH_PASTE_MAX)
    p["paste_dy"] = np.clip(p["paste_dy"], -_lib.PA_SYNTH_PASTE_MAX, _lib.PA_SYNTH_PASTE_MAX)
    p["reserved"] = 0
    return p


# ---- the twin --------------------------------------------------------------------------------------------------------------------

def sprite_size(h: int, w: int, dim: int):
    """``(ow, oh)`` of ``imutils.resize`` as ``load_and_augment_frame_to_stage_crop:120-123`` calls it (Python floats)."""
    if h > w:
        return int(w * (dim / float(h))), dim
    return dim, int(h * (dim / float(w)))


def _area_tab(ssize: int, dsize: int, scale: float):
    """``computeResizeAreaTab``: per destination index the list of (source index, float32 weight), in table order."""
    tab = []
    for d in range(dsize):
        fsx1 = d * scale
        fsx2 = fsx1 + scale
        cell = min(scale, ssize - fsx1)
        sx1, sx2 = int(np.ceil(fsx1)), int(np.floor(fsx2))
        sx2 = min(sx2, ssize - 1)
        sx1 = min(sx1, sx2)
        row = []
        if sx1 - fsx1 > 1e-3:
            row.append((sx1 - 1, np.float32((sx1 - fsx1) / cell)))
        row += [(sx, np.float32(1.0 / cell)) for sx in range(sx1, sx2)]
        if fsx2 - sx2 > 1e-3:
            row.append((sx2, np.float32(min(min(fsx2 - sx2, 1.0), cell) / cell)))
        tab.append(row)
    return tab


def _linear_coeffs(ssize: int, dsize: int, zero_at_edge: bool):
    """The 8-bit bilinear resizer's area-mode coefficients along one axis: (s0, s1, w0, w1, plain) per destination index.
    Along x (``zero_at_edge``) a column whose right neighbour would leave the source counts 2048 (``plain``); along y the two
    row indices are clipped and the weights stay."""
    inv = dsize / ssize
    scale = 1.0 / inv
    f32 = np.float32
    out = []
    for d in range(dsize):
        s = int(np.floor(d * scale))
        f = f32((d + 1) - (s + 1) * inv)
        f = f32(0.0) if f <= 0 else f32(f - f32(np.floor(f)))
        plain = zero_at_edge and s + 1 >= ssize
        if zero_at_edge and s >= ssize - 1:
            f, s = f32(0.0), ssize - 1
        w0, w1 = int(np.rint(f32(f32(1.0) - f) * f32(2048.0))), int(np.rint(f * f32(2048.0)))
        out.append((min(s, ssize - 1), min(s + 1, ssize - 1), w0, w1, plain))
    return out


def area_resize(img: np.ndarray, ow: int, oh: int) -> np.ndarray:
    """``cv2.resize(img, (ow, oh), interpolation=cv2.INTER_AREA)`` of uint8[h, w, C], every channel a plain channel, by the
    branch ``cv::resize`` takes -- as ``csrc/synth_math.h`` computes it."""
    h, w, cn = img.shape
    if (w, h) == (ow, oh):
        return img.copy()
    scale_x, scale_y = 1.0 / (ow / w), 1.0 / (oh / h)
    if scale_x < 1.0 or scale_y < 1.0:   # enlarging: the bilinear emulation
        src = img.astype(np.int64)
        xs, ys = _linear_coeffs(w, ow, True), _linear_coeffs(h, oh, False)
        hbuf = np.empty((h, ow, cn), dtype=np.int64)
        for dx, (s0, _, w0, w1, plain) in enumerate(xs):
            hbuf[:, dx] = src[:, s0] * 2048 if plain else src[:, s0] * w0 + src[:, min(s0 + 1, w - 1)] * w1
        out = np.empty((oh, ow, cn), dtype=np.uint8)
        for dy, (r0, r1, b0, b1, _) in enumerate(ys):
            out[dy] = ((((b0 * (hbuf[r0] >> 4)) >> 16) + ((b1 * (hbuf[r1] >> 4)) >> 16) + 2) >> 2) & 0xFF
        return out
    isx, isy = int(np.rint(scale_x)), int(np.rint(scale_y))
    eps = float(np.finfo(np.float64).eps)
    if abs(scale_x - isx) < eps and abs(scale_y - isy) < eps:
        s = img[:oh * isy, :ow * isx].reshape(oh, isy, ow, isx, cn).astype(np.int64).sum(axis=(1, 3))
        if isx == 2 and isy == 2:
            return ((s + 2) >> 2).astype(np.uint8)
        return np.clip(np.rint(s.astype(np.float32) * (np.float32(1.0) / np.float32(isx * isy))), 0, 255).astype(np.uint8)
    src = img.astype(np.float32)
    buf = np.zeros((h, ow, cn), dtype=np.float32)
    for dx, row in enumerate(_area_tab(w, ow, scale_x)):      # horizontal, table order, multiply then add
        for si, a in row:
            buf[:, dx] = buf[:, dx] + src[:, si] * a
    acc = np.zeros((oh, ow, cn), dtype=np.float32)
    for dy, row in enumerate(_area_tab(h, oh, scale_y)):      # vertical
        for si, b in row:
            acc[dy] = acc[dy] + b * buf[si]
    return np.clip(np.rint(acc), 0, 255).astype(np.uint8)


def paste_rgba(canvas: np.ndarray, sprite: np.ndarray, px: int, py: int) -> None:
    """``Image.paste(sprite, (px, py), sprite)`` onto uint8[D, D, 3] in place: Pillow's ``paste_mask_RGBA``, clipped."""
    H, W = canvas.shape[:2]
    sh, sw = sprite.shape[:2]
    x0, y0, x1, y1 = max(px, 0), max(py, 0), min(px + sw, W), min(py + sh, H)
    if x1 <= x0 or y1 <= y0:
        return
    s = sprite[y0 - py:y1 - py, x0 - px:x1 - px].astype(np.int32)
    d = canvas[y0:y1, x0:x1].astype(np.int32)
    a = s[..., 3:4]
    t = s[..., :3] * a + d * (255 - a) + 128
    canvas[y0:y1, x0:x1] = (((t >> 8) + t) >> 8).astype(np.uint8)


def composite_reference(sprite_arrays: Sequence[np.ndarray], stage_arrays: Sequence[np.ndarray], params: np.ndarray, dim: int = 128,
                        out_format: str = "uint8") -> np.ndarray:
    """The numpy twin of ``pa_synth_composite``: RGBA sprites, RGB stages and n records -> uint8[n, dim, dim, 3] (``"uint8"``)
    or float32[n, 3, 128, 128] with value ``float32(byte) / float32(255)`` (``"model"``, ``dim`` 128 only). The records are
    read as the kernel reads them (``clamp_params``)."""
    if out_format not in FORMATS:
        raise ValueError(f"out_format must be one of {sorted(FORMATS)}")
    D = int(dim)
    if not _lib.PA_SYNTH_DIM_MIN <= D <= _lib.PA_SYNTH_DIM_MAX or (out_format == "model" and D != 128):
        raise ValueError(f"dim is {_lib.PA_SYNTH_DIM_MIN}..{_lib.PA_SYNTH_DIM_MAX}, and 128 for the model layout")
    if any(s.shape[0] < D or s.shape[1] < D for s in stage_arrays):
        raise ValueError("a stage is smaller than dim")
    p = clamp_params(params, [s.shape for s in sprite_arrays], [s.shape for s in stage_arrays], D)
    out = np.empty((len(p), D, D, 3), dtype=np.uint8)
    resized = {}
    for i, r in enumerate(p):
        k = int(r["sprite"])
        if k not in resized:
            h, w = sprite_arrays[k].shape[:2]
            ow, oh = sprite_size(h, w, D)
            if ow < 1 or oh < 1:
                raise ValueError(f"sprite {k} ({h} x {w}) resizes to an empty image at dim {D} (cv2.resize raises)")
            resized[k] = area_resize(np.asarray(sprite_arrays[k]), min(ow, D), min(oh, D))
        s = resized[k]
        x, y = int(r["stage_x"]), int(r["stage_y"])
        out[i] = stage_arrays[int(r["stage"])][y:y + D, x:x + D]
        paste_rgba(out[i], s, int((D - s.shape[1]) / 2) + int(r["paste_dx"]), int((D - s.shape[0]) / 2) + int(r["paste_dy"]))
    if out_format == "uint8":
        return out
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)


# ---- the device ------------------------------------------------------------------------------------------------------------------

def composite(engine, sprites: SpriteBank, stages: StageBank, params: np.ndarray, dim: int = 128, out_format: str = "uint8", out=None,
              check: bool = True):
    """One ``pa_synth_composite`` launch on ``engine``: n records -> a device tensor uint8[n, dim, dim, 3] (``"uint8"``) or
    float32[n, 3, 128, 128] (``"model"``: the input of ``pa_backbone_windows`` / ``CNNActionDetector.forward``). The records go
    through ``pa_synth_params_check`` first (ValueError); ``check=False`` skips that -- the kernel is defined for any bytes
    and reads them as ``clamp_params`` does. ``out``: a contiguous device tensor of that shape and dtype (a slice of a larger
    one will do; the library refuses one that is not 16-byte aligned). Enqueue only: nothing is read back."""
    import torch

    if out_format not in FORMATS:
        raise ValueError(f"out_format must be one of {sorted(FORMATS)}")
    params = _as_params(params)
    n, D = len(params), int(dim)
    if check and not check_params(params, sprites, stages, D):
        raise ValueError("composite: pa_synth_params_check refused the records (a sprite or stage outside its bank, a stage smaller "
                         "than dim, an origin outside the stage, a paste offset beyond 4096, or a reserved word that is not 0)")
    pd = torch.from_numpy(params.view(np.uint8).reshape(n, PARAMS_DTYPE.itemsize)).to(engine.device)
    shape, dtype = ((n, D, D, 3), torch.uint8) if out_format == "uint8" else ((n, 3, D, D), torch.float32)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=engine.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"out is a contiguous {dtype} device tensor {shape}")
    engine._check(engine._lib.pa_synth_composite(engine._h, sprites._h, stages._h, C.c_void_p(pd.data_ptr()), n, D, FORMATS[out_format],
                                                 C.c_void_p(out.data_ptr()), engine._stream()))
    return out


# ---- the dataset -----------------------------------------------------------------------------------------------------------------

class SynthWindowDataset:
    """``UltActionRecogDataset`` on its synthetic split: item ``idx`` is one ``get_synth`` window, drawn as a pure function of
    ``(seed, epoch, idx)`` and composed on the device."""

    def __init__(self, engine, sprites: SpriteBank, stages: StageBank, animations: Optional[Sequence[str]] = None,
                 characters: Optional[Sequence[str]] = None, num_samples: int = 1024, num_frames_per_sample: int = 7,
                 img_dimension: int = 128, randomize_stage_background: bool = False, move_stage_background: bool = False,
                 paste_jitter: int = 0, seed: int = 0, synth_difficulty: int = 0, sprite_augment=None):
        """``animations``: the action list the labels index (default: the ontology's, as ``ClipWindowDataset``);
        ``characters``: the list the character label indexes (default: the bank's characters). ``paste_jitter``: the reference
        uses 40 when ``synth_difficulty`` is on. ``sprite_augment``: None, or 1 / 2 / a dict of ``augment_synth_char_crop``'s
        probabilities (``sprite_augment.sample_sprite_params``): every frame's render goes through that function, with its own
        draw from the item's generator AFTER the draws of ``sample_synth`` (so None gives the same windows as before), in one
        ``pa_sprite_augment`` launch per item or batch ahead of the one composite launch. ``synth_difficulty`` other than 0
        raises: see the module docstring."""
        if synth_difficulty:
            raise NotImplementedError("synth_difficulty 1 / 2 is augment_synth_char_crop (dataset_utils.py) on the sprite BEFORE the "
                                      "paste plus paste offsets of +-40: pass sprite_augment=level, paste_jitter=40, which together "
                                      "are the reference's level.")
        self.sprite_augment = self._check_sprite_augment(sprite_augment)
        self._aug_bank = None
        if animations is None:
            from .anim_ontology import MOVE_TO_CLASS_ID

            animations = list(MOVE_TO_CLASS_ID.keys())
        self.engine, self.sprites, self.stages = engine, sprites, stages
        self.animations = list(animations)
        self.characters = list(characters) if characters is not None else list(sprites.tree.keys())
        self.num_samples = int(num_samples)
        self.num_frames_per_sample = int(num_frames_per_sample)
        self.img_dimension = int(img_dimension)
        self.randomize_stage_background = bool(randomize_stage_background)
        self.move_stage_background = bool(move_stage_background)
        self.paste_jitter = int(paste_jitter)
        self.seed, self.epoch = int(seed), 0
        self._owner = None   # image number -> (char, action), built for simple_item

    def __len__(self):
        return self.num_samples

    def set_epoch(self, epoch: int):
        """The epoch the draws are keyed by (with ``seed`` and the item's index)."""
        self.epoch = int(epoch)

    @staticmethod
    def _check_sprite_augment(level):
        from . import sprite_augment as sa

        if level is None or isinstance(level, dict) or (not isinstance(level, bool) and level in sa.SPRITE_LEVELS):
            if isinstance(level, dict):
                sa.sample_sprite_params(1, level, np.random.default_rng(0))   # (ValueError for an unknown key)
            return level
        raise ValueError(f"sprite_augment is None, one of {sorted(sa.SPRITE_LEVELS)} or a dict, got {level!r}")

    def make_synth_more_challenging(self):
        """``UltActionRecogDataset.make_synth_more_challenging`` (``ult_action_dataset.py:561-564``) for the sprite augmentation: an
        integer level (None counts as 0) goes one up, 2 at most; a dict stays as it is."""
        from . import sprite_augment as sa

        if not isinstance(self.sprite_augment, dict):
            self.sprite_augment = min((self.sprite_augment or 0) + 1, sa.MAX_LEVEL)

    def _draw(self, idx: int):
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        rng = np.random.default_rng([self.seed, self.epoch, int(idx)])
        draw = sample_synth(rng, self.sprites.tree, self.animations, self.characters, self.num_frames_per_sample, self.img_dimension,
                            self.stages.shapes, self.randomize_stage_background, self.move_stage_background, self.paste_jitter)
        aug = None
        if self.sprite_augment is not None:
            from . import sprite_augment as sa

            aug = sa.sample_sprite_params(len(draw[0]), self.sprite_augment, rng, src=draw[0]["sprite"])
        return draw, aug

    def sample(self, idx: int):
        """``sample_synth`` for item ``idx``: the draw alone, nothing on the device."""
        return self._draw(idx)[0]

    def sample_sprite_augment(self, idx: int):
        """The ``pa_sprite_aug_params`` records of item ``idx``'s S frames (None without ``sprite_augment``): drawn from the item's
        generator after ``sample``'s draws; record k reads the render ``sample(idx)[0]["sprite"][k]``."""
        return self._draw(idx)[1]

    def _composite(self, params, aug, out_format):
        """The frames of ``params``; with ``aug`` (one record per frame) every render is augmented into a bank of ``len(params)``
        slots first and frame k pastes slot k."""
        if aug is None:
            return composite(self.engine, self.sprites, self.stages, params, self.img_dimension, out_format)
        from . import sprite_augment as sa

        if self._aug_bank is None or len(self._aug_bank) < len(params):   # kept: the launches on it are ordered by the engine's stream
            self._aug_bank = sa.AugmentedSpriteBank(self.engine, len(params))
        bank = sa.augment_sprites(self.engine, self.sprites, aug, out=self._aug_bank)
        params = params.copy()
        params["sprite"] = np.arange(len(params))
        return composite(self.engine, bank, self.stages, params, self.img_dimension, out_format)

    def _item(self, params, char_label, actions, frame_paths, aug=None):
        import torch

        frames = self._composite(params, aug, "uint8").cpu()
        return (frames.permute(0, 3, 1, 2).float() / 255.0, torch.tensor(char_label),
                torch.tensor([self.animations.index(a) for a in actions]),
                {"char": self.characters[char_label], "frames": list(frames.numpy()), "frame_paths": frame_paths, "actions": actions})

    def __getitem__(self, idx: int):
        """The reference's 4-tuple (``ult_action_dataset.py:676-689``): ``frames[S, 3, D, D].float() / 255``,
        ``tensor(char_label)``, ``tensor(anim_label[S])`` and a dict with ``char``, ``frames``, ``frame_paths``, ``actions``."""
        (params, char_label, actions, _), aug = self._draw(idx)
        return self._item(params, char_label, actions, [self.sprites.paths[int(k)] for k in params["sprite"]], aug)

    def simple_item(self, idx: int, frames: Sequence):
        """``simple_dataset``'s fixed-frame form (``ult_action_dataset.py:373-427``): the bank's images ``frames`` over stage 0
        at origin (0, 0), pasted centred; every frame is labelled with the action of the FIRST one, as there (the stray middle
        frame is to be predicted as its surroundings), and ``frame_paths`` are ``"<k>.png"``. ``frames`` may also be the
        reference's pair ``[batch_1, batch_2]`` of such lists: an odd ``idx`` takes ``batch_1``, an even one ``batch_2``
        (``selected_batch = batch_1 if idx % 2 else batch_2``). An action outside ``animations`` raises ``ValueError``, as
        the reference's ``animations.index(action)`` does."""
        frames = list(frames)
        if frames and not np.isscalar(frames[0]):
            if len(frames) != 2:
                raise ValueError("frames is a list of image numbers or the pair [batch_1, batch_2] of such lists")
            frames = list(frames[0] if idx % 2 else frames[1])
        if self._owner is None:
            self._owner = {}
            for char, acts in self.sprites.tree.items():
                for action, bodies in acts.items():
                    for raws in bodies.values():
                        for cams in raws.values():
                            for numbers in cams.values():
                                self._owner.update({k: (char, action) for k in numbers})
        char, action = self._owner[int(frames[0])]
        params = np.zeros(len(frames), dtype=PARAMS_DTYPE)
        params["sprite"] = frames
        self.animations.index(action)   # (ValueError for an action outside the list)
        actions = [action] * len(frames)
        return self._item(params, self.characters.index(char), actions, [f"{k}.png" for k in range(len(frames))])

    def batches(self, batch_size: int):
        """``(x[B, S, 3, 128, 128], char_ids[B], action_ids[B, S], metas)`` in index order, all ``B * S`` frames of a batch from
        ONE launch into the model layout; device tensors, as ``training_step`` of the three models takes them. ``metas`` holds
        ``char``, ``frame_paths`` and ``actions`` (no ``frames``: none exists on the host)."""
        import torch

        S = self.num_frames_per_sample
        for i0 in range(0, len(self), batch_size):
            both = [self._draw(i) for i in range(i0, min(i0 + batch_size, len(self)))]
            draws = [b[0] for b in both]
            params = np.concatenate([d[0] for d in draws])
            aug = np.concatenate([b[1] for b in both]) if self.sprite_augment is not None else None
            x = self._composite(params, aug, "model")
            dev = self.engine.device
            yield (x.view(len(draws), S, 3, self.img_dimension, self.img_dimension),
                   torch.tensor([d[1] for d in draws], device=dev),
                   torch.tensor([[self.animations.index(a) for a in d[2]] for d in draws], device=dev),
                   [{"char": self.characters[d[1]], "frame_paths": [self.sprites.paths[int(k)] for k in d[0]["sprite"]], "actions": d[2]}
                    for d in draws])
