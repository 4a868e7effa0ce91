"""The reference's training set for its DETECTOR: ``generate_stage_char_compositions`` / ``composite_chars_onto_stage``
(``playaid/data_gen_scripts/gen_synth_char_detection.py:190-308``), composed and encoded on the device.

Per image the reference draws one to four character renders, ``Image.resize``s each to a random width of 50..150, runs
``augment_synth_char_crop`` on it, pastes it at a Gaussian position over a whole stage picture and writes ``images/comp-i.jpg``
with ``labels/comp-i.txt`` in YOLO format. Here the renders and the stage pictures are in a ``SpriteBank`` / ``StageBank`` on
the device and a batch of images is four steps on it, no frame on the host:

* ``resize_sprites`` -- Pillow's RGBA ``Image.resize`` of n renders, each to its own size, into a ``ResizedSpriteBank``
  (``csrc/sprite_resize.hip``, ``pa_sprite_resize``);
* ``sprite_augment.augment_sprites`` on that bank (``pa_sprite_augment``);
* ``compose_scenes`` -- up to four augmented sprites pasted over a whole stage picture of any size
  (``csrc/scene_composite.hip``, ``pa_scene_composite``);
* ``JpegEncoder.encode_images(bgr=False, quality=95, subsampling=2)`` on the scenes as they lie: what the reference's
  ``cv.cvtColor(RGB2BGR)`` + ``cv.imwrite`` write.

``resize_sprites_reference`` and ``compose_scenes_reference`` are the NUMPY TWINS of the two kernels: the same arithmetic, and
the contract the kernels are tested against bit for bit. They are self-contained; tests pin them, on the CPU, to the installed
Pillow's own ``Image.resize`` and ``Image.paste``. ``sample_scenes`` draws, on the host, what the reference draws, and
``generate_stage_char_compositions`` is the reference's entry point.

The order of the draws in ``sample_scenes`` is fixed (scalars, from one ``numpy.random.Generator``; ``choice(seq)`` stands for
``seq[integers(0, len(seq))]``). Per image:

 1. the number of characters: ``integers(1, 4, endpoint=True)``
 2. per character: ``choice(the names of CHAR_LIST the bank has)``, ``choice(sorted(its actions))``, ``choice(the renders of that
    character and action, in bank order)``
 3. the stage: ``choice(stages)``
 4. per character, in order, if its render is at least 100 wide and 100 high (the reference's ``continue`` skips any other, so an
    image can have fewer characters than drawn, or none and an empty label file): ``basewidth = integers(50, 150,
    endpoint=True)``, ``hsize = int(h * (basewidth / float(w)))``; one ``sprite_augment.sample_sprite_params`` record (its
    twelve draws, with ``augment_synth_char_crop``'s own defaults); ``cx = int(normal(W / 2, W / 6))``, ``cy = int(normal(H / 2,
    H / 6))``. A ``cx`` outside ``[0, W]`` becomes the FLOAT ``W / 2``, as in the reference, and ``cy`` likewise: the sprite's
    corner is ``int(cx - 64.0)`` (Python's truncation) and the label carries the float.

A label row is ``(class_id, cx / W, cy / H, 128 / W, 128 / H)``: the reference labels the augmented 128 x 128 sprite, not the
character inside it. ``class_id`` is ``len(MOVE_TO_CLASS_ID) * char + action`` (``class_type="CHAR+ACTION"``, the reference's
setting) or the character's index in ``CHAR_LIST`` (``"CHAR"``).

Two readings of the reference: its line ``random.choice(char_animations[character][action])`` raises ``KeyError`` against the
nested dictionary ``get_character_actions_animations_dict`` returns today (a dict of bodies, not a list of paths); "a uniform
render of that character and action" is this project's reading of it. And the reference draws from Python's global ``random``;
the distributions are the same, the streams are not. Where it iterates ``dict.keys()`` this module sorts.
"""
from __future__ import annotations

import ctypes as C
import glob as _glob
import os
from typing import List, Optional, Sequence

import numpy as np

from . import _lib, constants
from . import sprite_augment as sa
from .anim_ontology import MOVE_TO_CLASS_ID
from .synth_dataset import SpriteBank, StageBank, _Bank, _choice, paste_rgba

SIZE = 128                                   # the augmented sprite's side
W_MAX, H_MAX = _lib.PA_SPRITE_RESIZE_W_MAX, _lib.PA_SPRITE_RESIZE_H_MAX
SPRITES_MAX = _lib.PA_SCENE_SPRITES_MAX
PASTE_MAX = _lib.PA_SYNTH_PASTE_MAX
BASEWIDTH_MIN, BASEWIDTH_MAX = 50, 150       # gen_synth_char_detection.py:216
RENDER_SIDE_MIN = 100                        # :207
MAX_NUM_CHAR = 4                             # :25
JPEG_QUALITY = 95                            # cv.imwrite's default

RESIZE_DTYPE = np.dtype([("src", "<i4"), ("out_w", "<i4"), ("out_h", "<i4"), ("reserved", "<i4")])
SCENE_DTYPE = np.dtype([("stage", "<i4"), ("n_sprites", "<i4"), ("sprites", [("slot", "<i4"), ("x", "<i4"), ("y", "<i4")], (SPRITES_MAX,)),
                        ("reserved", "<i4", (2,))])
assert RESIZE_DTYPE.itemsize == C.sizeof(_lib.pa_sprite_resize_params) == 16
assert SCENE_DTYPE.itemsize == C.sizeof(_lib.pa_scene_params) == 64


def _as(params, dtype, what: str) -> np.ndarray:
    params = np.ascontiguousarray(params)
    if params.dtype != dtype or params.ndim != 1 or len(params) < 1:
        raise ValueError(f"params is a non-empty 1-d array of detect_composite.{what}")
    return params


# ---- Pillow's RGBA resize ----------------------------------------------------------------------------------------------------------

class ResizedSpriteBank(_Bank):
    """A sprite bank of ``n`` slots of up to ``max_w`` x ``max_h`` RGBA pixels that ``pa_sprite_resize`` writes, descriptors
    included (``pa_sprite_resize_bank_create``), with the kernel's scratch. ``sprite_augment.augment_sprites`` and
    ``synth_dataset.composite`` take it as ``sprites``. ``shapes[i]`` is slot i's current ``(h, w)`` (1 x 1 until it is filled).
    ``engine=None`` makes a bank of sizes alone."""
    KIND = _lib.PA_SYNTH_SPRITES
    CHANNELS = 4

    def __init__(self, engine, n: int, max_w: int = W_MAX, max_h: int = H_MAX):
        n, self.max_w, self.max_h = int(n), int(max_w), int(max_h)
        self.engine = engine
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.pa_sprite_resize_bank_create(engine._h if engine is not None else None, n, self.max_w, self.max_h, C.byref(h))
        if rc == _lib.PA_ERR_INVALID_ARG:
            raise ValueError(f"pa_sprite_resize_bank_create: n is 1..65535, max_w 1..{W_MAX}, max_h 1..{H_MAX}")
        if rc != _lib.PA_OK:
            if engine is None:
                raise MemoryError("pa_sprite_resize_bank_create")
            engine._check(rc)
        self._h = h
        self.shapes = [(1, 1)] * n

    def read(self, slot: int) -> np.ndarray:
        """Slot ``slot`` as uint8[h, w, 4] on the host (``pa_sprite_resize_bank_read``: waits for the engine's stream)."""
        h, w = self.shapes[slot]
        out = np.empty((h, w, 4), dtype=np.uint8)
        rc = self._lib.pa_sprite_resize_bank_read(self.engine._h if self.engine is not None else None, self._h, int(slot),
                                                  out.ctypes.data_as(C.c_void_p), out.nbytes, self.engine._stream() if self.engine is not None else None)
        if rc == _lib.PA_ERR_INVALID_ARG:
            raise ValueError("pa_sprite_resize_bank_read: a bank made with an engine, and one of its slots")
        self.engine._check(rc)
        return out


def resize_params(src, out_w, out_h) -> np.ndarray:
    """Records from three equally long sequences."""
    p = np.zeros(len(src), dtype=RESIZE_DTYPE)
    p["src"], p["out_w"], p["out_h"] = src, out_w, out_h
    return p


def resize_check_status(params: np.ndarray, sprites: _Bank, out: ResizedSpriteBank) -> int:
    """``pa_sprite_resize_params_check``'s status (host code of the library; no device call): ``PA_OK``, ``PA_ERR_INVALID_ARG``
    for a source outside the bank, a size below 1 or a non-zero reserved word, ``PA_ERR_CAPACITY`` for more records than ``out``
    has slots or a size beyond them."""
    params = _as(params, RESIZE_DTYPE, "RESIZE_DTYPE")
    return int(_lib.load().pa_sprite_resize_params_check(params.ctypes.data_as(C.c_void_p), len(params), sprites._h, out._h))


def resize_clamp_params(params: np.ndarray, n_src: int, max_w: int = W_MAX, max_h: int = H_MAX) -> np.ndarray:
    """The records as the kernel reads them (include/playaid_hip.h): ``src`` clamped to ``[0, n_src)``, ``out_w`` to
    ``1..max_w``, ``out_h`` to ``1..max_h`` (the output bank's slot), the reserved word ignored (zero here)."""
    p = _as(params, RESIZE_DTYPE, "RESIZE_DTYPE").copy()
    p["src"] = np.clip(p["src"], 0, n_src - 1)
    p["out_w"] = np.clip(p["out_w"], 1, max_w)
    p["out_h"] = np.clip(p["out_h"], 1, max_h)
    p["reserved"] = 0
    return p


def pil_resize_rgba(img: np.ndarray, ow: int, oh: int) -> np.ndarray:
    """``Image.fromarray(img).resize((ow, oh))`` of uint8[h, w, 4] RGBA as Pillow does it (default filter BICUBIC): equal sizes
    copy; otherwise to premultiplied RGBa (``MULDIV255``), the horizontal 8-bit pass when the width changes, then the vertical
    one when the height changes (22-bit coefficients of ``precompute_coeffs``; a pass whose size stays is skipped), back to RGBA
    (alpha 0 or 255: unchanged, else ``min(255, 255 * c // a)``)."""
    h, w = img.shape[:2]
    if (w, h) == (ow, oh):
        return img.copy()
    a = img[..., 3:4].astype(np.int64)
    t = img[..., :3].astype(np.int64) * a + 128
    cur = np.concatenate([((t >> 8) + t) >> 8, a], axis=-1).astype(np.uint8)
    if ow != w:
        cur = sa._bicubic_axis0(cur.transpose(1, 0, 2), ow).transpose(1, 0, 2)
    if oh != h:
        cur = sa._bicubic_axis0(cur, oh)
    cur = cur.astype(np.int64)
    al = cur[..., 3:4]
    rgb = np.where((al == 0) | (al == 255), cur[..., :3], np.minimum(255 * cur[..., :3] // np.maximum(al, 1), 255))
    return np.concatenate([rgb, al], axis=-1).astype(np.uint8)


def resize_sprites_reference(sprite_arrays: Sequence[np.ndarray], params: np.ndarray, max_w: int = W_MAX, max_h: int = H_MAX) -> List[np.ndarray]:
    """The numpy twin of ``pa_sprite_resize``: RGBA renders and n records -> n arrays uint8[out_h, out_w, 4]. The records are
    read as the kernel reads them (``resize_clamp_params`` with the output bank's slot size)."""
    p = resize_clamp_params(params, len(sprite_arrays), max_w, max_h)
    done = {}
    out = []
    for r in p:
        key = (int(r["src"]), int(r["out_w"]), int(r["out_h"]))
        if key not in done:
            done[key] = pil_resize_rgba(np.asarray(sprite_arrays[key[0]]), key[1], key[2])
        out.append(done[key])
    return out


def resize_sprites(engine, sprites: _Bank, params: np.ndarray, out: Optional[ResizedSpriteBank] = None, check: bool = True) -> ResizedSpriteBank:
    """One ``pa_sprite_resize`` launch on ``engine``: slot i of ``out`` (default: a new ``ResizedSpriteBank`` of ``len(params)``
    slots of the largest size) becomes ``Image.resize((out_w, out_h))`` of render ``params[i].src`` of ``sprites``; ``out`` is
    returned, its ``shapes`` updated. The records go through ``pa_sprite_resize_params_check`` first (ValueError);
    ``check=False`` skips that -- the kernel is defined for any bytes and reads them as ``resize_clamp_params`` does. Enqueue
    only: nothing is read back."""
    params = _as(params, RESIZE_DTYPE, "RESIZE_DTYPE")
    n = len(params)
    if out is None:
        out = ResizedSpriteBank(engine, n)
    elif not isinstance(out, ResizedSpriteBank) or len(out) < n:
        raise ValueError(f"out is a ResizedSpriteBank of at least {n} slots")
    if check:
        rc = resize_check_status(params, sprites, out)
        if rc == _lib.PA_ERR_CAPACITY:
            raise ValueError(f"resize_sprites: a size beyond the output bank's slots ({out.max_w} x {out.max_h})")
        if rc != _lib.PA_OK:
            raise ValueError("resize_sprites: pa_sprite_resize_params_check refused the records (a source outside the bank, a size "
                             "below 1, or a reserved word that is not 0)")
    rc = engine._lib.pa_sprite_resize(engine._h, sprites._h, params.ctypes.data_as(C.c_void_p), n, out._h, engine._stream())
    if rc in (_lib.PA_ERR_INVALID_ARG, _lib.PA_ERR_CAPACITY):
        raise ValueError(engine._lib.pa_last_error(engine._h).decode())
    engine._check(rc)
    p = resize_clamp_params(params, len(sprites), out.max_w, out.max_h)
    out.shapes[:n] = [(int(h), int(w)) for h, w in zip(p["out_h"], p["out_w"])]
    return out


# ---- the scenes --------------------------------------------------------------------------------------------------------------------

def scene_check_params(params: np.ndarray, sprites: _Bank, stages: _Bank) -> bool:
    """``pa_scene_params_check`` (host code of the library; no device call): True when the kernel takes every record without
    clamping anything -- stage and slots inside their banks, ``n_sprites`` 0..4, offsets within +-4096, the unused entries and
    the reserved words zero. ``sprites``: a bank of 128 x 128 slots (``sprite_augment.AugmentedSpriteBank``)."""
    params = _as(params, SCENE_DTYPE, "SCENE_DTYPE")
    return _lib.load().pa_scene_params_check(params.ctypes.data_as(C.c_void_p), len(params), sprites._h, stages._h) == _lib.PA_OK


def scene_clamp_params(params: np.ndarray, n_slots: int, n_stages: int) -> np.ndarray:
    """The records as the kernel reads them: ``stage`` and ``slot`` clamped into their banks, ``n_sprites`` to 0..4, ``x`` and
    ``y`` to +-4096; the entries from ``n_sprites`` on and the reserved words are not read (zero here)."""
    p = _as(params, SCENE_DTYPE, "SCENE_DTYPE").copy()
    p["stage"] = np.clip(p["stage"], 0, n_stages - 1)
    p["n_sprites"] = np.clip(p["n_sprites"], 0, SPRITES_MAX)
    p["sprites"]["slot"] = np.clip(p["sprites"]["slot"], 0, n_slots - 1)
    p["sprites"]["x"] = np.clip(p["sprites"]["x"], -PASTE_MAX, PASTE_MAX)
    p["sprites"]["y"] = np.clip(p["sprites"]["y"], -PASTE_MAX, PASTE_MAX)
    unused = np.arange(SPRITES_MAX)[None, :] >= p["n_sprites"][:, None]
    for f in ("slot", "x", "y"):
        p["sprites"][f][unused] = 0
    p["reserved"] = 0
    return p


def scene_layout(params: np.ndarray, stage_shapes: Sequence):
    """Where ``pa_scene_composite`` puts the scenes: ``(offsets int64[n], total bytes)``; a scene takes its ``H * W * 3`` bytes
    rounded up to 16."""
    p = scene_clamp_params(params, 1, len(stage_shapes))
    hw = np.asarray([tuple(s[:2]) for s in stage_shapes], dtype=np.int64)[p["stage"]]
    sizes = (hw[:, 0] * hw[:, 1] * 3 + 15) & ~np.int64(15)
    ends = np.cumsum(sizes)
    return ends - sizes, int(ends[-1])


def compose_scenes_reference(slot_arrays, stage_arrays: Sequence[np.ndarray], params: np.ndarray) -> List[np.ndarray]:
    """The numpy twin of ``pa_scene_composite``: 128 x 128 RGBA sprites (uint8[slots, 128, 128, 4]), RGB stages and n records
    -> n arrays uint8[H, W, 3]: the stage with the record's sprites pasted over it in order, each through its own alpha
    (``synth_dataset.paste_rgba``: Pillow's ``paste_mask_RGBA``, clipped). The records are read as the kernel reads them
    (``scene_clamp_params``)."""
    p = scene_clamp_params(params, len(slot_arrays), len(stage_arrays))
    out = []
    for r in p:
        canvas = np.array(stage_arrays[int(r["stage"])], dtype=np.uint8)
        for k in range(int(r["n_sprites"])):
            s = r["sprites"][k]
            paste_rgba(canvas, np.asarray(slot_arrays[int(s["slot"])]), int(s["x"]), int(s["y"]))
        out.append(canvas)
    return out


def compose_scenes(engine, sprites: _Bank, stages: StageBank, params: np.ndarray, images=None, check: bool = True):
    """One ``pa_scene_composite`` call on ``engine``: n records -> ``(images, desc)``, the scenes as packed uint8[H][W][3] RGB in
    one uint8 device tensor (``scene_layout`` says where; ``images``: a contiguous uint8 device tensor of at least that many
    bytes to write into) and the int64[n, 2] device tensor ``JpegEncoder.encode_images`` takes (``pa_crop_image``). The records
    go through ``pa_scene_params_check`` first (ValueError); ``check=False`` skips that -- the kernel is defined for any bytes
    and reads them as ``scene_clamp_params`` does. Enqueue only: nothing is read back."""
    import torch

    params = _as(params, SCENE_DTYPE, "SCENE_DTYPE")
    n = len(params)
    if check and not scene_check_params(params, sprites, stages):
        raise ValueError("compose_scenes: pa_scene_params_check refused the records (a stage or slot outside its bank, more than 4 "
                         "sprites, an offset beyond 4096, or an unused entry or reserved word that is not 0)")
    _, total = scene_layout(params, stages.shapes)
    if images is None:
        images = torch.empty(total, dtype=torch.uint8, device=engine.device)
    elif images.dtype != torch.uint8 or not images.is_cuda or not images.is_contiguous() or images.numel() < total:
        raise ValueError(f"images is a contiguous uint8 device tensor of at least {total} bytes")
    pd = torch.from_numpy(params.view(np.uint8).reshape(n, SCENE_DTYPE.itemsize)).to(engine.device)
    desc = torch.empty((n, 2), dtype=torch.int64, device=engine.device)
    rc = engine._lib.pa_scene_composite(engine._h, sprites._h, stages._h, C.c_void_p(pd.data_ptr()), n, C.c_void_p(images.data_ptr()),
                                        images.numel(), C.c_void_p(desc.data_ptr()), engine._stream())
    if rc == _lib.PA_ERR_INVALID_ARG:
        raise ValueError(engine._lib.pa_last_error(engine._h).decode())
    engine._check(rc)
    return images, desc


def unpack_scenes(images, params: np.ndarray, stage_shapes: Sequence) -> List[np.ndarray]:
    """``compose_scenes``' buffer on the host as n arrays uint8[H, W, 3] (one copy; for tests and for looking at scenes)."""
    p = scene_clamp_params(params, 1, len(stage_shapes))
    offsets, total = scene_layout(params, stage_shapes)
    buf = images[:total].cpu().numpy()
    out = []
    for off, r in zip(offsets.tolist(), p):
        h, w = stage_shapes[int(r["stage"])][:2]
        out.append(buf[off:off + h * w * 3].reshape(h, w, 3).copy())
    return out


# ---- the sampler -------------------------------------------------------------------------------------------------------------------

def _renders(tree, char: str, action: str) -> List[int]:
    """The bank's image numbers of one character and action, in bank order."""
    return [k for raws in tree[char][action].values() for cams in raws.values() for frames in cams.values() for k in frames]


def check_bank(sprites: SpriteBank) -> None:
    """ValueError, with the render's name, for a bank with a render taller than 3.5 times its width: resized to any width it is
    beyond what ``pa_sprite_augment`` takes (as ``SynthWindowDataset(sprite_augment=)`` refuses it)."""
    for k, (h, w) in enumerate(sprites.shapes):
        if h > 3.5 * w:
            raise ValueError(f"{sprites.paths[k]} ({h} x {w}) is taller than 3.5 : 1: augment_synth_char_crop's pad step is beyond "
                             f"pa_sprite_augment's {sa.H1_MAX} rows at width 128")


def class_id(char: str, action: str, class_type: str = "CHAR+ACTION") -> int:
    """``composite_chars_onto_stage``'s label (:210-213)."""
    if class_type not in ("CHAR", "CHAR+ACTION"):
        raise ValueError('class_type is "CHAR" or "CHAR+ACTION"')
    c = constants.CHAR_LIST.index(char)
    return c if class_type == "CHAR" else len(MOVE_TO_CLASS_ID) * c + MOVE_TO_CLASS_ID[action]


def sample_scenes(rng: np.random.Generator, sprites: SpriteBank, stages: StageBank, n: int, class_type: str = "CHAR+ACTION",
                  augment: Optional[dict] = None):
    """``generate_stage_char_compositions``' loop body and ``composite_chars_onto_stage`` up to the pixels, for ``n`` images, in
    the draw order of this module's docstring. -> ``(resize, aug, scenes, labels)``: the m ``pa_sprite_resize_params`` and m
    ``pa_sprite_aug_params`` records of the m characters that were kept, over all images, in order (record j writes slot j of its
    bank, and the augmentation reads slot j of the resized bank); the n ``pa_scene_params`` records, whose sprites name those
    slots; and per image the list of label rows ``(class_id, cx / W, cy / H, 128 / W, 128 / H)``. m may be 0: the first two
    arrays are then empty and there is nothing to resize or augment. ``augment``: a dict that overrides
    ``augment_synth_char_crop``'s defaults (``sprite_augment.SPRITE_DEFAULTS``)."""
    check_bank(sprites)
    kw = dict(augment or {})
    chars = [c for c in constants.CHAR_LIST if c in sprites.tree]
    if not chars:
        raise ValueError("the sprite bank has no character of constants.CHAR_LIST")
    class_id(chars[0], next(iter(MOVE_TO_CLASS_ID)), class_type)   # (ValueError for an unknown class_type)
    resize, aug, labels = [], [], []
    scenes = np.zeros(int(n), dtype=SCENE_DTYPE)
    for i in range(int(n)):
        drawn = []
        for _ in range(int(rng.integers(1, MAX_NUM_CHAR, endpoint=True))):                 # 1
            char = _choice(rng, chars)                                                     # 2
            action = _choice(rng, sorted(sprites.tree[char].keys()))
            drawn.append((char, action, _choice(rng, _renders(sprites.tree, char, action))))
        stage = int(rng.integers(0, len(stages)))                                          # 3
        H, W = stages.shapes[stage]
        scenes["stage"][i] = stage
        rows = []
        for char, action, render in drawn:                                                 # 4
            h, w = sprites.shapes[render]
            if w < RENDER_SIDE_MIN or h < RENDER_SIDE_MIN:
                continue
            label = class_id(char, action, class_type)
            basewidth = int(rng.integers(BASEWIDTH_MIN, BASEWIDTH_MAX, endpoint=True))
            hsize = int(float(h) * (basewidth / float(w)))
            slot = len(resize)
            resize.append((render, basewidth, hsize, 0))
            aug.append(sa.sample_sprite_params(1, kw, rng, src=[slot]))
            cx, cy = int(rng.normal(W / 2, W / 6)), int(rng.normal(H / 2, H / 6))
            if cx < 0 or cx > W:
                cx = W / 2
            if cy < 0 or cy > H:
                cy = H / 2
            scenes["sprites"][i, len(rows)] = (slot, int(cx - (SIZE / 2)), int(cy - (SIZE / 2)))
            scenes["n_sprites"][i] = len(rows) + 1
            rows.append((label, cx / W, cy / H, SIZE / W, SIZE / H))
        labels.append(rows)
    resize = np.array(resize, dtype=RESIZE_DTYPE) if resize else np.zeros(0, dtype=RESIZE_DTYPE)
    aug = np.concatenate(aug) if aug else np.zeros(0, dtype=sa.PARAMS_DTYPE)
    return resize, aug, scenes, labels


def label_text(rows) -> str:
    """``write_yolo_output``'s file (:66-74) for one image's label rows."""
    return "".join(f"{c} {x} {y} {w} {h}\n" for c, x, y, w, h in rows)


# ---- the entry point ---------------------------------------------------------------------------------------------------------------

def compose_batch(engine, sprites: SpriteBank, stages: StageBank, draw, resized: Optional[ResizedSpriteBank] = None,
                  augmented: Optional[sa.AugmentedSpriteBank] = None, images=None):
    """The device chain of one ``sample_scenes`` draw: resize -> augment -> scenes. -> ``(images, desc)`` of ``compose_scenes``.
    ``resized`` / ``augmented``: banks to reuse (at least as many slots as characters were kept)."""
    resize, aug, scenes, _ = draw
    m = len(resize)
    if augmented is None:
        augmented = sa.AugmentedSpriteBank(engine, max(m, 1))
    if m:
        resized = resize_sprites(engine, sprites, resize, out=resized)
        sa.augment_sprites(engine, resized, aug, out=augmented)
    return compose_scenes(engine, augmented, stages, scenes, images=images)


def generate_stage_char_compositions(sub_dir_name: str, n_generations: int, root: str, sprites: SpriteBank, stages: StageBank,
                                     encoder=None, seed: int = 0, batch: int = 64, overwrite: bool = False, log_interval: int = 50,
                                     bbox_overlay: bool = False, class_type: str = "CHAR+ACTION", augment: Optional[dict] = None) -> List[str]:
    """The reference's entry point (``gen_synth_char_detection.py:265-300``): ``n_generations`` images
    ``root/sub_dir_name/images/comp-i.jpg`` with ``labels/comp-i.txt``, numbered on from the ``images/*.jpg`` that exist unless
    ``overwrite``. Per ``batch`` images: one ``sample_scenes`` draw from ``default_rng([seed, number of the batch's first
    image])`` (so a call that continues a folder draws new images, and the files are a function of the seed, the numbering and
    the batch size), the chain resize -> ``pa_sprite_augment`` -> scenes -> JPEG encode on ``sprites.engine``, one device -> host
    copy of the files (``JpegEncoder.unpack_files``), then the writes. ``encoder``: a ``JpegEncoder`` that takes ``batch`` images
    of the largest stage (default: one made here). -> the image paths written. ``bbox_overlay=True`` raises: the debugging
    rectangles are not built."""
    from .jpeg_encode import JpegEncoder

    if bbox_overlay:
        raise NotImplementedError("bbox_overlay draws cv.rectangle boxes for debugging; not built (DESIGN.md 5.17)")
    engine = sprites.engine
    n_generations, batch = int(n_generations), int(batch)
    if n_generations < 0 or batch < 1:
        raise ValueError("n_generations is at least 0, batch at least 1")
    check_bank(sprites)
    images_dir = os.path.join(root, sub_dir_name, "images")
    labels_dir = os.path.join(root, sub_dir_name, "labels")
    os.makedirs(images_dir, exist_ok=True)
    os.makedirs(labels_dir, exist_ok=True)
    first = 0 if overwrite else len(_glob.glob(os.path.join(images_dir, "*.jpg")))
    if n_generations == 0:
        return []
    batch = min(batch, n_generations)
    max_h, max_w = max(s[0] for s in stages.shapes), max(s[1] for s in stages.shapes)
    if encoder is None:
        encoder = JpegEncoder.for_frames(batch, max_h, max_w, subsampling=2, device=str(engine.device))
    resized = ResizedSpriteBank(engine, MAX_NUM_CHAR * batch, BASEWIDTH_MAX, int(3.5 * BASEWIDTH_MAX))
    augmented = sa.AugmentedSpriteBank(engine, MAX_NUM_CHAR * batch)
    written = []
    for i0 in range(first, first + n_generations, batch):
        b = min(batch, first + n_generations - i0)
        draw = sample_scenes(np.random.default_rng([int(seed), i0]), sprites, stages, b, class_type, augment)
        images, desc = compose_batch(engine, sprites, stages, draw, resized, augmented)
        files, records = encoder.encode_images(images, desc, max_h, max_w, quality=JPEG_QUALITY, subsampling=2, bgr=False)
        blobs = encoder.unpack_files(files, records)
        if any(f is None for f in blobs):
            encoder.overflows()
            raise ValueError("generate_stage_char_compositions: the scenes do not fit the encoder's scratch (max_blocks / scratch_bytes)")
        for k, (blob, rows) in enumerate(zip(blobs, draw[3])):
            i = i0 + k
            if i and i % log_interval == 0:
                print(f"Generated {i} composites for {sub_dir_name}/")
            path = os.path.join(images_dir, f"comp-{i}.jpg")
            with open(path, "wb") as f:
                f.write(blob)
            with open(os.path.join(labels_dir, f"comp-{i}.txt"), "w") as f:
                f.write(label_text(rows))
            written.append(path)
    return written
