"""The reference's augmentation of a character render BEFORE the paste, ``augment_synth_char_crop``
(``dataset_utils.py:255-378``), on the device.

``load_and_augment_frame_to_stage_crop`` passes every render through ``augment_synth_char_crop(render,
**synth_difficulty_map[level])`` when ``synth_difficulty`` is 1 or 2 (``ult_action_dataset.py:103-118``): ``imutils.resize`` to
width 128, ``ImageOps.pad`` to 128 x 128 (BICUBIC on premultiplied alpha for a tall render), now and then a shrink into a
transparent border (a canvas of side C = 129..160), an ``albumentations`` ``Compose`` on RGB with alpha as the mask, and
``imutils.resize`` back to width 128. Here the renders are in a ``SpriteBank`` on the device, so the whole function is one
launch from that bank into a bank of 128 x 128 slots that ``synth_dataset.composite`` takes like any other
(``csrc/sprite_augment.hip``, ``pa_sprite_augment``):

* ``sample_sprite_params`` draws, on the host, what the function and its transforms draw -- one ``pa_sprite_aug_params`` record
  per output sprite;
* ``augment_sprites`` checks the records (``pa_sprite_aug_params_check``), uploads them and launches;
* ``augment_sprites_reference`` is the NUMPY TWIN of the kernel: the same arithmetic, step by step, and the contract the kernel
  is tested against bit for bit. Its albumentations stages are ``augment.augment_reference``'s, on a C x C canvas.

Neither cv2, imutils nor albumentations is a dependency; tests pin the twin's front end, on the CPU, to the installed Pillow's
own ``ImageOps.pad`` / ``ImageOps.expand`` and to the INTER_AREA restatement the crop path is pinned to (DESIGN.md 5.16 lists
what is unverified).

The order of the draws in ``sample_sprite_params`` is fixed (vectors of n per line, from one ``numpy.random.Generator``):

 1. shrink: ``random(n) > 0.6`` (when ``resize`` is not 0), ``new_scale = int(128 * uniform(0.75, 1.0))``; C = 256 - new_scale
 2. flip: ``random(n)`` against ``horizontal_flip``
 3. brightness / contrast: ``random(n)`` against 0.3, ``alpha = 1 + uniform(-0.2, 0.2)``, ``beta = uniform(-0.2, 0.6)``
 4. blur: ``random(n)`` against 0.05, ``k = choice(arange(2, 3 + 1, 2))``
 5. hue, saturation, value shifts: ``uniform(-256, 256)``, ``uniform(-67, 67)``, ``uniform(-10, 10)`` (p = 1)
 6. noise: ``random(n)`` against 0.2, ``sigma = sqrt(uniform(427.63, 500))``
 7. pixel dropout: ``random(n)`` against ``hard_mode`` (probability 0.1: nothing more to draw)
 8. coarse dropout: ``random(n)`` against ``hard_mode``, ``holes = integers(1, 2, inclusive)``, then 2 ``y = random(n)`` and 2 ``x``
    likewise; a hole of side ``S = min(96, int(C / 3))`` starts at ``int((C - S + 1) * draw)``
 9. channel dropout: ``random(n)`` against ``hard_mode``, ``count = integers(1, 2, inclusive)``, a permutation of the three
    channels of which the first ``count`` are dropped
10. downscale: ``random(n)`` against ``downscale``, ``scale = uniform(0.7, 0.9)``
11. sized crop: ``random(n)`` against ``resize`` (when it is not 0), ``side = integers(38, 126, inclusive)``, ``h_start = random(n)``,
    ``w_start = random(n)``; the start is ``int((C - side + 1) * start)``
12. the 64-bit key of the sprite's noise and pixel-dropout streams: ``integers(0, 2**64)``

Every value is drawn for every sprite whether its stage is switched on or not, so one sprite's stages do not shift another's.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional, Sequence, Union

import numpy as np

from . import _lib, augment
from .synth_dataset import SpriteBank, _Bank, area_resize

# ult_action_dataset.py:104-117, value for value
SPRITE_LEVELS = {
    1: {"horizontal_flip": 0.0, "hard_mode": 0.0, "downscale": 0.1, "resize": 0.1},
    2: {"horizontal_flip": 0.0, "hard_mode": 0.2, "downscale": 0.3, "resize": 0.3},
}
# augment_synth_char_crop's own defaults (dataset_utils.py:255-262)
SPRITE_DEFAULTS = {"horizontal_flip": 0.5, "hard_mode": 0.1, "downscale": 0.2, "resize": 0.2}
MAX_LEVEL = 2

SIZE = 128
CANVAS_MAX = _lib.PA_SPRITE_CANVAS_MAX
H1_MAX = _lib.PA_SPRITE_H1_MAX
DROP_THR = _lib.PA_SPRITE_DROP_THR          # floor(0.1 * 2**32)
SIGMA_MIN, SIGMA_MAX = np.float32(20.679216), np.float32(22.360680)   # sqrt(427.63), sqrt(500)

# pa_sprite_aug_params of include/playaid_hip.h as a structured dtype (same offsets as _lib.pa_sprite_aug_params)
PARAMS_DTYPE = np.dtype({
    "names": ["src", "flip", "alpha", "beta", "blur_k", "hue_shift", "sat_shift", "val_shift", "noise_sigma", "pixel_drop_thr",
              "n_holes", "holes", "channel_mask", "new_scale", "sized_crop", "reserved", "xmap", "ymap", "axmap", "aymap", "key"],
    "formats": ["<i4", "<i4", "<f4", "<f4", "<i4", "<f4", "<f4", "<f4", "<f4", "<u4", "<i4", ("u1", (2, 2)), "<i4", "<i4", "<i4", "<i4",
                ("u1", (160,)), ("u1", (160,)), ("u1", (160,)), ("u1", (160,)), "<u8"],
    "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 48, 52, 56, 60, 64, 224, 384, 544, 704],
    "itemsize": 712,
})
assert PARAMS_DTYPE.itemsize == C.sizeof(_lib.pa_sprite_aug_params)
_MAPS = ("xmap", "ymap", "axmap", "aymap")


# ---- parameters ------------------------------------------------------------------------------------------------------------------

def canvas_side(new_scale) -> np.ndarray:
    """C of step c: 256 - new_scale after a shrink, 128 without one (``new_scale`` 0)."""
    ns = np.asarray(new_scale)
    return np.where(ns != 0, 256 - ns, SIZE)


def hole_side(c: int) -> int:
    return min(96, int(c / 3))


def identity_params(n: int, src=None, new_scale=0) -> np.ndarray:
    """n records whose Compose changes nothing: output sprite i is the front end's canvas of source ``src[i]`` (default i),
    resized back to width 128 when ``new_scale`` (a scalar or one value per record; 0: no shrink) made it larger."""
    p = np.zeros(n, dtype=PARAMS_DTYPE)
    p["src"] = np.arange(n) if src is None else np.asarray(src).reshape(n)
    p["alpha"] = 1.0
    p["new_scale"] = new_scale
    for m in _MAPS:
        p[m] = np.arange(CANVAS_MAX, dtype=np.uint8)
    return p


def compose_map(c: int, scale: Optional[float], side: Optional[int], start: int = 0) -> np.ndarray:
    """``augment.compose_map`` on a canvas of side ``c``: the source index of every output index along one axis after
    ``A.Downscale(scale)`` (None: not applied; c -> round(c * scale) -> c) and then ``A.RandomSizedCrop`` of ``side`` pixels from
    ``start`` resized to 128 (None: not applied), both nearest. c entries without the crop, 128 with it."""
    m = np.arange(c, dtype=np.int64)
    if scale is not None:
        small = int(round(c * float(scale)))
        down = augment.nearest_map(small, c, 1.0 / float(scale))
        up = augment.nearest_map(c, small, 1.0 / (c / float(small)))
        m = down[up]
    if side is not None:
        m = m[start + augment.nearest_map(SIZE, int(side), 1.0 / (SIZE / float(side)))]
    return m.astype(np.uint8)


def sample_sprite_params(n: int, level_or_kwargs: Union[int, dict], rng: np.random.Generator, src=None) -> np.ndarray:
    """n ``pa_sprite_aug_params`` records drawn as ``augment_synth_char_crop(**kwargs)`` draws them, in the order of this
    module's docstring. ``level_or_kwargs``: 1 or 2 (``SPRITE_LEVELS``) or a dict of the function's probabilities (missing ones
    take its defaults). ``src``: the source sprite of each record (default ``arange(n)``)."""
    if isinstance(level_or_kwargs, dict):
        unknown = set(level_or_kwargs) - set(SPRITE_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown augment_synth_char_crop arguments: {sorted(unknown)}")
        kw = dict(SPRITE_DEFAULTS, **level_or_kwargs)
    elif not isinstance(level_or_kwargs, bool) and level_or_kwargs in SPRITE_LEVELS:
        kw = SPRITE_LEVELS[level_or_kwargs]
    else:
        raise ValueError(f"sprite_augment level must be one of {sorted(SPRITE_LEVELS)} or a dict, got {level_or_kwargs!r}")
    n = int(n)
    if n < 1:
        raise ValueError("n is at least 1")
    p = identity_params(n, src)
    resize_on = bool(kw["resize"])
    on = (rng.random(n) > 0.6) & resize_on                                                # 1
    p["new_scale"] = np.where(on, (SIZE * rng.uniform(0.75, 1.0, n)).astype(np.int64), 0)
    side_c = canvas_side(p["new_scale"])
    p["flip"] = rng.random(n) < kw["horizontal_flip"]                                     # 2
    on = rng.random(n) < 0.3                                                              # 3
    alpha, beta = 1.0 + rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.6, n)
    p["alpha"], p["beta"] = np.where(on, alpha, 1.0), np.where(on, beta, 0.0)
    on = rng.random(n) < 0.05                                                             # 4
    ks = np.arange(2, 3 + 1, 2)
    p["blur_k"] = np.where(on, ks[rng.integers(0, len(ks), n)], 0)
    p["hue_shift"], p["sat_shift"], p["val_shift"] = rng.uniform(-256, 256, n), rng.uniform(-67, 67, n), rng.uniform(-10, 10, n)   # 5
    on = rng.random(n) < 0.2                                                              # 6
    sigma = np.clip(np.sqrt(rng.uniform(427.63, 500.0, n)).astype(np.float32), SIGMA_MIN, SIGMA_MAX)
    p["noise_sigma"] = np.where(on, sigma, np.float32(0.0))
    on = rng.random(n) < kw["hard_mode"]                                                  # 7
    p["pixel_drop_thr"] = np.where(on, DROP_THR, 0).astype(np.uint32)
    on = rng.random(n) < kw["hard_mode"]                                                  # 8
    holes = rng.integers(1, 2, n, endpoint=True)
    ys, xs = rng.random((n, 2)), rng.random((n, 2))
    room = (side_c - np.array([hole_side(int(c)) for c in side_c]) + 1)[:, None]
    p["n_holes"] = np.where(on, holes, 0)
    p["holes"][:, :, 0], p["holes"][:, :, 1] = (room * xs).astype(np.int64), (room * ys).astype(np.int64)
    on = rng.random(n) < kw["hard_mode"]                                                  # 9
    count = rng.integers(1, 2, n, endpoint=True)
    perm = rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1)
    mask = (1 << perm[:, 0]) | np.where(count == 2, 1 << perm[:, 1], 0)
    p["channel_mask"] = np.where(on, mask, 0)
    ds_on = rng.random(n) < kw["downscale"]                                               # 10
    scale = rng.uniform(0.7, 0.9, n)
    rs_on = (rng.random(n) < kw["resize"]) & resize_on                                    # 11
    side = rng.integers(int(SIZE * 0.3), SIZE - 2, n, endpoint=True)
    h_start, w_start = rng.random(n), rng.random(n)
    p["sized_crop"] = rs_on
    for i in range(n):
        c = int(side_c[i])
        sc = float(scale[i]) if ds_on[i] else None
        sd = int(side[i]) if rs_on[i] else None
        y0, x0 = int((c - side[i] + 1) * h_start[i]), int((c - side[i] + 1) * w_start[i])
        for name, s, start in (("ymap", sc, y0), ("xmap", sc, x0), ("aymap", None, y0), ("axmap", None, x0)):
            m = compose_map(c, s, sd, start)
            p[name][i, :len(m)] = m
    p["key"] = rng.integers(0, 2 ** 64, n, dtype=np.uint64)                               # 12
    return p


def _as_params(params) -> np.ndarray:
    params = np.ascontiguousarray(params)
    if params.dtype != PARAMS_DTYPE or params.ndim != 1 or len(params) < 1:
        raise ValueError("params is a non-empty 1-d array of sprite_augment.PARAMS_DTYPE (sample_sprite_params, identity_params)")
    return params


def check_status(params: np.ndarray, sprites: _Bank) -> int:
    """``pa_sprite_aug_params_check``'s status (host code of the library; no device call): ``PA_OK``, ``PA_ERR_INVALID_ARG`` for a
    record the kernel would clamp or that lies outside the reference's limits and for a bank with a render so flat that it
    resizes to an empty image, ``PA_ERR_CAPACITY`` for a bank with a render taller than 3.5 : 1 (h1 > 448)."""
    params = _as_params(params)
    return int(_lib.load().pa_sprite_aug_params_check(params.ctypes.data_as(C.c_void_p), len(params), sprites._h))


def check_params(params: np.ndarray, sprites: _Bank) -> bool:
    """True when ``check_status`` is ``PA_OK``: the kernel takes every record without clamping anything."""
    return check_status(params, sprites) == _lib.PA_OK


def clamp_params(params: np.ndarray, n_src: int) -> np.ndarray:
    """The records as the kernel reads them (include/playaid_hip.h): ``src`` clamped to ``[0, n_src)``, the floats as
    ``augment.clamp_params`` reads them, ``n_holes`` clamped to 0..2, ``channel_mask & 7``, ``flip`` and ``sized_crop`` 0 / 1, an
    unknown ``blur_k`` and a ``new_scale`` outside 96..127 0, the first O map entries clamped to C - 1 (the rest are not read).
    A record that passes ``check_params`` comes back unchanged."""
    p = _as_params(params).copy()
    p["src"] = np.clip(p["src"], 0, n_src - 1)
    p["flip"] = p["flip"] != 0
    p["sized_crop"] = p["sized_crop"] != 0
    p["alpha"] = augment._sane(p["alpha"], 1.0, 0.0, 4.0)
    p["beta"] = augment._sane(p["beta"], 0.0, -2.0, 2.0)
    p["blur_k"] = np.where(np.isin(p["blur_k"], (2, 3)), p["blur_k"], 0)
    p["hue_shift"] = augment._sane(p["hue_shift"], 0.0, -1024.0, 1024.0)
    p["sat_shift"] = augment._sane(p["sat_shift"], 0.0, -512.0, 512.0)
    p["val_shift"] = augment._sane(p["val_shift"], 0.0, -512.0, 512.0)
    p["noise_sigma"] = augment._sane(p["noise_sigma"], 0.0, 0.0, 256.0)
    p["n_holes"] = np.clip(p["n_holes"], 0, 2)
    p["channel_mask"] = p["channel_mask"] & 7
    p["new_scale"] = np.where((p["new_scale"] >= 96) & (p["new_scale"] <= 127), p["new_scale"], 0)
    side_c = canvas_side(p["new_scale"])
    used = np.arange(CANVAS_MAX)[None, :] < np.where(p["sized_crop"] != 0, SIZE, side_c)[:, None]
    for m in _MAPS:
        p[m] = np.where(used, np.minimum(p[m], (side_c - 1)[:, None]), p[m])
    return p


# ---- the twin --------------------------------------------------------------------------------------------------------------------

def resized_height(h: int, w: int) -> int:
    """h1 of ``imutils.resize(width=128)`` (Python floats)."""
    return int(h * (SIZE / float(w)))


def _bicubic_rows(in_size: int, out_size: int):
    """Pillow's ``precompute_coeffs`` + ``normalize_coeffs_8bpc`` for BICUBIC, per output index ``(first tap, int64 coefficients)``
    -- ``bicubic_coef_row`` of csrc/crop_math.h."""
    def filt(x):
        a = -0.5
        x = abs(x)
        if x < 1.0:
            return ((a + 2.0) * x - (a + 3.0)) * x * x + 1
        if x < 2.0:
            return (((x - 5) * x + 8) * x - 4) * a
        return 0.0

    scale = float(np.float32(in_size)) / out_size
    filterscale = max(scale, 1.0)
    support, ss = 2.0 * filterscale, 1.0 / filterscale
    rows = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size) - xmin
        k = [filt((x + xmin - center + 0.5) * ss) for x in range(xmax)]
        ww = 0.0
        for w in k:
            ww += w
        if ww != 0.0:
            k = [w / ww for w in k]
        rows.append((xmin, np.array([int(-0.5 + w * (1 << 22)) if w < 0 else int(0.5 + w * (1 << 22)) for w in k], dtype=np.int64)))
    return rows


def _bicubic_axis0(img: np.ndarray, out_size: int) -> np.ndarray:
    """One 8-bit pass of ``ImagingResample`` along axis 0 of uint8[in, m, ch]: 2^21 + sum, >> 22, clipped."""
    out = np.empty((out_size,) + img.shape[1:], dtype=np.uint8)
    src = img.astype(np.int64)
    for d, (first, k) in enumerate(_bicubic_rows(img.shape[0], out_size)):
        acc = (1 << 21) + np.tensordot(k, src[first:first + len(k)], axes=(0, 0))
        out[d] = np.clip(acc >> 22, 0, 255)
    return out


def pil_resize_rgba_bicubic(img: np.ndarray, ow: int, oh: int) -> np.ndarray:
    """``Image.fromarray(img).resize((ow, oh), BICUBIC)`` of uint8[h, w, 4] RGBA with both sizes changing, as Pillow does it: to
    premultiplied RGBa (``MULDIV255``), the horizontal then the vertical 8-bit pass on all four channels, back to RGBA."""
    a = img[..., 3:4].astype(np.int64)
    t = img[..., :3].astype(np.int64) * a + 128
    pre = np.concatenate([((t >> 8) + t) >> 8, a], axis=-1).astype(np.uint8)
    hz = _bicubic_axis0(pre.transpose(1, 0, 2), ow).transpose(1, 0, 2)
    vt = _bicubic_axis0(hz, oh).astype(np.int64)
    al = vt[..., 3:4]
    rgb = np.where((al == 0) | (al == 255), vt[..., :3], np.minimum(255 * vt[..., :3] // np.maximum(al, 1), 255))
    return np.concatenate([rgb, al], axis=-1).astype(np.uint8)


def front_reference(render: np.ndarray, new_scale: int = 0) -> np.ndarray:
    """Steps a-c on one uint8[h, w, 4] RGBA render: the C x C canvas the Compose works on (C = 256 - new_scale, or 128)."""
    h, w = render.shape[:2]
    h1 = resized_height(h, w)
    if h1 < 1:
        raise ValueError(f"a {h} x {w} render resizes to an empty image at width 128 (cv2.resize raises)")
    if h1 > H1_MAX:
        raise ValueError(f"a {h} x {w} render is {h1} high at width 128: beyond {H1_MAX} (pa_sprite_augment's limit)")
    t1 = area_resize(np.asarray(render), SIZE, h1)                                         # a
    if h1 == SIZE:                                                                         # b
        canvas = t1
    else:
        canvas = np.zeros((SIZE, SIZE, 4), dtype=np.uint8)
        if h1 < SIZE:   # contain: round(h1 / 128 * 128) == h1, a resize to the same size is a copy
            y = round((SIZE - h1) * 0.5)
            canvas[y:y + h1] = t1
        else:
            w2 = round(SIZE / h1 * SIZE)
            x = round((SIZE - w2) * 0.5)
            canvas[:, x:x + w2] = pil_resize_rgba_bicubic(t1, w2, SIZE)
    if not new_scale:
        return canvas
    ns = int(new_scale)                                                                    # c
    b = SIZE - ns
    out = np.zeros((ns + 2 * b, ns + 2 * b, 4), dtype=np.uint8)
    out[b:b + ns, b:b + ns] = area_resize(canvas, ns, ns)
    return out


def chain_reference(canvas: np.ndarray, p) -> np.ndarray:
    """Step d on a uint8[C, C, 4] canvas with one (clamped) record: uint8[O, O, 4], O = 128 after a sized crop, else C."""
    c = canvas.shape[0]
    rgb, al = canvas[..., :3], canvas[..., 3]
    lut_bc, lut_h, lut_s, lut_v = augment._tables(p)
    if p["flip"]:
        rgb, al = rgb[:, ::-1], al[:, ::-1]
    a = lut_bc[rgb]
    k = int(p["blur_k"])
    if k:
        a = augment.box_blur(a, k)
    if p["hue_shift"] != 0 or p["sat_shift"] != 0 or p["val_shift"] != 0:
        a = augment._hsv_shift(a, lut_h, lut_s, lut_v)
    pos = np.arange(c * c, dtype=np.int64).reshape(c, c)                                   # v * C + u
    sigma = np.float32(p["noise_sigma"])
    if sigma > 0:
        z = augment.normal_deviates(int(p["key"]), pos[..., None] * 3 + np.arange(3), stream=0)
        a = np.clip(a.astype(np.float32) + sigma * z, np.float32(0), np.float32(255)).astype(np.uint8)
    zero = np.zeros((c, c), dtype=bool)
    if p["pixel_drop_thr"] != 0:
        zero |= augment.stream_hash(int(p["key"]), 1, pos) < np.uint32(p["pixel_drop_thr"])
    s = hole_side(c)
    for hx, hy in p["holes"][: int(p["n_holes"])]:
        zero[int(hy):int(hy) + s, int(hx):int(hx) + s] = True
    a = np.where(zero[..., None], np.uint8(0), a)
    al = np.where(zero, np.uint8(0), al)
    for ch in range(3):
        if (int(p["channel_mask"]) >> ch) & 1:
            a[..., ch] = 0
    o = SIZE if p["sized_crop"] else c
    rgb_out = a[p["ymap"][:o].astype(np.int64)][:, p["xmap"][:o].astype(np.int64)]
    al_out = al[p["aymap"][:o].astype(np.int64)][:, p["axmap"][:o].astype(np.int64)]
    return np.concatenate([rgb_out, al_out[..., None]], axis=-1)


def augment_sprites_reference(sprite_arrays: Sequence[np.ndarray], params: np.ndarray) -> np.ndarray:
    """The numpy twin of ``pa_sprite_augment``: RGBA renders and n records -> uint8[n, 128, 128, 4]. The records are read as the
    kernel reads them (``clamp_params``)."""
    params = clamp_params(params, len(sprite_arrays))
    out = np.empty((len(params), SIZE, SIZE, 4), dtype=np.uint8)
    fronts = {}
    for i, p in enumerate(params):
        key = (int(p["src"]), int(p["new_scale"]))
        if key not in fronts:
            fronts[key] = front_reference(np.asarray(sprite_arrays[key[0]]), key[1])
        t = chain_reference(fronts[key], p)
        out[i] = t if t.shape[0] == SIZE else area_resize(t, SIZE, SIZE)                   # e
    return out


# ---- the device ------------------------------------------------------------------------------------------------------------------

class AugmentedSpriteBank(_Bank):
    """A sprite bank of ``n`` 128 x 128 RGBA slots that ``pa_sprite_augment`` writes (``pa_sprite_bank_create``), with the
    kernel's scratch. ``synth_dataset.composite`` takes it as ``sprites``; record ``sprite = i`` reads slot i. ``engine=None``
    makes a bank of sizes alone."""
    KIND = _lib.PA_SYNTH_SPRITES
    CHANNELS = 4

    def __init__(self, engine, n: int):
        n = int(n)
        self.engine = engine
        self._lib = _lib.load()
        h = C.c_void_p()
        rc = self._lib.pa_sprite_bank_create(engine._h if engine is not None else None, n, C.byref(h))
        if rc == _lib.PA_ERR_INVALID_ARG:
            raise ValueError("pa_sprite_bank_create: n is 1..65535")
        if rc != _lib.PA_OK:
            if engine is None:
                raise MemoryError("pa_sprite_bank_create")
            engine._check(rc)
        self._h = h
        self.shapes = [(SIZE, SIZE)] * n

    def read(self, first: int = 0, n: Optional[int] = None) -> np.ndarray:
        """Slots ``first .. first + n - 1`` (default: all from ``first``) as uint8[n, 128, 128, 4] on the host
        (``pa_sprite_bank_read``: waits for the engine's stream)."""
        n = len(self) - first if n is None else int(n)
        out = np.empty((max(n, 0), SIZE, SIZE, 4), dtype=np.uint8)
        rc = self._lib.pa_sprite_bank_read(self.engine._h if self.engine is not None else None, self._h, int(first), n,
                                           out.ctypes.data_as(C.c_void_p), self.engine._stream() if self.engine is not None else None)
        if rc == _lib.PA_ERR_INVALID_ARG:
            raise ValueError("pa_sprite_bank_read: a bank made with an engine, and a range inside its slots")
        self.engine._check(rc)
        return out


def augment_sprites(engine, sprites: SpriteBank, params: np.ndarray, out: Optional[AugmentedSpriteBank] = None, check: bool = True):
    """One ``pa_sprite_augment`` launch on ``engine``: output sprite i is ``augment_synth_char_crop`` of render ``params[i].src``
    of ``sprites``, written to slot i of ``out`` (default: a new ``AugmentedSpriteBank`` of ``len(params)`` slots), which is
    returned. The records go through ``pa_sprite_aug_params_check`` first (ValueError); ``check=False`` skips the per-record
    rules -- the kernel is defined for any bytes and reads them as ``clamp_params`` does -- but not the bank's limits, which the
    library refuses itself. Enqueue only: nothing is read back."""
    import torch

    params = _as_params(params)
    n = len(params)
    if check:
        rc = check_status(params, sprites)
        if rc == _lib.PA_ERR_CAPACITY:
            raise ValueError(f"augment_sprites: a render of the bank is taller than 3.5 : 1 (more than {H1_MAX} rows at width 128)")
        if rc != _lib.PA_OK:
            raise ValueError("augment_sprites: pa_sprite_aug_params_check refused the records (a source outside the bank, a map entry "
                             "or hole outside the canvas, a value outside the reference's limits, or a render that resizes to nothing)")
    if out is None:
        out = AugmentedSpriteBank(engine, n)
    elif not isinstance(out, AugmentedSpriteBank) or len(out) < n:
        raise ValueError(f"out is an AugmentedSpriteBank of at least {n} slots")
    pd = torch.from_numpy(params.view(np.uint8).reshape(n, PARAMS_DTYPE.itemsize)).to(engine.device)
    rc = engine._lib.pa_sprite_augment(engine._h, sprites._h, C.c_void_p(pd.data_ptr()), n, out._h, engine._stream())
    if rc in (_lib.PA_ERR_INVALID_ARG, _lib.PA_ERR_CAPACITY):
        raise ValueError(engine._lib.pa_last_error(engine._h).decode())
    engine._check(rc)
    return out
