"""The reference's training augmentation of crops, ``augment_char_crop`` (``dataset_utils.py:141-252``), on the device.

``UltActionRecogDataset.__getitem__`` passes every crop of every window through
``augment_char_crop(frame, **synth_difficulty_map[level])`` (``ult_action_dataset.py:299-330``): an ``albumentations``
``Compose`` of HorizontalFlip, RandomBrightnessContrast, Blur, HueSaturationValue, GaussNoise, PixelDropout, CoarseDropout,
ChannelDropout, Downscale and RandomSizedCrop on the 128 x 128 RGB crop. Here the crops are already in device memory, so the
chain is one kernel between them and the backbone (``csrc/augment.hip``, ``pa_augment_crops``):

* ``sample_params`` draws, on the host, what the reference's transforms draw -- one ``pa_augment_params`` record per output crop;
* ``augment_crops`` checks the records (``pa_augment_params_check``), uploads them and launches;
* ``augment_reference`` is the NUMPY TWIN of the kernel: the same arithmetic, stage by stage, and the contract the kernel is
  tested against bit for bit (the role ``encoder_trainer.dropout_keep`` has for dropout).

Neither cv2 nor albumentations is a dependency. The twin follows ``dataset_utils.py`` and those libraries' documented
arithmetic as closely as reading allows; bit-equality with cv2 is not claimed (DESIGN.md 5.14 lists what is unverified).

The order of the draws in ``sample_params`` is fixed (vectors of n per line, from one ``numpy.random.Generator``):

 1. flip: ``random(n)`` against ``horizontal_flip``
 2. brightness / contrast: ``random(n)`` against 0.3, ``alpha = 1 + uniform(-0.2, 0.2)``, ``beta = uniform(-0.2, 0.4)``
 3. blur: ``random(n)`` against 0.05, ``k = choice(arange(2, 3 + 1, 2))`` (albumentations steps ``blur_limit`` by 2: only 2)
 4. hue, saturation, value shifts: ``uniform(-256, 256)``, ``uniform(-67, 67)``, ``uniform(-5, 5)`` (p = 1)
 5. noise: ``random(n)`` against ``gauss_noise``, ``sigma = sqrt(uniform(0, 200))``
 6. pixel dropout: ``random(n)`` against ``pixel_dropout``, ``dropout_prob = uniform(0, 0.3)``
 7. coarse dropout: ``random(n)`` against ``course_dropout``, ``max_holes = int(uniform(1, 8))``, ``holes = integers(1, max_holes,
    inclusive)``, then 8 ``y = integers(0, 124, inclusive)`` and 8 ``x`` likewise (the first ``holes`` are used)
 8. channel dropout: ``random(n)`` against ``channel_dropout``, ``count = integers(1, 2, inclusive)``, a permutation of the
    three channels of which the first ``count`` are dropped
 9. downscale: ``random(n)`` against ``downscale``, ``scale = uniform(0.7, 0.9)``
10. sized crop: ``random(n)`` against ``resize``, ``side = integers(89, 126, inclusive)``, ``h_start = random(n)``,
    ``w_start = random(n)``; the start is ``int((128 - side + 1) * start)``
11. the 64-bit key of the crop's noise and pixel-dropout streams: ``integers(0, 2**64)``

Every value is drawn for every crop whether its stage is switched on or not, so one crop's stages do not shift another's draws.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Optional, Union

import numpy as np

from . import _lib

# ult_action_dataset.py:306-326, value for value (``hard_mode`` is passed and never read by augment_char_crop)
AUGMENT_LEVELS = {
    1: {"horizontal_flip": 0.0, "hard_mode": 0.0, "downscale": 0.1, "resize": 0.4, "course_dropout": 0.9, "channel_dropout": 0.0,
        "pixel_dropout": 0.1, "gauss_noise": 0.4},
    2: {"horizontal_flip": 0.0, "hard_mode": 0.2, "downscale": 0.3, "resize": 0.3, "course_dropout": 0.2, "channel_dropout": 0.01,
        "pixel_dropout": 0.1, "gauss_noise": 0.8},
}
# augment_char_crop's own defaults (dataset_utils.py:141-152): what a kwargs dict leaves out
AUGMENT_DEFAULTS = {"horizontal_flip": 0.5, "hard_mode": 0.1, "downscale": 0.2, "resize": 0.2, "course_dropout": 0.1,
                    "channel_dropout": 0.0, "pixel_dropout": 0.1, "gauss_noise": 0.5}
MAX_LEVEL = 2          # cnn_action_detector.py:118-129 stops raising synth_difficulty there
RAISE_ACCURACY = 0.85  # ... and raises it when the epoch's accuracy passes this

SIZE = 128

# pa_augment_params of include/playaid_hip.h as a structured dtype (same offsets as _lib.pa_augment_params)
PARAMS_DTYPE = np.dtype({
    "names": ["src", "flip", "alpha", "beta", "blur_k", "hue_shift", "sat_shift", "val_shift", "noise_sigma", "pixel_drop_thr",
              "n_holes", "holes", "channel_mask", "xmap", "ymap", "key"],
    "formats": ["<i4", "<i4", "<f4", "<f4", "<i4", "<f4", "<f4", "<f4", "<f4", "<u4", "<i4", ("u1", (8, 2)), "<i4", ("u1", (128,)),
                ("u1", (128,)), "<u8"],
    "offsets": [0, 4, 8, 12, 16, 20, 24, 28, 32, 36, 40, 44, 60, 64, 192, 320],
    "itemsize": 328,
})
FORMATS = {"uint8": _lib.PA_AUGMENT_U8, "model": _lib.PA_AUGMENT_MODEL}


# ---- parameters ------------------------------------------------------------------------------------------------------------------

def identity_params(n: int, src=None) -> np.ndarray:
    """n records that change nothing: output crop i is source crop ``src[i]`` (default i), byte for byte."""
    p = np.zeros(n, dtype=PARAMS_DTYPE)
    p["src"] = np.arange(n) if src is None else np.asarray(src).reshape(n)
    p["alpha"] = 1.0
    p["xmap"] = np.arange(SIZE, dtype=np.uint8)
    p["ymap"] = np.arange(SIZE, dtype=np.uint8)
    return p


def nearest_map(dst: int, src: int, inverse_scale: float) -> np.ndarray:
    """The source index of every destination index of ``cv2.resize(..., interpolation=INTER_NEAREST)``:
    ``min(floor(x * inverse_scale), src - 1)`` in float64."""
    return np.minimum(np.floor(np.arange(dst, dtype=np.float64) * np.float64(inverse_scale)), src - 1).astype(np.int64)


def compose_map(scale: Optional[float], side: Optional[int], start: int = 0) -> np.ndarray:
    """uint8[128]: the source index of every output index along one axis after ``A.Downscale(scale)`` (None: not applied) and
    then ``A.RandomSizedCrop`` of ``side`` pixels from ``start`` resized back to 128 (None: not applied), both nearest.

    Downscale is ``cv2.resize(img, None, fx=scale, fy=scale)`` -- the size is ``round(128 * scale)`` and the inverse scale stays
    ``1 / scale`` -- then ``cv2.resize(small, (128, 128))``, whose inverse scale is ``1 / (128 / small)``. The sized crop is
    ``cv2.resize(crop, (128, 128))`` with inverse scale ``1 / (128 / side)``."""
    m = np.arange(SIZE, dtype=np.int64)
    if scale is not None:
        small = int(round(SIZE * float(scale)))   # cv::saturate_cast<int>(double): to nearest, ties to even, as Python's round
        down = nearest_map(small, SIZE, 1.0 / float(scale))
        up = nearest_map(SIZE, small, 1.0 / (SIZE / float(small)))
        m = down[up]
    if side is not None:
        m = m[start + nearest_map(SIZE, int(side), 1.0 / (SIZE / float(side)))]
    return m.astype(np.uint8)


def sample_params(n: int, level_or_kwargs: Union[int, dict], rng: np.random.Generator, src=None) -> np.ndarray:
    """n ``pa_augment_params`` records drawn as ``augment_char_crop(**kwargs)`` draws them, in the order of this module's
    docstring. ``level_or_kwargs``: 1 or 2 (``AUGMENT_LEVELS``) or a dict of ``augment_char_crop``'s probabilities (missing ones
    take its defaults). ``src``: the source crop of each record (default ``arange(n)``)."""
    if isinstance(level_or_kwargs, dict):
        unknown = set(level_or_kwargs) - set(AUGMENT_DEFAULTS)
        if unknown:
            raise ValueError(f"unknown augment_char_crop arguments: {sorted(unknown)}")
        kw = dict(AUGMENT_DEFAULTS, **level_or_kwargs)
    elif level_or_kwargs in AUGMENT_LEVELS:
        kw = AUGMENT_LEVELS[level_or_kwargs]
    else:
        raise ValueError(f"synth_difficulty level must be one of {sorted(AUGMENT_LEVELS)} or a dict, got {level_or_kwargs!r}")
    n = int(n)
    if n < 1:
        raise ValueError("n is at least 1")
    p = identity_params(n, src)
    on = rng.random(n) < kw["horizontal_flip"]                                            # 1
    p["flip"] = on
    on = rng.random(n) < 0.3                                                              # 2
    alpha, beta = 1.0 + rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.4, n)
    p["alpha"], p["beta"] = np.where(on, alpha, 1.0), np.where(on, beta, 0.0)
    on = rng.random(n) < 0.05                                                             # 3
    ks = np.arange(2, 3 + 1, 2)
    p["blur_k"] = np.where(on, ks[rng.integers(0, len(ks), n)], 0)
    p["hue_shift"], p["sat_shift"], p["val_shift"] = rng.uniform(-256, 256, n), rng.uniform(-67, 67, n), rng.uniform(-5, 5, n)   # 4
    on = rng.random(n) < kw["gauss_noise"]                                                # 5
    p["noise_sigma"] = np.where(on, np.sqrt(rng.uniform(0.0, 200.0, n)), 0.0)
    on = rng.random(n) < kw["pixel_dropout"]                                              # 6
    thr = np.minimum(np.floor(rng.uniform(0.0, 0.3, n) * 4294967296.0), 4294967295.0)
    p["pixel_drop_thr"] = np.where(on, thr, 0.0).astype(np.uint32)
    on = rng.random(n) < kw["course_dropout"]                                             # 7
    max_holes = rng.uniform(1.0, 8.0, n).astype(np.int64)
    holes = rng.integers(1, max_holes, endpoint=True)
    ys, xs = rng.integers(0, 124, (n, 8), endpoint=True), rng.integers(0, 124, (n, 8), endpoint=True)
    p["n_holes"] = np.where(on, holes, 0)
    p["holes"][:, :, 0], p["holes"][:, :, 1] = xs, ys
    on = rng.random(n) < kw["channel_dropout"]                                            # 8
    count = rng.integers(1, 2, n, endpoint=True)
    perm = rng.permuted(np.tile(np.arange(3), (n, 1)), axis=1)
    mask = (1 << perm[:, 0]) | np.where(count == 2, 1 << perm[:, 1], 0)
    p["channel_mask"] = np.where(on, mask, 0)
    ds_on = rng.random(n) < kw["downscale"]                                               # 9
    scale = rng.uniform(0.7, 0.9, n)
    rs_on = rng.random(n) < kw["resize"]                                                  # 10
    side = rng.integers(89, 126, n, endpoint=True)
    h_start, w_start = rng.random(n), rng.random(n)
    for i in np.nonzero(ds_on | rs_on)[0]:
        sc = float(scale[i]) if ds_on[i] else None
        sd = int(side[i]) if rs_on[i] else None
        p["ymap"][i] = compose_map(sc, sd, int((SIZE - side[i] + 1) * h_start[i]))
        p["xmap"][i] = compose_map(sc, sd, int((SIZE - side[i] + 1) * w_start[i]))
    p["key"] = rng.integers(0, 2 ** 64, n, dtype=np.uint64)                               # 11
    return p


def check_params(params: np.ndarray, n_src: int) -> bool:
    """``pa_augment_params_check`` (host code of the library; no device call): True when every record is one the kernel takes
    without clamping anything and lies inside the reference's limits."""
    params = _as_params(params)
    rc = _lib.load().pa_augment_params_check(params.ctypes.data_as(C.c_void_p), len(params), int(n_src))
    return rc == _lib.PA_OK


def _as_params(params) -> np.ndarray:
    params = np.ascontiguousarray(params)
    if params.dtype != PARAMS_DTYPE or params.ndim != 1 or len(params) < 1:
        raise ValueError("params is a non-empty 1-d array of augment.PARAMS_DTYPE (sample_params, identity_params)")
    return params


def _sane(x, ident, lo, hi) -> np.ndarray:
    x = np.asarray(x, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        return np.where(np.isfinite(x), np.minimum(np.maximum(x, np.float32(lo)), np.float32(hi)), np.float32(ident)).astype(np.float32)


def clamp_params(params: np.ndarray, n_src: int) -> np.ndarray:
    """The records as the kernel reads them (include/playaid_hip.h): ``src`` clamped to ``[0, n_src)``, maps ``& 127``, ``n_holes``
    clamped to 0..8, ``channel_mask & 7``, ``flip`` 0 / 1, an unknown ``blur_k`` 0, floats that are not finite replaced by their
    identity value and finite ones clamped. A record that passes ``check_params`` comes back unchanged."""
    p = _as_params(params).copy()
    p["src"] = np.clip(p["src"], 0, n_src - 1)
    p["flip"] = p["flip"] != 0
    p["alpha"] = _sane(p["alpha"], 1.0, 0.0, 4.0)
    p["beta"] = _sane(p["beta"], 0.0, -2.0, 2.0)
    p["blur_k"] = np.where(np.isin(p["blur_k"], (2, 3)), p["blur_k"], 0)
    p["hue_shift"] = _sane(p["hue_shift"], 0.0, -1024.0, 1024.0)
    p["sat_shift"] = _sane(p["sat_shift"], 0.0, -512.0, 512.0)
    p["val_shift"] = _sane(p["val_shift"], 0.0, -512.0, 512.0)
    p["noise_sigma"] = _sane(p["noise_sigma"], 0.0, 0.0, 256.0)
    p["n_holes"] = np.clip(p["n_holes"], 0, 8)
    p["channel_mask"] = p["channel_mask"] & 7
    p["xmap"] &= 127
    p["ymap"] &= 127
    return p


# ---- the random streams ----------------------------------------------------------------------------------------------------------

_M32 = np.uint64(0xFFFFFFFF)


def _mix(x: np.ndarray) -> np.ndarray:
    """``mix`` of include/playaid_hip.h on uint32 values held in uint64 arrays."""
    x = np.asarray(x, dtype=np.uint64) & _M32
    x = x ^ (x >> np.uint64(16))
    x = (x * np.uint64(0x7FEB352D)) & _M32
    x = x ^ (x >> np.uint64(15))
    x = (x * np.uint64(0x846CA68B)) & _M32
    return x ^ (x >> np.uint64(16))


def stream_key(key: int, stream: int) -> int:
    """The 32-bit key of one of a crop's streams (0: noise, 1: pixel dropout)."""
    key = int(key) & 0xFFFFFFFFFFFFFFFF
    k = _mix((key + 0x9E3779B9) & 0xFFFFFFFF)
    k = _mix(int(k) ^ (key >> 32))
    return int(_mix(int(k) ^ (((stream + 1) * 0x85EBCA6B) & 0xFFFFFFFF)))


def stream_hash(key: int, stream: int, index: np.ndarray) -> np.ndarray:
    """r(i) = mix(mix(i ^ ks) + ks) as uint32: a function of (key, stream, element index) alone."""
    ks = np.uint64(stream_key(key, stream))
    return _mix(_mix(np.asarray(index, dtype=np.uint64) ^ ks) + ks).astype(np.uint32)


def _norm_cdf(x: float) -> float:
    return 0.5 * math.erfc(-x * 0.70710678118654752440)


def _norm_ppf_lower(p: float) -> float:
    lo, hi = -40.0, 0.0
    for _ in range(200):
        mid = 0.5 * (lo + hi)
        if _norm_cdf(mid) < p:
            lo = mid
        else:
            hi = mid
    return 0.5 * (lo + hi)


_QUANTILES = None


def quantile_table() -> np.ndarray:
    """float32[1025], ``pa_augment_quantiles`` computed here: q[j] = the standard normal quantile at j / 1024 (float64, rounded
    once); q[0] = -q[1024] closes the outermost cells so that they keep the normal's second moment over their 1 / 1024."""
    global _QUANTILES
    if _QUANTILES is None:
        q = np.zeros(1025, dtype=np.float64)
        for j in range(1, 512):
            q[j] = _norm_ppf_lower(j / 1024.0)
            q[1024 - j] = -q[j]
        a = -_norm_ppf_lower(1.0 / 1024.0)
        phi = math.exp(-0.5 * a * a) / math.sqrt(2.0 * 3.14159265358979323846)
        target = 3.0 * (1024.0 * a * phi + 1.0)
        c = 0.5 * (-a + math.sqrt(a * a - 4.0 * (a * a - target)))
        q[1024], q[0] = c, -c
        _QUANTILES = q.astype(np.float32)
    return _QUANTILES


def normal_deviates(key: int, index: np.ndarray, stream: int = 0) -> np.ndarray:
    """float32 standard normal deviates of the elements ``index``: the quantile table interpolated linearly at the hash's 32
    bits -- the cell from the upper 10, the position in it from the lower 22 (float32: one multiply, one subtract, one multiply,
    one add)."""
    r = stream_hash(key, stream, index)
    q = quantile_table()
    cell = (r >> np.uint32(22)).astype(np.int64)
    f = (r & np.uint32(0x3FFFFF)).astype(np.float32) * np.float32(1.0 / 4194304.0)
    q0 = q[cell]
    return (q0 + f * (q[cell + 1] - q0)).astype(np.float32)


# ---- the twin --------------------------------------------------------------------------------------------------------------------

def _tables(p):
    """The crop's four 256-byte tables: brightness / contrast (float32), hue / saturation / value (float64)."""
    k32 = np.arange(256, dtype=np.float32)
    bc = np.clip(k32 * np.float32(p["alpha"]) + np.float32(p["beta"]) * np.float32(255.0), np.float32(0), np.float32(255)).astype(np.uint8)
    k = np.arange(256, dtype=np.float64)
    t = k + np.float64(p["hue_shift"])
    r = t - np.floor(t * (1.0 / 180.0)) * 180.0
    r = np.where(r < 0.0, r + 180.0, r)
    r = np.where(r >= 180.0, r - 180.0, r)
    sat = np.clip(k + np.float64(p["sat_shift"]), 0.0, 255.0)
    val = np.clip(k + np.float64(p["val_shift"]), 0.0, 255.0)
    return bc, r.astype(np.uint8), sat.astype(np.uint8), val.astype(np.uint8)


_DIV = None


def _div_tables():
    global _DIV
    if _DIV is None:
        i = np.arange(1, 256, dtype=np.float64)
        sdiv, hdiv = np.zeros(256, np.int64), np.zeros(256, np.int64)
        sdiv[1:] = np.rint(float(255 << 12) / (1.0 * i))
        hdiv[1:] = np.rint(float(180 << 12) / (6.0 * i))
        _DIV = (sdiv, hdiv)
    return _DIV


def _hsv_shift(a: np.ndarray, lut_h, lut_s, lut_v) -> np.ndarray:
    """uint8[..., 3] RGB -> OpenCV's 8-bit HSV (integer form) -> the three tables -> RGB (float32, OpenCV's sector form)."""
    sdiv, hdiv = _div_tables()
    r, g, b = (a[..., c].astype(np.int64) for c in range(3))
    vmax, vmin = np.maximum(r, np.maximum(g, b)), np.minimum(r, np.minimum(g, b))
    diff = vmax - vmin
    s8 = ((diff * sdiv[vmax] + (1 << 11)) >> 12) & 255
    h = np.where(vmax == r, g - b, np.where(vmax == g, b - r + 2 * diff, r - g + 4 * diff))
    h = (h * hdiv[diff] + (1 << 11)) >> 12
    h = np.clip(np.where(h < 0, h + 180, h), 0, 255)
    H, S, V = lut_h[h], lut_s[s8], lut_v[vmax]
    f32 = np.float32
    vf = V.astype(f32) * (f32(1.0) / f32(255.0))
    sf = S.astype(f32) * (f32(1.0) / f32(255.0))
    hf = H.astype(f32) * (f32(6.0) / f32(180.0))
    sector = hf.astype(np.int32)
    hf = hf - sector.astype(f32)
    bad = sector >= 6
    sector, hf = np.where(bad, 0, sector), np.where(bad, f32(0), hf)
    one = f32(1.0)
    t1 = vf * (one - sf)
    t2 = vf * (one - sf * hf)
    t3 = vf * (one - sf * (one - hf))
    tab = np.stack([vf, t1, t2, t3])   # sector -> (b, g, r) rows of tab
    sec = np.array([[1, 3, 0], [1, 0, 2], [3, 0, 1], [0, 2, 1], [0, 1, 3], [2, 1, 0]])
    pick = lambda col: np.take_along_axis(tab, sec[sector, col][None], axis=0)[0]
    bf, gf, rf = pick(0), pick(1), pick(2)
    grey = S == 0
    out = np.stack([np.where(grey, vf, rf), np.where(grey, vf, gf), np.where(grey, vf, bf)], axis=-1)
    return np.clip(np.rint(out * f32(255.0)), 0, 255).astype(np.uint8)


def box_blur(a: np.ndarray, k: int) -> np.ndarray:
    """``cv2.blur(a, (k, k))`` of uint8[h, w, 3] for k = 2 or 3: the window starts at -1 (OpenCV's anchor k / 2), the border is
    reflect-101, the sum is divided by k * k to nearest, ties to even."""
    h, w = a.shape[:2]
    pad = np.pad(a.astype(np.int64), ((1, 1), (1, 1), (0, 0)), mode="reflect")
    s = sum(pad[dy:dy + h, dx:dx + w] for dy in range(k) for dx in range(k))
    if k == 2:
        q, rem = s >> 2, s & 3
        return (q + ((rem == 3) | ((rem == 2) & ((q & 1) == 1)))).astype(np.uint8)
    return ((2 * s + 9) // 18).astype(np.uint8)


def _augment_one(img: np.ndarray, p) -> np.ndarray:
    lut_bc, lut_h, lut_s, lut_v = _tables(p)
    a = lut_bc[img[:, ::-1] if p["flip"] else img]                                        # 1, 2
    k = int(p["blur_k"])
    if k:                                                                                  # 3
        a = box_blur(a, k)
    if p["hue_shift"] != 0 or p["sat_shift"] != 0 or p["val_shift"] != 0:                  # 4
        a = _hsv_shift(a, lut_h, lut_s, lut_v)
    pos = np.arange(SIZE * SIZE, dtype=np.int64).reshape(SIZE, SIZE)                       # v * 128 + u
    sigma = np.float32(p["noise_sigma"])
    if sigma > 0:                                                                          # 5
        z = normal_deviates(int(p["key"]), pos[..., None] * 3 + np.arange(3), stream=0)
        a = np.clip(a.astype(np.float32) + sigma * z, np.float32(0), np.float32(255)).astype(np.uint8)
    zero = np.zeros((SIZE, SIZE), dtype=bool)
    if p["pixel_drop_thr"] != 0:                                                           # 6
        zero |= stream_hash(int(p["key"]), 1, pos) < np.uint32(p["pixel_drop_thr"])
    for hx, hy in p["holes"][: int(p["n_holes"])]:                                         # 7
        zero[int(hy):int(hy) + 4, int(hx):int(hx) + 4] = True
    a = np.where(zero[..., None], np.uint8(0), a)
    for c in range(3):                                                                     # 8
        if (int(p["channel_mask"]) >> c) & 1:
            a[..., c] = 0
    return a[p["ymap"].astype(np.int64)][:, p["xmap"].astype(np.int64)]                    # 9


def augment_reference(crops_uint8: np.ndarray, params: np.ndarray, out_format: str = "uint8") -> np.ndarray:
    """The numpy twin of ``pa_augment_crops``: ``crops_uint8`` uint8[n_src, 128, 128, 3] (RGB) and n records ->
    uint8[n, 128, 128, 3] (``"uint8"``) or float32[n, 3, 128, 128] with value ``float32(byte) / float32(255)`` (``"model"``).
    The records are read as the kernel reads them (``clamp_params``)."""
    if out_format not in FORMATS:
        raise ValueError(f"out_format must be one of {sorted(FORMATS)}")
    crops = np.asarray(crops_uint8)
    if crops.dtype != np.uint8 or crops.ndim != 4 or crops.shape[1:] != (SIZE, SIZE, 3) or len(crops) < 1:
        raise ValueError(f"crops are uint8[n_src, {SIZE}, {SIZE}, 3], got {crops.dtype}{tuple(crops.shape)}")
    params = clamp_params(params, len(crops))
    out = np.stack([_augment_one(crops[int(p["src"])], p) for p in params])
    if out_format == "uint8":
        return out
    return np.ascontiguousarray(out.transpose(0, 3, 1, 2)).astype(np.float32) / np.float32(255.0)


# ---- the device ------------------------------------------------------------------------------------------------------------------

def augment_crops(engine, src_dev, params: np.ndarray, out_format: str = "uint8", out=None, check: bool = True):
    """One ``pa_augment_crops`` launch on ``engine`` (an ``engine.Engine``): ``src_dev`` a contiguous uint8 device tensor
    [n_src, 128, 128, 3] (RGB), ``params`` n records (``sample_params``) -> a device tensor uint8[n, 128, 128, 3] (``"uint8"``)
    or float32[n, 3, 128, 128] (``"model"``: the input of ``pa_backbone_windows`` / ``CNNActionDetector.forward``). The records
    go through ``pa_augment_params_check`` first (ValueError); ``check=False`` skips that -- the kernel is defined for any
    bytes and reads them as ``clamp_params`` does. Enqueue only: nothing is read back."""
    import torch

    if out_format not in FORMATS:
        raise ValueError(f"out_format must be one of {sorted(FORMATS)}")
    if not isinstance(src_dev, torch.Tensor) or src_dev.dtype != torch.uint8 or not src_dev.is_cuda or not src_dev.is_contiguous() \
            or src_dev.dim() != 4 or tuple(src_dev.shape[1:]) != (SIZE, SIZE, 3) or src_dev.shape[0] < 1:
        raise ValueError(f"src_dev is a contiguous uint8 device tensor [n_src, {SIZE}, {SIZE}, 3]")
    params = _as_params(params)
    n, n_src = len(params), int(src_dev.shape[0])
    if check and not check_params(params, n_src):
        raise ValueError("augment_crops: pa_augment_params_check refused the records (a source outside the array, a map entry or "
                         "hole outside the image, or a value outside the reference's limits)")
    pd = torch.from_numpy(params.view(np.uint8).reshape(n, PARAMS_DTYPE.itemsize)).to(engine.device)
    shape, dtype = ((n, SIZE, SIZE, 3), torch.uint8) if out_format == "uint8" else ((n, 3, SIZE, SIZE), torch.float32)
    if out is None:
        out = torch.empty(shape, dtype=dtype, device=engine.device)
    elif tuple(out.shape) != shape or out.dtype != dtype or not out.is_cuda or not out.is_contiguous():
        raise ValueError(f"out is a contiguous {dtype} device tensor {shape}")
    engine._check(engine._lib.pa_augment_crops(engine._h, C.c_void_p(src_dev.data_ptr()), n_src, C.c_void_p(pd.data_ptr()), n,
                                               FORMATS[out_format], C.c_void_p(out.data_ptr()), engine._stream()))
    return out
