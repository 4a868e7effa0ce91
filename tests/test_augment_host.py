"""Augmentation of training crops (``playaid_core_amd/augment.py``, ``csrc/augment.hip``), the parts that need no GPU: the
parameter record and its host-side check, the sampler against the reference's probabilities and limits, and the numpy twin's
own properties (the GPU tests pin the kernel to the twin bit for bit)."""
import ctypes
import os
import re

import numpy as np
import pytest

from playaid_core_amd import _build, _lib, augment

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    _build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def image():
    return np.random.default_rng(11).integers(0, 256, (1, 128, 128, 3), dtype=np.uint8)


def test_params_mirrors_have_the_headers_layout():
    """The ctypes mirror and the numpy dtype against the struct as include/playaid_hip.h declares it (natural alignment)."""
    hdr = open(os.path.join(ROOT, "include", "playaid_hip.h")).read()
    body = re.search(r"typedef struct pa_augment_params \{(.*?)\} pa_augment_params;", hdr, re.S).group(1)
    sizes = {"int32_t": 4, "uint32_t": 4, "float": 4, "uint8_t": 1, "uint64_t": 8}
    off, want = 0, {}
    for ctype, names in re.findall(r"(\w+)\s+([^;]+);", body):
        for name in names.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", name)
            off = (off + sizes[ctype] - 1) // sizes[ctype] * sizes[ctype]
            want[m.group(1)] = off
            off += sizes[ctype] * int(m.group(2) or 1)
    size = (off + 7) // 8 * 8
    assert size == 328 and len(want) == 16
    assert ctypes.sizeof(_lib.pa_augment_params) == size == augment.PARAMS_DTYPE.itemsize
    for name, o in want.items():
        assert getattr(_lib.pa_augment_params, name).offset == o, name
        assert augment.PARAMS_DTYPE.fields[name][1] == o, name
    assert [n for n, _ in _lib.pa_augment_params._fields_] == list(want)
    assert int(re.search(r"#define PA_AUGMENT_QUANTILES (\d+)", hdr).group(1)) == _lib.PA_AUGMENT_QUANTILES == len(augment.quantile_table())
    assert int(re.search(r"#define PA_AUGMENT_MODEL (\d+)", hdr).group(1)) == _lib.PA_AUGMENT_MODEL == augment.FORMATS["model"]
    assert int(re.search(r"#define PA_AUGMENT_U8 (\d+)", hdr).group(1)) == _lib.PA_AUGMENT_U8 == augment.FORMATS["uint8"]


def test_check_accepts_the_sampler_and_refuses_each_bad_field(lib):
    rng = np.random.default_rng(5)
    for level in (1, 2):
        p = augment.sample_params(500, level, rng, src=rng.integers(0, 9, 500))
        assert augment.check_params(p, 9) and p["src"].max() == 8
        assert not augment.check_params(p, 8)
    good = augment.sample_params(3, {"course_dropout": 1.0, "gauss_noise": 1.0, "pixel_dropout": 1.0}, rng)
    good["n_holes"] = 8
    assert augment.check_params(good, 3)

    def bad(field, value, index=None):
        p = good.copy()
        if index is None:
            p[field][1] = value
        else:
            p[field][1][index] = value
        return not augment.check_params(p, 3)

    assert bad("src", 3) and bad("src", -1)
    assert bad("xmap", 128, 7) and bad("ymap", 128, 127)
    assert bad("holes", 125, (7, 0)) and bad("holes", 125, (0, 1))
    assert bad("blur_k", 4) and bad("blur_k", 1) and not bad("blur_k", 3) and not bad("blur_k", 2)
    assert bad("alpha", np.nan) and bad("alpha", np.inf) and bad("alpha", 1.3) and bad("alpha", 0.7)
    assert bad("beta", np.nan) and bad("beta", 0.5) and bad("beta", -0.3)
    assert bad("hue_shift", 257.0) and bad("hue_shift", -np.inf) and bad("sat_shift", 68.0) and bad("val_shift", -5.5)
    assert bad("noise_sigma", -1.0) and bad("noise_sigma", 14.2) and bad("noise_sigma", np.nan)
    assert bad("n_holes", 9) and bad("n_holes", -1)
    assert bad("channel_mask", 7) and bad("channel_mask", 8) and bad("flip", 2)
    assert lib.pa_augment_params_check(None, 1, 1) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_augment_params_check(good.ctypes.data_as(ctypes.c_void_p), 0, 3) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_augment_params_check(good.ctypes.data_as(ctypes.c_void_p), 3, 0) == _lib.PA_ERR_INVALID_ARG
    # what the check refuses is what clamp_params changes; what it accepts comes back as it went in
    assert augment.clamp_params(good, 3).tobytes() == good.tobytes()


def test_librarys_quantile_table_is_the_twins(lib):
    q = np.zeros(_lib.PA_AUGMENT_QUANTILES, np.float32)
    assert lib.pa_augment_quantiles(q.ctypes.data_as(ctypes.c_void_p)) == _lib.PA_OK
    assert np.array_equal(q, augment.quantile_table())
    assert np.all(np.diff(q) > 0) and q[512] == 0 and np.array_equal(q, -q[::-1])
    scipy_stats = pytest.importorskip("scipy.stats")
    assert np.abs(q[1:1024] - scipy_stats.norm.ppf(np.arange(1, 1024) / 1024.0)).max() < 1e-6


def test_levels_are_the_references_literals():
    assert augment.AUGMENT_LEVELS == {
        1: {"horizontal_flip": 0.0, "hard_mode": 0.0, "downscale": 0.1, "resize": 0.4, "course_dropout": 0.9, "channel_dropout": 0.0,
            "pixel_dropout": 0.1, "gauss_noise": 0.4},
        2: {"horizontal_flip": 0.0, "hard_mode": 0.2, "downscale": 0.3, "resize": 0.3, "course_dropout": 0.2, "channel_dropout": 0.01,
            "pixel_dropout": 0.1, "gauss_noise": 0.8},
    }
    assert augment.AUGMENT_DEFAULTS == {"horizontal_flip": 0.5, "hard_mode": 0.1, "downscale": 0.2, "resize": 0.2, "course_dropout": 0.1,
                                        "channel_dropout": 0.0, "pixel_dropout": 0.1, "gauss_noise": 0.5}
    assert augment.MAX_LEVEL == 2 and augment.RAISE_ACCURACY == 0.85


@pytest.mark.parametrize("level", [1, 2, {"horizontal_flip": 0.5, "channel_dropout": 0.3}])
def test_sampler_rates_and_limits(level):
    """Over N = 20 000 draws the share of crops with a stage switched on lies within 5 binomial standard deviations,
    5 sqrt(p (1 - p) / N), of the stage's probability (exactly 0 for p = 0); every value lies inside the reference's limits."""
    n = 20000
    p = augment.sample_params(n, level, np.random.default_rng(1234))
    kw = dict(augment.AUGMENT_DEFAULTS, **level) if isinstance(level, dict) else augment.AUGMENT_LEVELS[level]
    ident = np.arange(128)
    geo_x, geo_y = (p["xmap"] != ident).any(1), (p["ymap"] != ident).any(1)
    assert np.array_equal(geo_x, geo_y)
    bc = (p["alpha"] != 1) | (p["beta"] != 0)
    p_geo = 1 - (1 - kw["downscale"]) * (1 - kw["resize"])
    for name, on, prob in (("flip", p["flip"] == 1, kw["horizontal_flip"]), ("brightness_contrast", bc, 0.3), ("blur", p["blur_k"] != 0, 0.05),
                           ("noise", p["noise_sigma"] > 0, kw["gauss_noise"]), ("pixel_dropout", p["pixel_drop_thr"] != 0, kw["pixel_dropout"]),
                           ("coarse_dropout", p["n_holes"] > 0, kw["course_dropout"]), ("channel_dropout", p["channel_mask"] != 0, kw["channel_dropout"]),
                           ("downscale_or_crop", geo_x, p_geo)):
        share, bound = float(on.mean()), 5 * np.sqrt(prob * (1 - prob) / n)
        assert abs(share - prob) <= bound, (name, share, prob, bound)
    # (a crop side of 128 never occurs and a downscale always repeats pixels, so either of the two shows in the maps)
    f32 = np.float32
    assert p["alpha"].min() >= f32(0.8) and p["alpha"].max() <= f32(1.2) and p["beta"].min() >= f32(-0.2) and p["beta"].max() <= f32(0.4)
    assert set(np.unique(p["blur_k"])) <= {0, 2, 3} and set(np.unique(p["flip"])) <= {0, 1}
    assert np.abs(p["hue_shift"]).max() <= 256 and np.abs(p["sat_shift"]).max() <= 67 and np.abs(p["val_shift"]).max() <= 5
    assert (p["hue_shift"] != 0).all()   # p = 1
    assert p["noise_sigma"].min() >= 0 and float(p["noise_sigma"].max()) ** 2 <= 200 * (1 + 1e-6)
    assert p["pixel_drop_thr"].max() <= 0.3 * 2 ** 32
    assert p["n_holes"].min() >= 0 and p["n_holes"].max() <= 8 and p["holes"].max() <= 124
    assert set(np.unique(p["channel_mask"])) <= {0, 1, 2, 4, 3, 5, 6}
    assert p["xmap"].max() <= 127 and p["ymap"].max() <= 127
    assert (np.diff(p["xmap"].astype(int), axis=1) >= 0).all() and (np.diff(p["ymap"].astype(int), axis=1) >= 0).all()
    span = p["xmap"][geo_x].astype(int)
    assert (span[:, -1] - span[:, 0] >= 88 - 1).all()   # side >= 89 of a picture downscaled by >= 0.7: at least 88 source pixels apart
    assert len(np.unique(p["key"])) == n
    assert augment.check_params(p, n)
    # the draw is a function of the generator's state alone
    assert augment.sample_params(n, level, np.random.default_rng(1234)).tobytes() == p.tobytes()


def test_composed_maps():
    assert np.array_equal(augment.compose_map(None, None), np.arange(128))
    assert np.array_equal(augment.compose_map(None, 128, 0), np.arange(128))        # "no downscale, crop side 128"
    m = augment.compose_map(None, 89, 39)                                            # the largest start of the smallest crop
    assert m[0] == 39 and m[-1] == 39 + int(np.floor(127 * (1.0 / (128 / 89.0)))) <= 127
    m = augment.compose_map(0.7, None)                                               # 128 -> 90 -> 128
    assert m[0] == 0 and len(np.unique(m)) == 90 and m.max() <= 127
    m = augment.compose_map(0.9, 126, 2)
    assert m.max() <= 127 and (np.diff(m.astype(int)) >= 0).all()


def test_twin_identity_flip_hue_and_grey(image):
    ident = augment.identity_params(1)
    assert np.array_equal(augment.augment_reference(image, ident), image)
    assert np.array_equal(augment.augment_reference(image, ident, "model"), image.transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255))
    flip = ident.copy()
    flip["flip"] = 1
    once = augment.augment_reference(image, flip)
    assert np.array_equal(once, image[:, :, ::-1]) and np.array_equal(augment.augment_reference(once, flip), image)
    # hue is periodic: a shift of 180 is a shift of 0. (With all three shifts exactly 0 the stage is skipped altogether, as
    # albumentations does, while 180 alone goes through the lossy 8-bit HSV round trip -- so both sides carry a saturation
    # shift and go through it.)
    a, b = ident.copy(), ident.copy()
    a["sat_shift"], b["sat_shift"] = 10, 10
    b["hue_shift"] = 180
    assert np.array_equal(augment.augment_reference(image, a), augment.augment_reference(image, b))
    b["hue_shift"] = -180
    assert np.array_equal(augment.augment_reference(image, a), augment.augment_reference(image, b))
    b["hue_shift"] = 60
    assert not np.array_equal(augment.augment_reference(image, a), augment.augment_reference(image, b))
    grey = ident.copy()
    grey["sat_shift"] = -255
    out = augment.augment_reference(image, grey)
    assert np.array_equal(out[..., 0], out[..., 1]) and np.array_equal(out[..., 1], out[..., 2])
    assert np.array_equal(out[..., 0], image.max(-1))   # V = max(R, G, B) survives


def test_twin_stage_arithmetic(image):
    """Each integer shortcut of the twin (and the kernel) against the plain formula it stands for."""
    ident = augment.identity_params(1)
    img = image[0].astype(np.int64)
    for k in (2, 3):
        p = ident.copy()
        p["blur_k"] = k
        pad = np.pad(img, ((1, 1), (1, 1), (0, 0)), mode="reflect")
        s = sum(pad[dy:dy + 128, dx:dx + 128] for dy in range(k) for dx in range(k))
        assert np.array_equal(augment.augment_reference(image, p)[0], np.rint(s * (1.0 / (k * k))).astype(np.uint8))   # rint: ties to even
    # the hue table against numpy's own mod
    for shift in (-256.0, -0.5, 0.25, 179.5, 256.0):
        p = ident.copy()
        p["hue_shift"] = shift
        assert np.array_equal(augment._tables(p[0])[1], np.mod(np.arange(256) + np.float64(np.float32(shift)), 180).astype(np.uint8))
    # holes, channels, pixel dropout
    p = ident.copy()
    p["n_holes"], p["channel_mask"] = 2, 0b010
    p["holes"][0, 0], p["holes"][0, 1] = (0, 0), (124, 124)
    out = augment.augment_reference(image, p)[0]
    want = image[0].copy()
    want[0:4, 0:4] = 0
    want[124:128, 124:128] = 0
    want[..., 1] = 0
    assert np.array_equal(out, want)
    p = ident.copy()
    p["pixel_drop_thr"], p["key"] = int(0.3 * 2 ** 32), 99
    out = augment.augment_reference(image, p)[0]
    dropped = (out == 0).all(-1) & ~(image[0] == 0).all(-1)
    assert abs(dropped.mean() - 0.3) <= 5 * np.sqrt(0.3 * 0.7 / 16384) and np.array_equal(out[~dropped], image[0][~dropped])


def test_twin_normal_deviates():
    """N = 2^18 deviates at a fixed key: |mean| <= 5 / sqrt(N), |variance - 1| <= 5 sqrt(2 / N) (the standard errors of a
    normal sample's mean and variance), Kolmogorov-Smirnov distance to the normal below 1.95 / sqrt(N) (the 0.1 % level)."""
    stats = pytest.importorskip("scipy.stats")
    n = 1 << 18
    z = augment.normal_deviates(0x0123456789ABCDEF, np.arange(n)).astype(np.float64)
    assert abs(z.mean()) <= 5 / np.sqrt(n), z.mean()
    assert abs(z.var() - 1) <= 5 * np.sqrt(2.0 / n), z.var()
    d = stats.kstest(z, "norm").statistic
    assert d < 1.95 / np.sqrt(n), d
    # the streams are functions of (key, stream, index): any order, any subset
    idx = np.random.default_rng(0).permutation(n)[:1000]
    assert np.array_equal(augment.normal_deviates(0x0123456789ABCDEF, idx).astype(np.float64), z[idx])
    assert not np.array_equal(augment.normal_deviates(0x0123456789ABCDEE, np.arange(1000)).astype(np.float64), z[:1000])
    # the hash is the encoder trainer's (mix of include/playaid_hip.h)
    from playaid_core_amd import encoder_trainer
    if hasattr(encoder_trainer, "_mix"):
        x = np.arange(1000, dtype=np.uint32) * np.uint32(2654435761)
        assert np.array_equal(np.asarray(encoder_trainer._mix(x)).astype(np.uint64), augment._mix(x))
