"""Sprite augmentation (``playaid_core_amd/sprite_augment.py``, ``csrc/sprite_augment.hip``), the parts that need no GPU: the
numpy twin's front end against the libraries byte for byte -- ``oracle.resample.cv_resize_area`` for INTER_AREA, the installed
Pillow's own ``ImageOps.pad`` and ``ImageOps.expand`` --, its Compose against ``augment.augment_reference``, the sampler and
the host-side checks of the C ABI. (The GPU tests pin the kernel to the twin bit for bit.)"""
import numpy as np
import pytest
from PIL import Image, ImageOps

from oracle.resample import cv_resize_area
from playaid_core_amd import _build, _lib, augment
from playaid_core_amd import sprite_augment as sa
from playaid_core_amd import synth_dataset as sd

# h x w: copy; wide (vertical pad); tall (premultiplied BICUBIC); 3 : 1 (13 taps); enlarging; the two fast branches; small, wide;
# the entry's own limit, 3.5 : 1 (15 taps)
SHAPES = [(128, 128), (150, 200), (200, 150), (300, 100), (64, 64), (256, 256), (384, 384), (60, 90), (350, 100)]
ALPHAS = ["zero", "full", "random", "one", "254"]
NEW_SCALES = [0, 127, 111, 96]   # C = 128, 129, 145, 160


@pytest.fixture(scope="module", autouse=True)
def lib():
    _build.build()
    return _lib.load()


def make_render(h, w, alpha, seed=0):
    rng = np.random.default_rng([h, w, ALPHAS.index(alpha), seed])
    s = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha != "random":
        s[..., 3] = {"zero": 0, "full": 255, "one": 1, "254": 254}[alpha]
    return s


def front_by_the_libraries(render, new_scale):
    """Lines 274-295 of the reference's function with the libraries it calls (cv2's INTER_AREA as the oracle restates it)."""
    h, w = render.shape[:2]
    img = cv_resize_area(render, 128, int(h * (128 / float(w))))
    img = np.array(ImageOps.pad(Image.fromarray(img), (128, 128), color=(0, 0, 0, 0)))
    if new_scale:
        img = cv_resize_area(img, new_scale, int(128 * (new_scale / float(128))))
        img = np.array(ImageOps.expand(Image.fromarray(img), border=128 - new_scale, fill=(0, 0, 0, 0)))
    return img


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_front_end_equals_oracle_and_pillow(shape):
    for alpha in ALPHAS:
        render = make_render(*shape, alpha)
        for ns in NEW_SCALES:
            want = front_by_the_libraries(render, ns)
            got = sa.front_reference(render, ns)
            c = 256 - ns if ns else 128
            assert want.shape == (c, c, 4) and got.shape == want.shape and got.dtype == np.uint8
            assert np.array_equal(got, want), (shape, alpha, ns)
            # ... and it is what the twin hands out under identity records (C > 128: through the final resample)
            out = sa.augment_sprites_reference([render], sa.identity_params(1, new_scale=ns))[0]
            assert np.array_equal(out, want if c == 128 else cv_resize_area(want, 128, 128)), (shape, alpha, ns)


def _all_stages(n, rng, sized_crop=True, holes=False, drop=False, new_scale=0):
    """Records with every stage on (holes and pixel dropout by request), drawn inside the reference's limits."""
    p = sa.identity_params(n, src=np.zeros(n, dtype=np.int64), new_scale=new_scale)
    c = int(sa.canvas_side(new_scale))
    p["flip"] = 1
    p["alpha"], p["beta"] = rng.uniform(0.8, 1.2, n), rng.uniform(-0.2, 0.6, n)
    p["blur_k"] = rng.choice([2, 3], n)
    p["hue_shift"], p["sat_shift"], p["val_shift"] = rng.uniform(-256, 256, n), rng.uniform(-67, 67, n), rng.uniform(-10, 10, n)
    p["noise_sigma"] = np.sqrt(rng.uniform(427.63, 500.0, n))
    p["channel_mask"] = rng.integers(1, 6, n, endpoint=True)
    p["key"] = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    if drop:
        p["pixel_drop_thr"] = sa.DROP_THR
    if holes:
        p["n_holes"] = rng.integers(1, 2, n, endpoint=True)
        p["holes"] = rng.integers(0, c - sa.hole_side(c), (n, 2, 2), endpoint=True)
    p["sized_crop"] = sized_crop
    for i in range(n):
        scale, side = float(rng.uniform(0.7, 0.9)), int(rng.integers(38, 126, endpoint=True))
        y0, x0 = (int((c - side + 1) * rng.random()) for _ in range(2))
        sd_ = side if sized_crop else None
        for name, s, st in (("ymap", scale, y0), ("xmap", scale, x0), ("aymap", None, y0), ("axmap", None, x0)):
            m = sa.compose_map(c, s, sd_, st)
            p[name][i, :len(m)] = m
    return p


def test_chain_equals_the_existing_twin_on_an_opaque_128_render():
    rng = np.random.default_rng(5)
    render = make_render(128, 128, "full")
    p = _all_stages(6, rng)
    p["blur_k"][:2] = 0
    got = sa.augment_sprites_reference([render], p)
    q = augment.identity_params(6, src=np.zeros(6, dtype=np.int64))
    for f in ("flip", "alpha", "beta", "blur_k", "hue_shift", "sat_shift", "val_shift", "noise_sigma", "channel_mask", "key"):
        q[f] = p[f]
    q["xmap"], q["ymap"] = p["xmap"][:, :128], p["ymap"][:, :128]
    want = augment.augment_reference(render[None, ..., :3], q)
    assert np.array_equal(got[..., :3], want)
    assert len(np.unique(got[..., :3].reshape(6, -1), axis=0)) == 6
    # the mask: opaque everywhere, so a ramp in its place shows the map -- the sized crop's alone, after the flip
    ramp = render.copy()
    ramp[..., 3] = (np.arange(128)[:, None] + 2 * np.arange(128)[None, :]) % 251
    got = sa.augment_sprites_reference([ramp], p)
    for i in range(6):
        assert np.array_equal(got[i, ..., 3], ramp[:, ::-1, 3][p["aymap"][i, :128].astype(int)][:, p["axmap"][i, :128].astype(int)])
        assert not np.array_equal(p["xmap"][i, :128], p["axmap"][i, :128])   # (Downscale is in the image's map only)


@pytest.mark.parametrize("new_scale", NEW_SCALES)
def test_holes_and_pixel_dropout_zero_image_and_mask(new_scale):
    rng = np.random.default_rng(9)
    render = make_render(150, 200, "random")
    c = int(sa.canvas_side(new_scale))
    base = _all_stages(3, rng, sized_crop=False, new_scale=new_scale)
    for m in sa._MAPS:
        base[m] = np.arange(160, dtype=np.uint8)   # no gather: positions are canvas positions
    base["flip"] = 0
    holed = base.copy()
    holed["pixel_drop_thr"] = sa.DROP_THR
    holed["n_holes"] = [1, 2, 2]
    s = sa.hole_side(c)
    assert s == int(c / 3)
    holed["holes"] = rng.integers(0, c - s, (3, 2, 2), endpoint=True)
    holed["holes"][2, 1] = (c - s, c - s)   # the last admissible position
    canvas = sa.front_reference(render, new_scale)
    for i in range(3):
        plain = sa.chain_reference(canvas, sa.clamp_params(base, 1)[i])
        got = sa.chain_reference(canvas, sa.clamp_params(holed, 1)[i])
        assert plain.shape == got.shape == (c, c, 4)
        zero = augment.stream_hash(int(holed["key"][i]), 1, np.arange(c * c).reshape(c, c)) < np.uint32(sa.DROP_THR)
        assert 0.05 < zero.mean() < 0.15
        for hx, hy in holed["holes"][i][: int(holed["n_holes"][i])]:
            zero[hy:hy + s, hx:hx + s] = True
        assert np.all(got[zero] == 0) and np.array_equal(got[~zero], plain[~zero])
        assert np.any(plain[zero][:, 3] != 0)


@pytest.mark.parametrize("new_scale", NEW_SCALES[1:])
def test_final_resample_is_inter_area_of_the_chains_output(new_scale):
    rng = np.random.default_rng(13)
    render = make_render(200, 150, "random")
    p = _all_stages(2, rng, sized_crop=False, holes=True, drop=True, new_scale=new_scale)
    c = 256 - new_scale
    canvas = sa.front_reference(render, new_scale)
    out = sa.augment_sprites_reference([render], p)
    for i in range(2):
        chain = sa.chain_reference(canvas, sa.clamp_params(p, 1)[i])
        assert chain.shape == (c, c, 4)
        assert np.array_equal(out[i], cv_resize_area(chain, 128, 128))


def test_sampler_order_levels_and_frequencies():
    n = 4000
    a = sa.sample_sprite_params(n, {"horizontal_flip": 0.5, "hard_mode": 0.1, "downscale": 0.2, "resize": 0.2}, np.random.default_rng(3))
    b = sa.sample_sprite_params(n, {"horizontal_flip": 1.0, "hard_mode": 1.0, "downscale": 1.0, "resize": 1.0}, np.random.default_rng(3))
    assert np.array_equal(a["key"], b["key"])   # the last draw did not move
    for f in ("alpha", "beta", "blur_k", "hue_shift", "sat_shift", "val_shift", "noise_sigma", "new_scale"):
        assert np.array_equal(a[f], b[f]), f
    on = a["n_holes"] > 0
    assert np.array_equal(a["holes"][on], b["holes"][on]) and np.array_equal(a["n_holes"][on], b["n_holes"][on])
    assert np.all(b["flip"] == 1) and np.all(b["pixel_drop_thr"] == sa.DROP_THR) and np.all(b["sized_crop"] == 1)

    def within(count, prob, what):   # five standard deviations of a binomial count
        assert abs(count - n * prob) <= 5 * np.sqrt(n * prob * (1 - prob)) + 1e-9, (what, count, n * prob)

    within(int((a["new_scale"] != 0).sum()), 0.4, "shrink")
    within(int(a["flip"].sum()), 0.5, "flip")
    within(int((a["alpha"] != 1).sum()), 0.3, "brightness")
    within(int((a["blur_k"] != 0).sum()), 0.05, "blur")
    within(int((a["noise_sigma"] != 0).sum()), 0.2, "noise")
    within(int((a["pixel_drop_thr"] != 0).sum()), 0.1, "pixel dropout")
    within(int((a["n_holes"] != 0).sum()), 0.1, "coarse dropout")
    within(int((a["channel_mask"] != 0).sum()), 0.1, "channel dropout")
    within(int(a["sized_crop"].sum()), 0.2, "sized crop")
    c = sa.canvas_side(a["new_scale"])
    ident = np.array([np.array_equal(r["xmap"][:k], np.arange(k)) for r, k in zip(a, c)])
    within(int((~ident & (a["sized_crop"] == 0)).sum()), 0.2 * 0.8, "downscale alone")
    assert set(np.unique(a["new_scale"])) <= {0, *range(96, 128)} and set(np.unique(a["n_holes"])) == {0, 1, 2}
    assert np.all((a["noise_sigma"] == 0) | ((a["noise_sigma"] >= sa.SIGMA_MIN) & (a["noise_sigma"] <= sa.SIGMA_MAX)))
    assert np.all(np.abs(a["val_shift"]) <= 10) and np.any(np.abs(a["val_shift"]) > 5) and np.any(a["beta"] > 0.4)
    bank = sd.SpriteBank.from_arrays(None, {"c": {"a": {"b": {"r": {"0": [make_render(64, 64, "full")]}}}}})
    for level in (1, 2, {"resize": 0.0}, {}):
        p = sa.sample_sprite_params(500, level, np.random.default_rng(1), src=np.zeros(500, dtype=np.int64))
        assert sa.check_params(p, bank) and np.array_equal(sa.clamp_params(p, 1), p)
    one = sa.sample_sprite_params(n, 1, np.random.default_rng(2))
    assert not one["flip"].any() and not one["pixel_drop_thr"].any() and not one["n_holes"].any() and not one["channel_mask"].any()
    within(int(one["sized_crop"].sum()), 0.1, "level 1 sized crop")
    off = sa.sample_sprite_params(n, {"resize": 0.0}, np.random.default_rng(2))
    assert not off["new_scale"].any() and not off["sized_crop"].any()   # `if resize and output_size`
    for bad in ({"gauss_noise": 0.5}, 0, 3, True, None):
        with pytest.raises(ValueError):
            sa.sample_sprite_params(2, bad, np.random.default_rng(0))
    bank.close()


def _bank(shapes):
    return sd.SpriteBank.from_arrays(None, {"c": {"a": {"b": {"r": {"0": [make_render(h, w, "full") for h, w in shapes]}}}}})


def test_check_refuses_each_rule_once_and_clamp_is_idempotent():
    bank = _bank([(64, 64), (300, 100)])
    good = sa.sample_sprite_params(4, 2, np.random.default_rng(8), src=[0, 1, 0, 1])
    good["new_scale"][1], good["sized_crop"][1] = 100, 0
    for m in sa._MAPS:
        good[m][1] = np.minimum(np.arange(160), 155)
    assert sa.check_params(good, bank)
    c1 = 156
    rules = [("src", 0, 2), ("src", 0, -1), ("flip", 0, 2), ("alpha", 0, 1.3), ("alpha", 0, np.nan), ("beta", 0, 0.61), ("beta", 0, -0.21),
             ("blur_k", 0, 4), ("hue_shift", 0, 257.0), ("sat_shift", 0, -68.0), ("val_shift", 0, 10.5), ("noise_sigma", 0, 14.0),
             ("noise_sigma", 0, 22.5), ("noise_sigma", 0, np.inf), ("pixel_drop_thr", 0, 5), ("n_holes", 0, 3), ("n_holes", 0, -1),
             ("channel_mask", 0, 7), ("channel_mask", 0, -1), ("new_scale", 0, 95), ("new_scale", 0, 128), ("sized_crop", 0, 2),
             ("reserved", 0, 1)]
    for field, i, value in rules:
        bad = good.copy()
        bad[field][i] = value
        assert not sa.check_params(bad, bank), (field, value)
        assert sa.check_status(bad, bank) == _lib.PA_ERR_INVALID_ARG
    for m in sa._MAPS:   # a map entry at C (record 1: C = 156, O = C), and one past O that is not read
        bad = good.copy()
        bad[m][1, 7] = c1
        assert not sa.check_params(bad, bank), m
        ok = good.copy()
        ok[m][1, c1:] = 255
        ok[m][0, 128:] = 255   # (record 0: C = 128)
        ok["new_scale"][0] = 0
        ok[m][0, :128] = np.arange(128)
        assert sa.check_params(ok, bank), m
    bad = good.copy()   # a hole beyond C - S
    bad["n_holes"][1] = 2
    bad["holes"][1] = [[0, 0], [c1 - 52 + 1, 0]]
    assert not sa.check_params(bad, bank)
    bad["holes"][1] = [[0, 0], [c1 - 52, c1 - 52]]
    assert sa.check_params(bad, bank)
    # the bank's limits: 3 : 1 and 3.5 : 1 are taken, anything beyond h1 = 448 is a capacity refusal, a render that resizes to nothing
    # is invalid
    tall, flat, limit = _bank([(64, 64), (351, 100)]), _bank([(1, 200)]), _bank([(350, 100)])
    assert sa.resized_height(300, 100) == 384 and sa.resized_height(350, 100) == 448 and sa.resized_height(351, 100) == 449
    assert sa.resized_height(1, 200) == 0 and sa.check_params(good[:1], limit)
    assert sa.check_status(good[:1], tall) == _lib.PA_ERR_CAPACITY and sa.check_status(good[:1], flat) == _lib.PA_ERR_INVALID_ARG
    with pytest.raises(ValueError):
        sa.front_reference(make_render(351, 100, "full"))
    with pytest.raises(ValueError):
        sa.front_reference(make_render(1, 200, "full"))
    # clamp_params: what passes the check is unchanged; garbage comes out as something that is idempotent
    assert np.array_equal(sa.clamp_params(good, 2), good)
    rng = np.random.default_rng(17)
    junk = np.frombuffer(rng.bytes(64 * sa.PARAMS_DTYPE.itemsize), dtype=sa.PARAMS_DTYPE).copy()
    once = sa.clamp_params(junk, 2)
    assert once.tobytes() == sa.clamp_params(once, 2).tobytes()
    assert once["src"].min() >= 0 and once["src"].max() <= 1 and set(np.unique(once["n_holes"])) <= {0, 1, 2}
    for b in (bank, tall, flat, limit):
        b.close()


def test_the_c_entries_refuse_bad_arguments_without_a_device(lib):
    import ctypes as C

    h = C.c_void_p()
    assert lib.pa_sprite_bank_create(None, 0, C.byref(h)) == _lib.PA_ERR_INVALID_ARG and not h
    assert lib.pa_sprite_bank_create(None, 65536, C.byref(h)) == _lib.PA_ERR_INVALID_ARG and not h
    assert lib.pa_sprite_bank_create(None, 3, None) == _lib.PA_ERR_INVALID_ARG
    out = sa.AugmentedSpriteBank(None, 3)
    assert len(out) == 3 and out.shapes == [(128, 128)] * 3
    p = sa.identity_params(3)
    assert sa.check_params(p, out)   # (a bank of slots is a sprite bank)
    assert lib.pa_sprite_aug_params_check(None, 3, out._h) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_sprite_aug_params_check(p.ctypes.data_as(C.c_void_p), 0, out._h) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_sprite_aug_params_check(p.ctypes.data_as(C.c_void_p), 3, None) == _lib.PA_ERR_INVALID_ARG
    stages = sd.StageBank.from_arrays(None, [np.zeros((200, 200, 3), np.uint8)])
    assert lib.pa_sprite_aug_params_check(p.ctypes.data_as(C.c_void_p), 3, stages._h) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_sprite_augment(None, out._h, p.ctypes.data_as(C.c_void_p), 3, out._h, None) == _lib.PA_ERR_INVALID_ARG
    # the compositor's host check takes the bank of slots
    rec = np.zeros(3, dtype=sd.PARAMS_DTYPE)
    rec["sprite"] = [0, 1, 2]
    assert sd.check_params(rec, out, stages, 128) and sd.check_params(rec, out, stages, 32)
    rec["sprite"][2] = 3
    assert not sd.check_params(rec, out, stages, 128)
    out.close()
    stages.close()


def test_dataset_arguments_without_a_device():
    bank = _bank([(64, 64), (80, 60), (70, 90)])
    stages = sd.StageBank.from_arrays(None, [np.zeros((200, 200, 3), np.uint8)])
    kw = dict(animations=["a"], num_samples=3, num_frames_per_sample=2, seed=5, paste_jitter=40)
    plain = sd.SynthWindowDataset(None, bank, stages, **kw)
    hard = sd.SynthWindowDataset(None, bank, stages, sprite_augment=2, **kw)
    assert plain.sample_sprite_augment(0) is None
    for i in range(3):
        a, b = plain.sample(i), hard.sample(i)
        assert np.array_equal(a[0], b[0]) and a[1:3] == b[1:3]   # the existing draws did not move
        aug = hard.sample_sprite_augment(i)
        assert aug.dtype == sa.PARAMS_DTYPE and np.array_equal(aug["src"], b[0]["sprite"]) and sa.check_params(aug, bank)
        assert aug.tobytes() == hard.sample_sprite_augment(i).tobytes()
    assert hard.sample_sprite_augment(0).tobytes() != hard.sample_sprite_augment(1).tobytes()
    low = sd.SynthWindowDataset(None, bank, stages, **kw)
    seen = []
    for _ in range(4):
        seen.append(low.sprite_augment)
        low.make_synth_more_challenging()
    assert seen == [None, 1, 2, 2]
    custom = sd.SynthWindowDataset(None, bank, stages, sprite_augment={"hard_mode": 1.0}, **kw)
    custom.make_synth_more_challenging()
    assert custom.sprite_augment == {"hard_mode": 1.0}
    for bad in (0, 3, True, "2", {"gauss_noise": 1.0}):
        with pytest.raises(ValueError):
            sd.SynthWindowDataset(None, bank, stages, sprite_augment=bad, **kw)
    with pytest.raises(NotImplementedError, match="sprite_augment=level, paste_jitter=40"):
        sd.SynthWindowDataset(None, bank, stages, synth_difficulty=1, **kw)
    bank.close()
    stages.close()
