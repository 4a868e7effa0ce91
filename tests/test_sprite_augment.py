"""``pa_sprite_augment`` (``csrc/sprite_augment.hip``) against its numpy twin ``sprite_augment.augment_sprites_reference``, bit for
bit: every render shape and alpha plane of the host tests (which pin the twin to Pillow and the INTER_AREA oracle) with every
stage on and off, every canvas side the shrink can make, records that break every rule of the host check, and the compositor
reading the augmented bank."""
import numpy as np
import pytest

from playaid_core_amd import sprite_augment as sa
from playaid_core_amd import synth
from playaid_core_amd import synth_dataset as sd

pytestmark = pytest.mark.gpu

SHAPES = [(128, 128), (150, 200), (200, 150), (300, 100), (64, 64), (256, 256), (384, 384), (60, 90)]
ALPHAS = ["zero", "full", "random", "one", "254"]
NEW_SCALES = [0, 127, 111, 96]   # C = 128, 129, 145, 160


def make_render(h, w, alpha, seed=0):
    rng = np.random.default_rng([h, w, ALPHAS.index(alpha), seed])
    s = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha != "random":
        s[..., 3] = {"zero": 0, "full": 255, "one": 1, "254": 254}[alpha]
    return s


@pytest.fixture(scope="module")
def engine():
    from playaid_core_amd.engine import Engine

    eng = Engine(synth.make_state_dict(seed=7), max_batch_frames=4, max_clip_frames=16, max_frame_height=128, max_frame_width=128)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def renders():
    return [make_render(h, w, a) for h, w in SHAPES for a in ALPHAS] + [make_render(350, 100, "random")]   # ... and the 15-tap limit


@pytest.fixture(scope="module")
def bank(engine, renders):
    b = sd.SpriteBank.from_arrays(engine, {"c": {"a": {"b": {"r": {"0": renders}}}}})
    yield b
    b.close()


def all_stages(src, rng, new_scale=0, sized_crop=True):
    """One record per entry of ``src`` with every stage on, inside the reference's limits."""
    n = len(src)
    p = sa.identity_params(n, src=np.asarray(src), new_scale=new_scale)
    c = sa.canvas_side(p["new_scale"])
    p["flip"] = 1
    p["alpha"], p["beta"] = rng.uniform(0.8, 1.2, n), rng.uniform(-0.2, 0.6, n)
    p["blur_k"] = rng.choice([2, 3], n)
    p["hue_shift"], p["sat_shift"], p["val_shift"] = rng.uniform(-256, 256, n), rng.uniform(-67, 67, n), rng.uniform(-10, 10, n)
    p["noise_sigma"] = np.clip(np.sqrt(rng.uniform(427.63, 500.0, n)).astype(np.float32), sa.SIGMA_MIN, sa.SIGMA_MAX)
    p["pixel_drop_thr"] = sa.DROP_THR
    p["n_holes"] = rng.integers(1, 2, n, endpoint=True)
    p["channel_mask"] = rng.choice([0, 0, 1, 2, 4, 3, 5, 6], n)
    p["key"] = rng.integers(0, 2 ** 64, n, dtype=np.uint64)
    p["sized_crop"] = sized_crop
    for i in range(n):
        ci = int(c[i])
        p["holes"][i] = rng.integers(0, ci - sa.hole_side(ci), (2, 2), endpoint=True)
        scale, side = float(rng.uniform(0.7, 0.9)), int(rng.integers(38, 126, endpoint=True))
        y0, x0 = (int((ci - side + 1) * rng.random()) for _ in range(2))
        sd_ = side if sized_crop else None
        for name, s, st in (("ymap", scale, y0), ("xmap", scale, x0), ("aymap", None, y0), ("axmap", None, x0)):
            m = sa.compose_map(ci, s, sd_, st)
            p[name][i, :len(m)] = m
    return p


def compare(engine, bank, renders, params, check=True):
    want = sa.augment_sprites_reference(renders, params)
    out = sa.augment_sprites(engine, bank, params, check=check)
    got = out.read()
    out.close()
    assert got.shape == want.shape == (len(params), 128, 128, 4)
    bad = [i for i in range(len(params)) if not np.array_equal(got[i], want[i])]
    assert not bad, (bad, [int(params["src"][i]) for i in bad])
    return want


def test_every_shape_and_alpha_with_every_stage_on_and_off(engine, bank, renders):
    rng = np.random.default_rng(41)
    n = len(renders)
    on = all_stages(np.arange(n), rng)
    on["blur_k"][::3] = 0
    want = compare(engine, bank, renders, np.concatenate([sa.identity_params(n), on]))
    for i, r in enumerate(renders):   # identity on a 128 x 128 render is the render; a transparent one stays transparent
        if r.shape[:2] == (128, 128):
            assert np.array_equal(want[i], r)
        if not r[..., 3].any():
            assert not want[i, ..., 3].any() and not want[n + i, ..., 3].any()
    assert not np.array_equal(want[:n], want[n:])


@pytest.mark.parametrize("new_scale", NEW_SCALES)
def test_every_canvas_side(engine, bank, renders, new_scale):
    rng = np.random.default_rng(43 + new_scale)
    src = [SHAPES.index(s) * len(ALPHAS) + ALPHAS.index("random") for s in SHAPES] + [SHAPES.index((200, 150)) * len(ALPHAS) + ALPHAS.index("254"), 40]
    cropped = all_stages(src, rng, new_scale, sized_crop=True)
    whole = all_stages(src, rng, new_scale, sized_crop=False)   # C > 128: through the final resample
    compare(engine, bank, renders, np.concatenate([sa.identity_params(len(src), src=np.asarray(src), new_scale=new_scale), cropped, whole]))


def test_one_sprite_and_a_mixed_batch_with_repeated_sources(engine, bank, renders):
    rng = np.random.default_rng(47)
    compare(engine, bank, renders, sa.sample_sprite_params(1, 2, rng, src=[12]))
    kw = {"horizontal_flip": 0.5, "hard_mode": 0.6, "downscale": 0.5, "resize": 0.5}
    p = sa.sample_sprite_params(23, kw, rng, src=rng.integers(0, 6, 23) * 5 + 2)
    assert len(np.unique(p["src"])) < 23 and len(np.unique(sa.canvas_side(p["new_scale"]))) > 3
    assert p["sized_crop"].any() and not p["sized_crop"].all() and p["n_holes"].any() and p["pixel_drop_thr"].any()
    compare(engine, bank, renders, p)
    # a larger bank than the launch fills, and a second launch into it: slots past n keep what they held
    out = sa.AugmentedSpriteBank(engine, 30)
    assert not out.read().any()
    sa.augment_sprites(engine, bank, p, out=out)
    first = out.read()
    sa.augment_sprites(engine, bank, p[:4][::-1].copy(), out=out)
    second = out.read()
    assert np.array_equal(second[:4], first[:4][::-1]) and np.array_equal(second[4:], first[4:]) and not first[23:].any()
    with pytest.raises(ValueError):
        sa.augment_sprites(engine, bank, p, out=sa.AugmentedSpriteBank(engine, 22))
    out.close()


def test_unchecked_records_are_read_clamped(engine, bank, renders):
    rng = np.random.default_rng(53)
    n_src = len(renders)
    good = all_stages(rng.integers(0, n_src, 24), rng, new_scale=rng.choice(NEW_SCALES, 24), sized_crop=False)
    good["sized_crop"][::2] = 1
    rules = [("src", n_src), ("src", -1), ("src", 2 ** 31 - 1), ("flip", 2), ("flip", -7), ("alpha", 9.0), ("alpha", np.nan), ("alpha", -1.0),
             ("beta", 5.0), ("beta", -np.inf), ("blur_k", 4), ("blur_k", -2), ("hue_shift", 4000.0), ("sat_shift", -900.0), ("val_shift", np.nan),
             ("noise_sigma", 14.0), ("noise_sigma", 1000.0), ("noise_sigma", -3.0), ("pixel_drop_thr", 0xFFFFFFFF), ("pixel_drop_thr", 5),
             ("n_holes", 3), ("n_holes", -1), ("n_holes", 2 ** 31 - 1), ("channel_mask", 7), ("channel_mask", -1), ("new_scale", 95),
             ("new_scale", 128), ("new_scale", -100), ("new_scale", 2 ** 31 - 1), ("sized_crop", 2), ("sized_crop", -1), ("reserved", 77)]
    p = np.resize(good, len(rules)).copy()
    for i, (field, value) in enumerate(rules):
        p[field][i] = value
        assert not sa.check_params(p[i:i + 1], bank), (field, value)
    maps = np.resize(good, 6)
    for i, m in enumerate(sa._MAPS):
        maps[m][i] = 255
    maps["holes"][4] = 255
    maps["n_holes"][4] = 2
    maps["holes"][5] = [[200, 3], [3, 200]]
    maps["n_holes"][5] = 2
    assert not any(sa.check_params(maps[i:i + 1], bank) for i in range(6))
    junk = np.frombuffer(rng.bytes(40 * sa.PARAMS_DTYPE.itemsize), dtype=sa.PARAMS_DTYPE).copy()
    junk["new_scale"][:20] = rng.integers(96, 127, 20, endpoint=True)   # (else hardly any junk record shrinks)
    with pytest.raises(ValueError):
        sa.augment_sprites(engine, bank, p)
    compare(engine, bank, renders, np.concatenate([p, maps, junk]), check=False)


@pytest.mark.parametrize("dim", [32, 97, 128, 256])
def test_composite_from_the_augmented_bank(engine, bank, renders, dim):
    rng = np.random.default_rng(59 + dim)
    stage_arrays = [rng.integers(0, 256, (300, 320, 3), dtype=np.uint8), rng.integers(0, 256, (256, 256, 3), dtype=np.uint8)]
    stages = sd.StageBank.from_arrays(engine, stage_arrays)
    n = 9
    aug = sa.sample_sprite_params(n, {"hard_mode": 0.5, "resize": 0.5, "downscale": 0.5}, rng, src=rng.integers(0, len(renders), n))
    twin_sprites = list(sa.augment_sprites_reference(renders, aug))
    rec = np.zeros(n, dtype=sd.PARAMS_DTYPE)
    rec["sprite"] = rng.permutation(n)
    rec["stage"] = rng.integers(0, 2, n)
    hw = np.array([stage_arrays[s].shape[:2] for s in rec["stage"]])
    rec["stage_x"], rec["stage_y"] = rng.integers(0, hw[:, 1] - dim, endpoint=True), rng.integers(0, hw[:, 0] - dim, endpoint=True)
    rec["paste_dx"], rec["paste_dy"] = rng.integers(-40, 40, n, endpoint=True), rng.integers(-40, 40, n, endpoint=True)
    out = sa.augment_sprites(engine, bank, aug)
    for fmt in ("uint8", "model") if dim == 128 else ("uint8",):
        want = sd.composite_reference(twin_sprites, stage_arrays, rec, dim, fmt)
        got = sd.composite(engine, out, stages, rec, dim, fmt).cpu().numpy()
        assert got.dtype == want.dtype and np.array_equal(got, want), fmt
    out.close()
    stages.close()


def test_the_entry_refuses_what_it_cannot_take(engine, bank):
    tall = sd.SpriteBank.from_arrays(engine, {"c": {"a": {"b": {"r": {"0": [make_render(64, 64, "full"), make_render(351, 100, "full")]}}}}})
    p = sa.identity_params(1)
    for check in (True, False):   # the bank's limits are the library's own, with or without the record check
        with pytest.raises(ValueError, match="taller"):
            sa.augment_sprites(engine, tall, p, check=check)
    tall.close()
    hostless = sa.AugmentedSpriteBank(None, 2)
    with pytest.raises(ValueError):
        sa.augment_sprites(engine, bank, p, out=hostless)
    hostless.close()
