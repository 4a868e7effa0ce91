"""``playaid_core_amd.detect_composite`` on the CPU: the numpy twins of ``pa_sprite_resize`` and ``pa_scene_composite`` against
the installed Pillow's own ``Image.resize`` and ``Image.paste``, byte for byte; the sampler's draws, its two quirks and its
label text; the host checks of the records (library code, no device)."""
import os
import re
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import detect_composite_cases as cases  # noqa: E402

from playaid_core_amd import _lib  # noqa: E402
from playaid_core_amd import detect_composite as dc  # noqa: E402
from playaid_core_amd import sprite_augment as sa  # noqa: E402
from playaid_core_amd import synth_dataset as sd  # noqa: E402


# ---- the resize twin ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shape,target", cases.RESIZE_CASES + cases.ONE_PASS_CASES)
def test_resize_twin_equals_pillow(shape, target):
    for alpha in cases.ALPHAS:
        r = cases.make_render(*shape, alpha)
        want = np.asarray(Image.fromarray(r).resize(target))
        got = dc.resize_sprites_reference([r], dc.resize_params([0], [target[0]], [target[1]]))[0]
        assert got.shape == want.shape == (target[1], target[0], 4)
        assert np.array_equal(got, want), (shape, target, alpha, int(np.abs(got.astype(int) - want).max()))


def test_resize_is_premultiplied_and_the_equal_size_is_a_copy():
    """What the header says about the arithmetic: plain channels give other bytes, and the premultiply round trip is not the
    identity, so a resize to the same size must be a copy."""
    r = cases.make_render(120, 110, "random")
    twin = dc.pil_resize_rgba(r, 60, 65)
    plain = sa._bicubic_axis0(sa._bicubic_axis0(r.transpose(1, 0, 2), 60).transpose(1, 0, 2), 65)
    assert not np.array_equal(twin, plain)
    assert np.array_equal(dc.pil_resize_rgba(r, 110, 120), r)
    a = r[..., 3:4].astype(np.int64)
    t = r[..., :3].astype(np.int64) * a + 128
    pre = ((t >> 8) + t) >> 8
    back = np.where((a == 0) | (a == 255), pre, np.minimum(255 * pre // np.maximum(a, 1), 255))
    assert not np.array_equal(back, r[..., :3])


def test_tap_bound_of_the_header():
    """83 taps for 1024 -> 50, and one pass's table -- out rows of min(ksize, in) taps -- fits PA_SPRITE_RESIZE_COEFS for every
    pair of sizes the call takes."""
    def ksize(i, o):
        return int(np.ceil(2.0 * max(float(np.float32(i)) / o, 1.0))) * 2 + 1

    assert ksize(1024, 50) == 83
    assert 80 <= max(len(k) for _, k in sa._bicubic_rows(1024, 50)) <= 83   # (Pillow's own allocation per row is ksize)
    i = np.arange(1, _lib.PA_SYNTH_SPRITE_MAX + 1, dtype=np.float64)[:, None]
    o = np.arange(1, _lib.PA_SPRITE_RESIZE_H_MAX + 1, dtype=np.float64)[None, :]
    k = np.ceil(2.0 * np.maximum(i.astype(np.float32).astype(np.float64) / o, 1.0)) * 2 + 1
    assert int((o * np.minimum(k, i)).max()) <= _lib.PA_SPRITE_RESIZE_COEFS
    hdr = open(os.path.join(ROOT, "include", "playaid_hip.h")).read()
    for name in ("PA_SPRITE_RESIZE_W_MAX", "PA_SPRITE_RESIZE_H_MAX", "PA_SPRITE_RESIZE_COEFS", "PA_SCENE_SPRITES_MAX"):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == getattr(_lib, name), name
    assert int(re.search(r"#define PA_ABI_VERSION (\d+)", hdr).group(1)) == 15 == _lib.PA_ABI_VERSION
    assert _lib.PA_SPRITE_RESIZE_W_MAX >= 150 and _lib.PA_SPRITE_RESIZE_H_MAX >= int(3.5 * 150)


def test_resize_clamps():
    p = dc.resize_params([-3, 9, 1], [0, 1000, 50], [-5, 9999, 60])
    p["reserved"] = 7
    c = dc.resize_clamp_params(p, 4, 150, 525)
    assert c["src"].tolist() == [0, 3, 1] and c["out_w"].tolist() == [1, 150, 50] and c["out_h"].tolist() == [1, 525, 60]
    assert not c["reserved"].any()
    ok = dc.resize_params([1], [50], [60])
    assert np.array_equal(dc.resize_clamp_params(ok, 4), ok)


def test_resize_record_check_refuses_each_rule():
    """pa_sprite_resize_params_check with banks of sizes alone (engine=None): no device."""
    renders = [cases.make_render(120, 110, "random"), cases.make_render(300, 1024, "full")]
    bank = sd.SpriteBank.from_arrays(None, {"c": {"a": {"b": {"r": {"0": renders}}}}})
    out = dc.ResizedSpriteBank(None, 3, 150, 525)
    assert len(out) == 3 and out.shapes == [(1, 1)] * 3
    good = dc.resize_params([0, 1, 1], [50, 150, 1], [60, 525, 1])
    assert dc.resize_check_status(good, bank, out) == _lib.PA_OK
    for field, i, value, want in (("src", 0, -1, _lib.PA_ERR_INVALID_ARG), ("src", 1, 2, _lib.PA_ERR_INVALID_ARG),
                                  ("out_w", 0, 0, _lib.PA_ERR_INVALID_ARG), ("out_h", 2, 0, _lib.PA_ERR_INVALID_ARG),
                                  ("reserved", 1, 1, _lib.PA_ERR_INVALID_ARG), ("out_w", 1, 151, _lib.PA_ERR_CAPACITY),
                                  ("out_h", 1, 526, _lib.PA_ERR_CAPACITY)):
        bad = good.copy()
        bad[field][i] = value
        assert dc.resize_check_status(bad, bank, out) == want, (field, value)
    assert dc.resize_check_status(np.concatenate([good, good]), bank, out) == _lib.PA_ERR_CAPACITY   # more records than slots
    for n, w, h in ((0, 150, 525), (3, 161, 100), (3, 100, 561), (3, 0, 10)):
        with pytest.raises(ValueError):
            dc.ResizedSpriteBank(None, n, w, h)
    dc.ResizedSpriteBank(None, 1, 160, 560).close()


# ---- the scene twin ----------------------------------------------------------------------------------------------------------------

def _pillow_scene(stage, slots, rec):
    im = Image.fromarray(stage)
    for k in range(int(rec["n_sprites"])):
        s = rec["sprites"][k]
        char = Image.fromarray(slots[int(s["slot"])])
        im.paste(char, (int(s["x"]), int(s["y"])), char)
    return np.asarray(im)


def test_scene_twin_equals_pillow_paste():
    stages, slots, recs = cases.make_stages(), cases.make_slots(), cases.scene_records()
    got = dc.compose_scenes_reference(slots, stages, recs)
    counts = set()
    for r, g in zip(recs, got):
        want = _pillow_scene(stages[int(r["stage"])], slots, r)
        assert g.shape == want.shape and np.array_equal(g, want), r
        counts.add(int(r["n_sprites"]))
        if int(r["n_sprites"]) == 1:
            x, y = int(r["sprites"][0]["x"]), int(r["sprites"][0]["y"])
            h, w = g.shape[:2]
            outside = x <= -128 or y <= -128 or x >= w or y >= h
            assert np.array_equal(g, stages[int(r["stage"])]) == outside, r   # (the slots of one-sprite records are not transparent)
    assert counts == {0, 1, 4}
    per_stage = len(recs) // len(stages)
    for g in range(len(stages)):   # the two orders of the overlapping pair differ
        assert not np.array_equal(got[(g + 1) * per_stage - 2], got[(g + 1) * per_stage - 1])


def test_scene_clamps_and_layout():
    r = cases.scene(9, [(77, 5000, -5000), (-1, 1, 2)])
    r["n_sprites"] = 9
    r["reserved"] = 3
    c = dc.scene_clamp_params(r, 6, 3)
    assert int(c["stage"][0]) == 2 and int(c["n_sprites"][0]) == 4 and not c["reserved"].any()
    assert c["sprites"]["slot"][0].tolist() == [5, 0, 0, 0] and c["sprites"]["x"][0].tolist() == [4096, 1, 0, 0]
    assert c["sprites"]["y"][0].tolist() == [-4096, 2, 0, 0]
    recs = cases.scene_records()
    assert np.array_equal(dc.scene_clamp_params(recs, 6, 3), recs)
    off, total = dc.scene_layout(np.concatenate([cases.scene(1, []), cases.scene(0, []), cases.scene(1, [])]), cases.STAGE_SHAPES)
    a, b = (77 * 131 * 3 + 15) // 16 * 16, 150 * 200 * 3
    assert off.tolist() == [0, a, a + b] and total == 2 * a + b and a != 77 * 131 * 3


def test_scene_record_check_refuses_each_rule():
    """pa_scene_params_check with banks of sizes alone (engine=None): no device."""
    stages = sd.StageBank.from_arrays(None, cases.make_stages())
    slots = sa.AugmentedSpriteBank(None, 6)
    recs = cases.scene_records()
    assert dc.scene_check_params(recs, slots, stages)
    good = cases.scene(1, [(5, -4096, 4096), (0, 3, 4)])
    assert dc.scene_check_params(good, slots, stages)

    def bad(mutate):
        r = good.copy()
        mutate(r)
        return not dc.scene_check_params(r, slots, stages)

    assert bad(lambda r: r["stage"].__setitem__(0, 3)) and bad(lambda r: r["stage"].__setitem__(0, -1))
    assert bad(lambda r: r["n_sprites"].__setitem__(0, 5)) and bad(lambda r: r["n_sprites"].__setitem__(0, -1))
    assert bad(lambda r: r["sprites"]["slot"].__setitem__((0, 1), 6)) and bad(lambda r: r["sprites"]["slot"].__setitem__((0, 0), -1))
    assert bad(lambda r: r["sprites"]["x"].__setitem__((0, 0), -4097)) and bad(lambda r: r["sprites"]["y"].__setitem__((0, 1), 4097))
    assert bad(lambda r: r["sprites"]["x"].__setitem__((0, 2), 1))         # an entry behind n_sprites
    assert bad(lambda r: r["sprites"]["slot"].__setitem__((0, 3), 1))
    assert bad(lambda r: r["reserved"].__setitem__((0, 0), 1)) and bad(lambda r: r["reserved"].__setitem__((0, 1), 1))
    # the sprites are 128 x 128 slots: a bank of renders is refused
    renders = sd.SpriteBank.from_arrays(None, {"c": {"a": {"b": {"r": {"0": [cases.make_render(128, 128, "full")]}}}}})
    assert not dc.scene_check_params(cases.scene(0, []), renders, stages)


# ---- the sampler -------------------------------------------------------------------------------------------------------------------

@pytest.fixture(scope="module")
def banks():
    return sd.SpriteBank.from_arrays(None, cases.sampler_tree()), sd.StageBank.from_arrays(None, cases.make_stages())


def test_sample_is_a_function_of_the_seed(banks):
    sprites, stages = banks
    a = dc.sample_scenes(np.random.default_rng(5), sprites, stages, 12)
    b = dc.sample_scenes(np.random.default_rng(5), sprites, stages, 12)
    c = dc.sample_scenes(np.random.default_rng(6), sprites, stages, 12)
    for x, y in zip(a[:3], b[:3]):
        assert np.array_equal(x, y)
    assert a[3] == b[3] and not np.array_equal(a[2], c[2])
    resize, aug, scenes, labels = a
    m = len(resize)
    assert len(aug) == m == int(scenes["n_sprites"].sum()) == sum(len(r) for r in labels) and len(scenes) == len(labels) == 12
    assert aug["src"].tolist() == list(range(m))
    used = [int(s["slot"]) for r in scenes for s in r["sprites"][:int(r["n_sprites"])]]
    assert used == list(range(m))                                      # record j writes slot j, in scene order
    for j, r in enumerate(resize):
        h, w = sprites.shapes[int(r["src"])]
        assert w >= 100 and h >= 100 and 50 <= r["out_w"] <= 150 and r["out_h"] == int(float(h) * (int(r["out_w"]) / float(w)))
    # the records pass the three host checks
    out = dc.ResizedSpriteBank(None, m, 150, 525)
    assert dc.resize_check_status(resize, sprites, out) == _lib.PA_OK
    assert dc.scene_check_params(scenes, sa.AugmentedSpriteBank(None, m), stages)
    # the augmentation's defaults are augment_synth_char_crop's own, and the dict overrides them
    off = dc.sample_scenes(np.random.default_rng(5), sprites, stages, 12, augment={"horizontal_flip": 0.0, "hard_mode": 0.0, "resize": 0.0})
    assert not off[1]["flip"].any() and not off[1]["new_scale"].any() and not off[1]["pixel_drop_thr"].any()
    assert aug["flip"].any()
    with pytest.raises(ValueError):
        dc.sample_scenes(np.random.default_rng(5), sprites, stages, 1, augment={"nonsense": 1})
    with pytest.raises(ValueError):
        dc.sample_scenes(np.random.default_rng(5), sprites, stages, 1, class_type="ACTION")


def test_sample_quirks_and_label_text(banks):
    """Seed 68, 12 images: both quirks of the reference occur. The float-centre fallback: image 3's second Gaussian x falls
    outside the 131-wide picture and becomes the FLOAT 65.5, so the label reads 0.5 (no integer centre gives that on an odd
    width) and the corner is int(65.5 - 64.0) = 1. The under-100 skip: images 0 and 7 drew only renders below 100 pixels and
    have no sprite and an empty label file."""
    sprites, stages = banks
    resize, aug, scenes, labels = dc.sample_scenes(np.random.default_rng(68), sprites, stages, 12)
    assert stages.shapes[int(scenes["stage"][3])] == (77, 131)
    assert labels[3][1][1] == 0.5 and int(scenes["sprites"][3, 1]["x"]) == int(131 / 2 - 64.0) == 1
    assert dc.label_text(labels[3]) == ("196 0.5114503816793893 0.3246753246753247 0.9770992366412213 1.6623376623376624\n"
                                        "196 0.5 0.4155844155844156 0.9770992366412213 1.6623376623376624\n")
    for i in (0, 7):
        assert labels[i] == [] and int(scenes["n_sprites"][i]) == 0 and dc.label_text(labels[i]) == ""
    assert dc.label_text(labels[8]) == "196 0.665 0.6066666666666667 0.64 0.8533333333333334\n"
    assert scenes["sprites"][8, 0].tolist() == (19, 69, 27)            # int(0.665 * 200) - 64, int(91 - 64)
    # every other centre is a truncated Gaussian draw, an integer inside the picture, and the corner is 64 less
    for i, rows in enumerate(labels):
        H, W = stages.shapes[int(scenes["stage"][i])]
        for k, (c, x, y, w, h) in enumerate(rows):
            if (i, k) == (3, 1):
                continue
            sx, sy = int(scenes["sprites"][i, k]["x"]), int(scenes["sprites"][i, k]["y"])
            assert abs(x * W - (sx + 64)) < 1e-9 and abs(y * H - (sy + 64)) < 1e-9 and 0 <= sx + 64 <= W and 0 <= sy + 64 <= H
            assert (w, h) == (128 / W, 128 / H)
    # no render below 100 pixels is ever resized
    assert all(min(sprites.shapes[int(k)]) >= 100 for k in resize["src"])


def test_class_ids(banks):
    sprites, stages = banks
    assert dc.class_id("Pikachu", "Grabbed") == 63 * 2 + 62 and dc.class_id("Joker", "UpSmash") == 63 * 3 + 7
    assert dc.class_id("Pikachu", "Grabbed", "CHAR") == 2 and dc.class_id("Joker", "UpSmash", "CHAR") == 3
    both = dc.sample_scenes(np.random.default_rng(3), sprites, stages, 10)[3]
    char = dc.sample_scenes(np.random.default_rng(3), sprites, stages, 10, class_type="CHAR")[3]
    ids = [(a[0], b[0]) for ra, rb in zip(both, char) for a, b in zip(ra, rb)]
    assert ids and set(ids) <= {(63 * 2 + 62, 2), (63 * 3 + 7, 3)} and len(set(ids)) == 2
    assert [r[1:] for rows in both for r in rows] == [r[1:] for rows in char for r in rows]
    assert dc.label_text([(194, 0.5, 0.25, 0.64, 128 / 150)]) == "194 0.5 0.25 0.64 0.8533333333333334\n"


def test_a_render_taller_than_the_pad_step_takes_is_refused_by_name(banks):
    _, stages = banks
    tree = cases.sampler_tree()
    tree["Joker"]["UpSmash"]["c00"]["c05attackhi4"]["0"] = [cases.make_render(351, 100, "full")]
    sprites = sd.SpriteBank.from_arrays(None, tree)
    with pytest.raises(ValueError, match=r"Joker_c00_c05attackhi4_0_0\.png \(351 x 100\)"):
        dc.sample_scenes(np.random.default_rng(0), sprites, stages, 1)
    with pytest.raises(NotImplementedError):
        dc.generate_stage_char_compositions("train", 1, "/nonexistent", sprites, stages, bbox_overlay=True)
