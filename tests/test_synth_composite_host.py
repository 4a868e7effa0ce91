"""Synthetic training windows (``playaid_core_amd/synth_dataset.py``, ``csrc/synth_composite.hip``), the parts that need no
GPU: the numpy twin against the libraries byte for byte -- ``oracle.resample.cv_resize_area`` for the resample, Pillow's own
``Image.paste`` for the blend --, the host-side argument checks of the C ABI, and the ``get_synth`` sampler. (The GPU tests pin
the kernel to the twin bit for bit.)"""
import ctypes
import os
import re

import numpy as np
import pytest
from PIL import Image

from oracle.resample import cv_resize_area
from playaid_core_amd import _build, _lib
from playaid_core_amd import synth_dataset as sd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# h x w: 128 x 128 copy, 256 x 256 2 x 2 fast, 384 x 384 integer fast, 200 x 150 general with h > w, 300 x 301 general with
# oh = 127, 90 x 60 enlarging, 37 x 128 and 4 x 128 wide copies, 127 x 3 enlarging with one axis at scale exactly 1
SIZES = [(1, 1), (128, 128), (256, 256), (384, 384), (200, 150), (300, 301), (90, 60), (37, 128), (127, 3), (4, 128), (1024, 1000)]
ALPHAS = ["zero", "full", "random", "one", "254"]
OFFSETS = [(0, 0), (-40, 40), (40, -40), (200, 0), (-200, 0)]   # the last two: fully off the canvas
STAGE_SHAPES = [(144, 160), (720, 1280)]                          # (H, W)


@pytest.fixture(scope="module", autouse=True)
def lib():
    _build.build()
    return _lib.load()


@pytest.fixture(scope="module")
def stage_images():
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in STAGE_SHAPES]


def make_sprite(h, w, alpha, seed=0):
    rng = np.random.default_rng([h, w, ALPHAS.index(alpha), seed])
    s = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha != "random":
        s[..., 3] = {"zero": 0, "full": 255, "one": 1, "254": 254}[alpha]
    return s


def grid_records(stage_images, dim, sprite=0):
    """Every paste offset at every stage origin -- (0, 0) and (W - D, H - D) -- of every stage that holds a dim x dim crop."""
    recs = []
    for k, st in enumerate(stage_images):
        H, W = st.shape[:2]
        if H < dim or W < dim:
            continue
        for x, y in ((0, 0), (W - dim, H - dim)):
            recs += [(sprite, k, x, y, dx, dy, (0, 0)) for dx, dy in OFFSETS]
    return np.array(recs, dtype=sd.PARAMS_DTYPE)


def by_the_libraries(sprite, stage_images, recs, dim):
    """The reference's own steps with the libraries it calls: the (ow, oh) rule of imutils.resize, the oracle's INTER_AREA,
    Pillow's paste through the sprite's alpha."""
    h, w = sprite.shape[:2]
    ow, oh = (int(w * (dim / float(h))), dim) if h > w else (dim, int(h * (dim / float(w))))
    char = Image.fromarray(cv_resize_area(sprite, ow, oh))
    assert char.mode == "RGBA" and char.size == (ow, oh)
    out = []
    for r in recs:
        x, y = int(r["stage_x"]), int(r["stage_y"])
        crop = Image.fromarray(np.ascontiguousarray(stage_images[int(r["stage"])][y:y + dim, x:x + dim]))
        px, py = int((crop.width - char.width) / 2) + int(r["paste_dx"]), int((crop.height - char.height) / 2) + int(r["paste_dy"])
        crop.paste(char, (px, py), char)
        out.append(np.array(crop))
    return np.stack(out), (ow, oh)


def assert_same(got, want, what):
    assert got.dtype == want.dtype and got.shape == want.shape, what
    if not np.array_equal(got, want):
        bad = np.argwhere(got != want)
        raise AssertionError(f"{what}: {len(bad)} values differ, first at {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")


@pytest.mark.parametrize("hw", SIZES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_twin_equals_the_libraries_at_128(stage_images, hw):
    for alpha in ALPHAS:
        sprite = make_sprite(*hw, alpha)
        recs = grid_records(stage_images, 128)
        want, (ow, oh) = by_the_libraries(sprite, stage_images, recs, 128)
        got = sd.composite_reference([sprite], stage_images, recs, 128, "uint8")
        assert_same(got, want, f"{hw} alpha {alpha}")
        assert sd.sprite_size(*hw, 128) == (ow, oh)
        # the off-canvas offsets and a zero alpha leave the stage crop; everything else changes it
        crop0 = stage_images[0][:128, :128]
        assert np.array_equal(got[3], crop0) and np.array_equal(got[4], crop0)
        assert np.array_equal(got[0], crop0) == (alpha == "zero")
    model = sd.composite_reference([sprite], stage_images, recs[:2], 128, "model")
    assert model.dtype == np.float32 and model.shape == (2, 3, 128, 128)
    assert np.array_equal(model, got[:2].transpose(0, 3, 1, 2).astype(np.float32) / np.float32(255))


def test_the_sizes_take_the_branches_they_are_named_for():
    want = {(128, 128): (128, 128), (256, 256): (128, 128), (384, 384): (128, 128), (200, 150): (96, 128), (300, 301): (128, 127),
            (90, 60): (85, 128), (37, 128): (128, 37), (127, 3): (3, 128), (4, 128): (128, 4), (1, 1): (128, 128)}
    for hw, size in want.items():
        assert sd.sprite_size(*hw, 128) == size, hw


@pytest.mark.parametrize("dim", [32, 96, 256])
def test_twin_equals_the_libraries_at_other_sizes(stage_images, dim):
    stage_images = [s for s in stage_images if min(s.shape[:2]) >= dim]   # (a bank with a stage smaller than dim is refused whole)
    for hw in [(1, 1), (128, 128), (256, 256), (200, 150), (300, 301), (90, 60), (127, 3), (1024, 1000)]:
        if hw == (127, 3) and dim == 32:   # ow = int(3 * (32 / 127.0)) = 0: cv2.resize raises, and so does everything here
            with pytest.raises(ValueError):
                sd.composite_reference([make_sprite(*hw, "random")], stage_images, grid_records(stage_images, dim), dim)
            continue
        for alpha in ("random", "254"):
            sprite = make_sprite(*hw, alpha, seed=dim)
            recs = grid_records(stage_images, dim)
            assert len(recs) == (10 if dim == 256 else 20)
            want, _ = by_the_libraries(sprite, stage_images, recs, dim)
            assert_same(sd.composite_reference([sprite], stage_images, recs, dim, "uint8"), want, f"dim {dim} {hw} alpha {alpha}")


# ---- the C ABI's host side -------------------------------------------------------------------------------------------------------

def test_symbols_and_record_layout(lib):
    hdr = open(os.path.join(ROOT, "include", "playaid_hip.h")).read()
    names = [n for n, _, _ in _lib.SYMBOLS]
    for name in ("pa_synth_bank_create", "pa_synth_bank_destroy", "pa_synth_params_check", "pa_synth_composite"):
        assert hasattr(lib, name) and name in names and re.search(rf"\b{name}\(", hdr), name
    body = re.search(r"typedef struct pa_synth_params \{(.*?)\} pa_synth_params;", hdr, re.S).group(1)
    fields = []
    for decl in re.findall(r"int32_t\s+([^;]+);", body):
        for name in decl.split(","):
            m = re.match(r"\s*(\w+)(?:\[(\d+)\])?\s*$", name)
            fields.append((m.group(1), int(m.group(2) or 1)))
    assert fields == [("sprite", 1), ("stage", 1), ("stage_x", 1), ("stage_y", 1), ("paste_dx", 1), ("paste_dy", 1), ("reserved", 2)]
    assert ctypes.sizeof(_lib.pa_synth_params) == 32 == sd.PARAMS_DTYPE.itemsize
    off = 0
    for name, count in fields:
        assert getattr(_lib.pa_synth_params, name).offset == off == sd.PARAMS_DTYPE.fields[name][1], name
        off += 4 * count
    for name in ("PA_SYNTH_SPRITES", "PA_SYNTH_STAGES", "PA_SYNTH_U8", "PA_SYNTH_MODEL", "PA_SYNTH_DIM_MIN", "PA_SYNTH_DIM_MAX",
                 "PA_SYNTH_SPRITE_MAX", "PA_SYNTH_STAGE_MAX", "PA_SYNTH_PASTE_MAX"):
        assert int(re.search(rf"#define {name} (\d+)", hdr).group(1)) == getattr(_lib, name), name
    assert int(re.search(r"#define PA_ABI_VERSION (\d+)", hdr).group(1)) == 15 == _lib.PA_ABI_VERSION


def _bank_rc(lib, kind, shapes, n=None, null_image=False):
    ch = 4 if kind == _lib.PA_SYNTH_SPRITES else 3
    arrays = [np.zeros((h, w, ch), dtype=np.uint8) if h > 0 and w > 0 else np.zeros((1, 1, ch), dtype=np.uint8) for h, w in shapes]
    k = max(len(shapes), 1)
    ptrs = (ctypes.c_void_p * k)(*[None if null_image else a.ctypes.data for a in arrays])
    widths = (ctypes.c_int32 * k)(*[w for _, w in shapes])
    heights = (ctypes.c_int32 * k)(*[h for h, _ in shapes])
    h = ctypes.c_void_p()
    rc = lib.pa_synth_bank_create(None, kind, ptrs, widths, heights, len(shapes) if n is None else n, ctypes.byref(h))
    if rc == _lib.PA_OK:
        assert h.value
        lib.pa_synth_bank_destroy(h)
    else:
        assert not h.value
    return rc


def test_bank_create_refuses_on_the_host(lib):
    """Every refusal comes back with no engine and no device in the process: before any device call."""
    S, G, BAD = _lib.PA_SYNTH_SPRITES, _lib.PA_SYNTH_STAGES, _lib.PA_ERR_INVALID_ARG
    assert _bank_rc(lib, S, [(1, 1), (1024, 1024), (1024, 32), (32, 1024), (1, 32), (127, 3), (1024, 4), (1, 256)]) == _lib.PA_OK
    assert _bank_rc(lib, G, [(1, 1), (4096, 3), (720, 1280)]) == _lib.PA_OK
    assert _bank_rc(lib, S, [(5, 5)], n=0) == BAD and _bank_rc(lib, S, [(5, 5)], n=-1) == BAD
    assert _bank_rc(lib, 2, [(5, 5)]) == BAD and _bank_rc(lib, -1, [(5, 5)]) == BAD
    assert _bank_rc(lib, S, [(5, 5)], null_image=True) == BAD
    for bad in [(0, 5), (5, 0), (-1, 5), (1025, 1024), (1024, 1025), (1024, 3), (3, 1024), (1, 257), (514, 2)]:   # the last four: empty at every dim
        assert _bank_rc(lib, S, [(8, 8), bad]) == BAD, bad
    for bad in [(0, 5), (5, 0), (4097, 8), (8, 4097)]:
        assert _bank_rc(lib, G, [(8, 8), bad]) == BAD, bad
    assert lib.pa_synth_bank_create(None, S, None, None, None, 1, None) == BAD
    with pytest.raises(ValueError):
        sd.StageBank.from_arrays(None, [np.zeros((5000, 8, 3), np.uint8)])
    with pytest.raises(ValueError):
        sd.SpriteBank.from_arrays(None, {"a": {"A": {"c00": {"r": {"90": [np.zeros((8, 8, 3), np.uint8)]}}}}})   # RGB, not RGBA


# ---- the sampler -----------------------------------------------------------------------------------------------------------------

ANIMS = ["Jab", "Dash", "Unknown"]


def make_tree(seed=3):
    """Two characters, three actions in the list and two outside it, one body, one raw animation, two cameras of 5..9 frames;
    the sprites are 1 x 1 (the sampler reads no pixel). Every list of frames has its own length where possible."""
    rng = np.random.default_rng(seed)
    tree = {}
    for char in ("mario", "link"):
        tree[char] = {}
        for action in ("Jab", "Dash", "Grab", "Taunt"):
            tree[char][action] = {"c00": {f"{action.lower()}_raw": {cam: [np.zeros((1, 1, 4), np.uint8)] * int(rng.integers(5, 10))
                                                                    for cam in ("90", "-90")}}}
    return tree


@pytest.fixture(scope="module")
def banks():
    sprites = sd.SpriteBank.from_arrays(None, make_tree())
    stages = sd.StageBank.from_arrays(None, [np.zeros((140, 136, 3), np.uint8), np.zeros((129, 300, 3), np.uint8)])
    yield sprites, stages
    sprites.close()
    stages.close()


def draw(banks, seed, **kw):
    sprites, stages = banks
    args = dict(num_frames_per_sample=7, dim=128, randomize_stage_background=False, move_stage_background=False, paste_jitter=0)
    args.update(kw)
    return sd.sample_synth(np.random.default_rng(seed), sprites.tree, ANIMS, ["mario", "link"], stage_sizes=stages.shapes, **args)


def test_dataset_draw_is_a_function_of_seed_epoch_and_index(banks):
    sprites, stages = banks
    a = sd.SynthWindowDataset(None, sprites, stages, animations=ANIMS, num_samples=6, seed=5, paste_jitter=3)
    b = sd.SynthWindowDataset(None, sprites, stages, animations=ANIMS, num_samples=6, seed=5, paste_jitter=3)
    assert len(a) == 6
    first = [a.sample(i) for i in range(6)]
    for i in (5, 0, 3):   # any order, either object
        got = b.sample(i)
        assert np.array_equal(got[0], first[i][0]) and got[1:3] == first[i][1:3]
    assert any(not np.array_equal(first[0][0], first[i][0]) for i in range(1, 6))
    b.set_epoch(1)
    assert any(not np.array_equal(b.sample(i)[0], first[i][0]) for i in range(6))
    b.set_epoch(0)
    assert np.array_equal(b.sample(2)[0], first[2][0])
    c = sd.SynthWindowDataset(None, sprites, stages, animations=ANIMS, num_samples=6, seed=6, paste_jitter=3)
    assert any(not np.array_equal(c.sample(i)[0], first[i][0]) for i in range(6))
    with pytest.raises(IndexError):
        a.sample(6)


def test_window_lies_in_the_timeline_and_labels_follow_the_frames(banks):
    sprites, _ = banks
    crossed = unknown = 0
    for seed in range(300):
        params, char_label, actions, meta = draw(banks, seed)
        S = 7
        assert len(params) == len(actions) == S and meta["char"] == ["mario", "link"][char_label]
        assert len(meta["segments"]) >= 2 and len(meta["timeline"]) == sum(s[4] for s in meta["segments"]) >= S
        last = meta["last_frame"]
        assert S <= last <= len(meta["timeline"]) - 1
        assert list(params["sprite"]) == meta["timeline"][last - S:last]
        # frame by frame: the record's sprite belongs to the segment whose drawn action labels it
        owner, segment_of = [], []
        for k, (drawn, used, raw, cam, n) in enumerate(meta["segments"]):
            frames = sprites.tree[meta["char"]][used][meta["body"]][raw][cam]
            assert len(frames) == n
            owner += [(drawn, f) for f in frames]
            segment_of += [k] * n
            if drawn == "Unknown":
                assert used in ("Grab", "Taunt")   # the character's actions outside the list
                unknown += 1
            else:
                assert used == drawn
        assert [(a, int(k)) for a, k in zip(actions, params["sprite"])] == owner[last - S:last]
        crossed += len(set(segment_of[last - S:last])) > 1
    assert crossed > 20 and unknown > 50   # windows across an animation boundary, and "Unknown" passes, both occur


def test_origin_move_and_jitter_ranges_are_exact(banks):
    _, stages = banks
    xs, ys, moves, jit = set(), set(), set(), set()
    for seed in range(400):
        p = draw(banks, seed)[0]
        assert len(set(p["stage"])) == 1 and len(set(p["stage_x"])) == 1 and (p["paste_dx"] == 0).all() and (p["reserved"] == 0).all()
        h, w = stages.shapes[int(p["stage"][0])]
        assert 0 <= p["stage_x"][0] < w - 128 and 0 <= p["stage_y"][0] < h - 128   # randrange: upper bound exclusive
        if (h, w) == (129, 300):
            assert p["stage_y"][0] == 0
        if (h, w) == (140, 136):
            xs.add(int(p["stage_x"][0]))
            ys.add(int(p["stage_y"][0]))
        m = draw(banks, seed, move_stage_background=True)[0]
        h, w = stages.shapes[int(m["stage"][0])]
        x, y = np.asarray(m["stage_x"], np.int64), np.asarray(m["stage_y"], np.int64)
        assert (x >= 0).all() and (x <= w - 128).all() and (y >= 0).all() and (y <= h - 128).all()   # the clamp is inclusive
        inner = (x[1:] > 0) & (x[1:] < w - 128) & (x[:-1] > 0) & (x[:-1] < w - 128)
        moves.update((x[1:] - x[:-1])[inner].tolist())
        j = draw(banks, seed, paste_jitter=40)[0]
        jit.update(j["paste_dx"].tolist())
        jit.update(j["paste_dy"].tolist())
        r = draw(banks, seed, randomize_stage_background=True, move_stage_background=True)[0]
        for rec in r:
            hh, ww = stages.shapes[int(rec["stage"])]
            assert 0 <= rec["stage_x"] < ww - 128 and 0 <= rec["stage_y"] < hh - 128
    assert xs == set(range(0, 8)) and ys == set(range(0, 12))
    assert moves == set(range(-10, 10))
    assert jit == set(range(-40, 41))


def test_sampler_raises_the_references_exceptions(banks):
    sprites, stages = banks
    base = dict(animations=["Jab"], characters=["mario"], num_frames_per_sample=7, dim=128, stage_sizes=stages.shapes)
    rng = lambda: np.random.default_rng(0)
    frames = [0] * 8
    with pytest.raises(Exception, match="Requested action Jab for mario has no associated body"):
        sd.sample_synth(rng(), {"mario": {"Jab": {}}}, **base)
    with pytest.raises(Exception, match="Requested action Jab for mario and body c00 has no raw anim"):
        sd.sample_synth(rng(), {"mario": {"Jab": {"c00": {}}}}, **base)
    with pytest.raises(Exception, match="Requested raw action r for mario and body c00 has no cam"):
        sd.sample_synth(rng(), {"mario": {"Jab": {"c00": {"r": {}}}}}, **base)
    with pytest.raises(Exception, match="Requested cam for mario c00 r 90 has no anim"):
        sd.sample_synth(rng(), {"mario": {"Jab": {"c00": {"r": {"90": []}}}}}, **base)
    good = {"mario": {"Jab": {"c00": {"r": {"90": frames}}}}}
    assert len(sd.sample_synth(rng(), good, **base)[0]) == 7
    for shape in ((128, 128), (128, 300), (300, 128), (100, 300)):   # a stage must be strictly larger than D: randrange(0, 0)
        with pytest.raises(ValueError):
            sd.sample_synth(rng(), good, **dict(base, stage_sizes=[shape]))
    with pytest.raises(IndexError):   # "Unknown" with nothing outside the list: random.choice of an empty list
        for seed in range(40):   # (one of two draws per pass is "Unknown")
            sd.sample_synth(np.random.default_rng(seed), good, **dict(base, animations=["Jab", "Unknown"]))
    # a listed action the character lacks: the stand-in draw raises the reference's KeyError when it hits it; when it does not,
    # the loop draws again each time it comes up ("keep trying") and the window never carries it
    kept = 0
    for seed in range(40):
        try:
            actions = sd.sample_synth(np.random.default_rng(seed), good, **dict(base, animations=["Jab", "Shield"]))[2]
        except KeyError as exc:
            assert exc.args == ("Shield",)
            continue
        assert actions == ["Jab"] * 7
        kept += 1
    assert 5 < kept < 35
    with pytest.raises(NotImplementedError, match="augment_synth_char_crop"):
        sd.SynthWindowDataset(None, sprites, stages, animations=ANIMS, num_samples=1, synth_difficulty=1)


def test_banks_from_directories(tmp_path):
    """The layout ``get_character_actions_animations_dict`` walks: frames sorted by their NUMBER (10 after 9), odd animation
    names kept whole, stray files skipped; stages are every ``**/*.jpg``."""
    rng = np.random.default_rng(8)
    chars = tmp_path / "chars"
    names = {"byleth": {"Jab": ["byleth_c00_c03attack11_frame_90_10", "byleth_c00_c03attack11_frame_90_9", "byleth_c00_c03attack11_frame_-90_2",
                                "byleth_c01_j02win1+us_en_frame_-90_63"],
                        "Dash": ["byleth_c00_c02dash_frame_90_0"]}}
    pixels = {}
    for char, moves in names.items():
        for move, stems in moves.items():
            (chars / char / move).mkdir(parents=True)
            for k, stem in enumerate(stems):
                pixels[stem] = rng.integers(0, 256, (5 + k, 7, 4), dtype=np.uint8)
                Image.fromarray(pixels[stem]).save(chars / char / move / f"{stem}.png")
    (chars / "notes.txt").write_text("not a character")
    (chars / "byleth" / "readme.txt").write_text("not a move")
    bank = sd.SpriteBank.from_directory(None, str(chars))
    assert list(bank.tree) == ["byleth"] and sorted(bank.tree["byleth"]) == ["Dash", "Jab"]
    jab = bank.tree["byleth"]["Jab"]
    assert sorted(jab) == ["c00", "c01"] and list(jab["c01"]) == ["j02win1+us_en_frame"] and sorted(jab["c00"]["c03attack11_frame"]) == ["-90", "90"]
    nine, ten = jab["c00"]["c03attack11_frame"]["90"]   # (the reference keeps "_frame" in the name)
    assert bank.paths[nine].endswith("_90_9.png") and bank.paths[ten].endswith("_90_10.png")
    assert len(bank) == 5 and bank.shapes[nine] == (6, 7) and bank.shapes[ten] == (5, 7)
    assert sd.frame_number(bank.paths[jab["c01"]["j02win1+us_en_frame"]["-90"][0]]) == 63
    bank.close()
    stages = tmp_path / "stages"
    (stages / "battlefield").mkdir(parents=True)
    Image.fromarray(rng.integers(0, 256, (150, 140, 3), dtype=np.uint8)).save(stages / "battlefield" / "b.jpg")
    Image.fromarray(rng.integers(0, 256, (130, 200, 3), dtype=np.uint8)).save(stages / "a.jpg")
    Image.fromarray(rng.integers(0, 256, (9, 9, 3), dtype=np.uint8)).save(stages / "skipped.png")
    sb = sd.StageBank.from_directory(None, str(stages))
    assert [p[len(str(stages)) + 1:] for p in sb.paths] == ["a.jpg", "battlefield/b.jpg"] and sb.shapes == [(130, 200), (150, 140)]
    sb.close()


# ---- the host check --------------------------------------------------------------------------------------------------------------

def test_check_accepts_the_sampler_and_refuses_each_bad_field(banks):
    sprites, stages = banks
    for seed in range(60):
        for kw in ({}, {"move_stage_background": True}, {"randomize_stage_background": True, "paste_jitter": 40}):
            assert sd.check_params(draw(banks, seed, **kw)[0], sprites, stages, 128)
    good = np.zeros(3, dtype=sd.PARAMS_DTYPE)
    good[1] = (len(sprites) - 1, 1, 300 - 128, 129 - 128, 4096, -4096, (0, 0))   # every field at its limit
    good[2] = (3, 0, 136 - 128, 140 - 128, -4096, 4096, (0, 0))
    assert sd.check_params(good, sprites, stages, 128)
    assert np.array_equal(sd.clamp_params(good, sprites.shapes, stages.shapes, 128), good)

    def refused(field, value, at=1):
        p = good.copy()
        p[field][at] = value
        clamped = sd.clamp_params(p, sprites.shapes, stages.shapes, 128)
        assert not np.array_equal(clamped, p) and sd.check_params(clamped, sprites, stages, 128), field
        return not sd.check_params(p, sprites, stages, 128)

    assert refused("sprite", len(sprites)) and refused("sprite", -1) and refused("sprite", 2 ** 31 - 1)
    assert refused("stage", 2) and refused("stage", -1) and refused("stage", -2 ** 31)
    assert refused("stage_x", 300 - 128 + 1) and refused("stage_x", -1) and refused("stage_y", 2) and refused("stage_y", -1)
    assert refused("paste_dx", 4097) and refused("paste_dx", -4097) and refused("paste_dy", 4097) and refused("paste_dy", -2 ** 31)
    assert refused("reserved", (1, 0)) and refused("reserved", (0, -1))
    # a sprite too thin for dim (127 x 3 gives ow = 0 below dim 43), a stage smaller than dim, and a dim outside 32..256
    thin = sd.SpriteBank.from_arrays(None, {"a": {"A": {"c00": {"r": {"90": [np.zeros((127, 3, 4), np.uint8), np.zeros((9, 9, 4), np.uint8)]}}}}})
    big = sd.StageBank.from_arrays(None, [np.zeros((300, 300, 3), np.uint8)])
    assert sd.sprite_size(127, 3, 42)[0] == 0 and sd.sprite_size(127, 3, 43)[0] == 1
    assert sd.check_params(good[:1], thin, big, 43) and not sd.check_params(good[:1], thin, big, 42)
    assert sd.check_params(good[:1], sprites, stages, 129) and not sd.check_params(good[:1], sprites, stages, 137)
    assert not sd.check_params(good[1:2], sprites, stages, 130)
    assert not sd.check_params(good[:1], sprites, stages, 31) and not sd.check_params(good[:1], sprites, stages, 257)
    assert not sd.check_params(good, stages, stages, 128) and not sd.check_params(good, sprites, sprites, 128)   # the wrong kind
    with pytest.raises(ValueError):
        sd.check_params(np.zeros(0, dtype=sd.PARAMS_DTYPE), sprites, stages, 128)
