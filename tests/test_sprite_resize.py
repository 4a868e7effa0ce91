"""``pa_sprite_resize`` (``csrc/sprite_resize.hip``) against its numpy twin ``detect_composite.resize_sprites_reference``, bit for
bit: every case and alpha plane of the host tests (which pin the twin to the installed Pillow's ``Image.resize``), one record
alone, a mixed batch with repeated sources, records that break every rule of the host check and random bytes, and
``pa_sprite_augment`` reading the resized bank."""
import os
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import detect_composite_cases as cases  # noqa: E402

from playaid_core_amd import detect_composite as dc  # noqa: E402
from playaid_core_amd import sprite_augment as sa  # noqa: E402
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd import synth_dataset as sd  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from playaid_core_amd.engine import Engine

    eng = Engine(synth.make_state_dict(seed=7), max_batch_frames=4, max_clip_frames=16, max_frame_height=128, max_frame_width=128)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def renders():
    return cases.resize_renders()


@pytest.fixture(scope="module")
def bank(engine, renders):
    b = sd.SpriteBank.from_arrays(engine, {"c": {"a": {"b": {"r": {"0": renders[0]}}}}})
    yield b
    b.close()


def _compare(out, want):
    for i, w in enumerate(want):
        got = out.read(i)
        assert got.shape == w.shape, (i, got.shape, w.shape)
        assert np.array_equal(got, w), (i, w.shape, int(np.abs(got.astype(int) - w).max()), int((got != w).sum()))


def test_every_case_bit_for_bit(engine, bank, renders):
    arrays, params = renders
    out = dc.resize_sprites(engine, bank, params)
    assert out.shapes == [(int(h), int(w)) for h, w in zip(params["out_h"], params["out_w"])]
    _compare(out, dc.resize_sprites_reference(arrays, params))
    out.close()


def test_one_record_and_a_mixed_batch_with_repeated_sources(engine, bank, renders):
    arrays, _ = renders
    one = dc.resize_params([17], [50], [14])                           # a 300 x 1024 render through the 83-tap pass
    out = dc.resize_sprites(engine, bank, one)
    _compare(out, dc.resize_sprites_reference(arrays, one))
    src = [12, 12, 2, 27, 12, 2, 44, 7]
    mixed = dc.resize_params(src, [50, 150, 77, 1, 160, 100, 160, 128], [85, 300, 33, 1, 274, 100, 560, 128])
    big = dc.ResizedSpriteBank(engine, 16)
    assert dc.resize_sprites(engine, bank, mixed, out=big) is big
    _compare(big, dc.resize_sprites_reference(arrays, mixed))
    # a second call on the same bank, fewer records: its slots change, the ones behind them stay
    again = dc.resize_params([30, 5], [60, 149], [65, 58])
    dc.resize_sprites(engine, bank, again, out=big)
    _compare(big, dc.resize_sprites_reference(arrays, again) + dc.resize_sprites_reference(arrays, mixed)[2:])
    out.close()
    big.close()


def test_records_the_check_refuses_are_clamped_as_the_twin_clamps(engine, bank, renders):
    arrays, _ = renders
    small = dc.ResizedSpriteBank(engine, 24, 150, 525)
    bad = dc.resize_params([-5, 1000, 3, 8, 2, 40], [50, 60, 0, -7, 151, 4000], [60, 65, 20, 20, 526, -1])
    bad["reserved"] = [0, 0, 0, 5, 0, -1]
    rng = np.random.default_rng(21)
    noise = rng.integers(0, 256, 12 * dc.RESIZE_DTYPE.itemsize, dtype=np.uint8).view(dc.RESIZE_DTYPE)
    noise["out_w"][:6] = rng.integers(-3, 200, 6)                      # ... some of them near the limits
    noise["out_h"][:6] = rng.integers(-3, 700, 6)
    noise["src"][:6] = rng.integers(-2, len(arrays) + 2, 6)
    params = np.concatenate([bad, noise])
    assert dc.resize_check_status(params, bank, small) != 0
    with pytest.raises(ValueError):
        dc.resize_sprites(engine, bank, params, out=small)
    dc.resize_sprites(engine, bank, params, out=small, check=False)
    want = dc.resize_sprites_reference(arrays, params, 150, 525)
    assert all(w.shape[0] <= 525 and w.shape[1] <= 150 for w in want)
    _compare(small, want)
    small.close()


def test_sprite_augment_reads_the_resized_bank(engine, bank, renders):
    import test_sprite_augment_host as sah

    arrays, _ = renders
    src = [2 + 5 * k for k in range(len(cases.RESIZE_CASES))]         # the random-alpha render of every case of the table
    params = dc.resize_params(src, [t[0] for _, t in cases.RESIZE_CASES], [t[1] for _, t in cases.RESIZE_CASES])
    resized = dc.resize_sprites(engine, bank, params)
    twin = dc.resize_sprites_reference(arrays, params)
    n = len(src)
    aug = np.concatenate([sa.identity_params(n), sah._all_stages(1, np.random.default_rng(4), holes=True, drop=True, new_scale=111)])
    aug["src"][n] = 2
    assert sa.check_params(aug, resized)                               # (the host's descriptors are the resized sizes)
    got = sa.augment_sprites(engine, resized, aug).read()
    want = sa.augment_sprites_reference(twin, aug)
    assert np.array_equal(got, want), int((got != want).sum())
    resized.close()
