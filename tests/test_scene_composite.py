"""``pa_scene_composite`` (``csrc/scene_composite.hip``) against its numpy twin ``detect_composite.compose_scenes_reference``, bit
for bit: every stage and sprite position of the host tests (which pin the twin to Pillow's own ``Image.paste``), one record
alone, a mixed batch, one 1280 x 720 stage with four sprites, records that break every rule of the host check and random
bytes, and a buffer too small for the batch."""
import ctypes as C
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

BIG = 3   # the 1280 x 720 stage's number in the bank


@pytest.fixture(scope="module")
def engine():
    from playaid_core_amd.engine import Engine

    eng = Engine(synth.make_state_dict(seed=7), max_batch_frames=4, max_clip_frames=16, max_frame_height=128, max_frame_width=128)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def stage_arrays():
    return cases.make_stages(cases.STAGE_SHAPES + [(720, 1280)])


@pytest.fixture(scope="module")
def stages(engine, stage_arrays):
    b = sd.StageBank.from_arrays(engine, stage_arrays)
    yield b
    b.close()


@pytest.fixture(scope="module")
def slots(engine):
    """Six 128 x 128 sprites in a bank of slots (identity records of pa_sprite_augment put them there), and what the bank holds."""
    arrays = cases.make_slots()
    src = sd.SpriteBank.from_arrays(engine, {"c": {"a": {"b": {"r": {"0": list(arrays)}}}}})
    bank = sa.augment_sprites(engine, src, sa.identity_params(len(arrays)))
    held = bank.read()
    assert np.array_equal(held[..., 3], arrays[..., 3])   # the alpha planes of the cases: zero, full, random, 1, 254, random
    yield bank, held
    bank.close()
    src.close()


def _compare(engine, slots, stages, stage_arrays, recs, check=True):
    bank, held = slots
    images, desc = dc.compose_scenes(engine, bank, stages, recs, check=check)
    got = dc.unpack_scenes(images, recs, stages.shapes)
    want = dc.compose_scenes_reference(held, stage_arrays, recs)
    offsets, total = dc.scene_layout(recs, stages.shapes)
    d = desc.cpu().numpy()
    assert d[:, 0].tolist() == offsets.tolist() and images.numel() == total
    assert d[:, 1].tolist() == [(w.shape[1] << 32) | w.shape[0] for w in want]
    for i, (g, w) in enumerate(zip(got, want)):
        assert g.shape == w.shape and np.array_equal(g, w), (i, recs[i], int((g != w).sum()))
    return want


def test_every_stage_and_position_bit_for_bit(engine, slots, stages, stage_arrays):
    _compare(engine, slots, stages, stage_arrays, cases.scene_records())


def test_one_record_and_a_mixed_batch(engine, slots, stages, stage_arrays):
    recs = cases.scene_records()
    _compare(engine, slots, stages, stage_arrays, recs[-1:])
    order = np.random.default_rng(2).permutation(len(recs))[:20]       # stages of three sizes in one call, slots repeated
    _compare(engine, slots, stages, stage_arrays, recs[order])


def test_a_1280_x_720_stage_with_four_sprites(engine, slots, stages, stage_arrays):
    rec = cases.scene(BIG, [(2, 576, 296), (5, 640, 350), (1, -30, 650), (4, 1200, -64)])
    want = _compare(engine, slots, stages, stage_arrays, rec)
    assert not np.array_equal(want[0], stage_arrays[BIG])
    # ... and beside small stages: the launch is sized by the bank's largest picture
    _compare(engine, slots, stages, stage_arrays, np.concatenate([cases.scene(1, [(2, 0, 0)]), rec, cases.scene(2, [(5, -5, -5)])]))


def test_records_the_check_refuses_are_clamped_as_the_twin_clamps(engine, slots, stages, stage_arrays):
    bank, _ = slots
    bad = np.concatenate([cases.scene(7, [(2, 10, 10)]), cases.scene(-1, [(2, 10, 10)]), cases.scene(1, [(6, 0, 0), (-1, 20, 20)]),
                          cases.scene(0, [(2, 5000, 10)]), cases.scene(0, [(2, 10, -5000)]), cases.scene(2, [(1, 1, 1)] * 4),
                          cases.scene(1, [(5, 3, 3)]), cases.scene(2, [(2, 9, 9)])])
    bad["n_sprites"][5] = 9
    bad["n_sprites"][6] = -2
    bad["sprites"]["x"][7, 3] = 50                                     # an entry behind n_sprites: not read
    bad["reserved"][7] = (1, -1)
    for i in range(len(bad)):
        assert not dc.scene_check_params(bad[i:i + 1], bank, stages), i
    with pytest.raises(ValueError):
        dc.compose_scenes(engine, bank, stages, bad)
    _compare(engine, slots, stages, stage_arrays, bad, check=False)
    rng = np.random.default_rng(33)
    noise = rng.integers(0, 256, 16 * dc.SCENE_DTYPE.itemsize, dtype=np.uint8).view(dc.SCENE_DTYPE)
    noise["stage"][:12] = rng.integers(-1, 4, 12)                      # ... most of them near the limits
    noise["n_sprites"][:12] = rng.integers(-2, 7, 12)
    noise["sprites"]["slot"][:12] = rng.integers(-3, 9, (12, 4))
    noise["sprites"]["x"][:12] = rng.integers(-200, 300, (12, 4))
    noise["sprites"]["y"][:12] = rng.integers(-200, 300, (12, 4))
    _compare(engine, slots, stages, stage_arrays, noise, check=False)


def test_a_buffer_too_small_leaves_the_scenes_behind_it_empty(engine, slots, stages, stage_arrays):
    import torch

    bank, held = slots
    recs = np.concatenate([cases.scene(0, [(2, 10, 10)]), cases.scene(1, [(5, 0, 0)]), cases.scene(2, [])])
    offsets, total = dc.scene_layout(recs, stages.shapes)
    images = torch.full((total,), 0xAB, dtype=torch.uint8, device=engine.device)
    desc = torch.zeros((3, 2), dtype=torch.int64, device=engine.device)
    pd = torch.from_numpy(recs.view(np.uint8).reshape(3, dc.SCENE_DTYPE.itemsize)).to(engine.device)
    cap = int(offsets[2]) - 16                                         # the second scene's last 16 bytes do not fit
    engine._check(engine._lib.pa_scene_composite(engine._h, bank._h, stages._h, C.c_void_p(pd.data_ptr()), 3, C.c_void_p(images.data_ptr()),
                                                 cap, C.c_void_p(desc.data_ptr()), engine._stream()))
    d, buf = desc.cpu().numpy(), images.cpu().numpy()
    assert d[:, 0].tolist() == offsets.tolist() and d[:, 1].tolist() == [(200 << 32) | 150, 0, 0]
    want = dc.compose_scenes_reference(held, stage_arrays, recs[:1])[0]
    assert np.array_equal(buf[:150 * 200 * 3].reshape(150, 200, 3), want) and (buf[int(offsets[1]):] == 0xAB).all()
    # bad arguments are refused on the host
    for n, img in ((0, images.data_ptr()), (3, images.data_ptr() + 4), (70000, images.data_ptr())):
        assert engine._lib.pa_scene_composite(engine._h, bank._h, stages._h, C.c_void_p(pd.data_ptr()), n, C.c_void_p(img), total,
                                              C.c_void_p(desc.data_ptr()), engine._stream()) == -1
    assert engine._lib.pa_scene_composite(engine._h, stages._h, stages._h, C.c_void_p(pd.data_ptr()), 3, C.c_void_p(images.data_ptr()), total,
                                          C.c_void_p(desc.data_ptr()), engine._stream()) == -1   # sprites must be a bank of slots
