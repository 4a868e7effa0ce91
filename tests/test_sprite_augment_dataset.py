"""``SynthWindowDataset(sprite_augment=2)`` on the device against the numpy twins on the host: items, batches, and one training
step of ``CNNActionDetector`` from a device batch. The bank and the model are ``tests/test_synth_dataset.py``'s: S = 3, A = 5,
two characters, three actions, 5 to 9 frames each of 40..200 px sprites, two 200 x 160 stages."""
import numpy as np
import pytest
import torch

from playaid_core_amd import sprite_augment as sa
from playaid_core_amd import synth
from playaid_core_amd import synth_dataset as sd

pytestmark = pytest.mark.gpu

S, A = 3, 5
ACTIONS = ["Jab", "Dash", "Unknown", "Shield", "Roll"]
ANIMS = ACTIONS[:3]


def _model(state):
    from playaid_core_amd.cnn_action_detector import CNNActionDetector

    return CNNActionDetector(ACTIONS, sequence_length=S, state_dict=state, max_batch_frames=16, max_clip_frames=64, max_frame_height=96,
                             max_frame_width=128, freeze_encoder=True, learning_rate=1e-3)


@pytest.fixture(scope="module")
def state():
    return synth.make_state_dict(seed=21, num_actions=A, sequence_length=S)


@pytest.fixture(scope="module")
def model(state):
    return _model(state)


@pytest.fixture(scope="module")
def world(model):
    rng = np.random.default_rng(77)
    tree = {}
    for char in ("mario", "link"):
        tree[char] = {}
        for action in ("Jab", "Dash", "Grab"):
            frames = []
            for _ in range(int(rng.integers(5, 10))):
                h, w = (int(v) for v in rng.integers(40, 201, 2))
                s = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
                yy, xx = np.mgrid[0:h, 0:w]
                inside = ((yy - h / 2) / (h / 2)) ** 2 + ((xx - w / 2) / (w / 2)) ** 2
                s[..., 3] = np.clip((1.2 - inside) * 400, 0, 255).astype(np.uint8)
                frames.append(s)
            tree[char][action] = {"c00": {f"{action.lower()}_raw": {"90": frames}}}
    stage_arrays = [rng.integers(0, 256, (160, 200, 3), dtype=np.uint8) for _ in range(2)]
    sprites = sd.SpriteBank.from_arrays(model._engine, tree)
    stages = sd.StageBank.from_arrays(model._engine, stage_arrays)
    sprite_arrays = [f for char in tree.values() for a in char.values() for f in a["c00"][next(iter(a["c00"]))]["90"]]
    yield sprites, stages, sprite_arrays, stage_arrays
    sprites.close()
    stages.close()


def _dataset(model, world, **kw):
    sprites, stages = world[:2]
    args = dict(animations=ANIMS, num_samples=6, num_frames_per_sample=S, move_stage_background=True, paste_jitter=40, seed=4, sprite_augment=2)
    args.update(kw)
    return sd.SynthWindowDataset(model._engine, sprites, stages, **args)


_TWINS = {}


def _twin_item(ds, world, idx):
    """Item ``idx`` built on the host: the same draws, the two twins' frames, the reference's conversions. (Computed once per
    (seed, epoch, idx): the tests share it.)"""
    key = (ds.seed, ds.epoch, idx)
    if key not in _TWINS:
        _, _, sprite_arrays, stage_arrays = world
        params, char_label, actions, _ = ds.sample(idx)
        aug = ds.sample_sprite_augment(idx)
        sprites = list(sa.augment_sprites_reference(sprite_arrays, aug))
        pasted = params.copy()
        pasted["sprite"] = np.arange(S)
        frames = sd.composite_reference(sprites, stage_arrays, pasted, 128, "uint8")
        _TWINS[key] = (torch.tensor(frames).permute(0, 3, 1, 2).float() / 255.0, torch.tensor(char_label),
                       torch.tensor([ANIMS.index(a) for a in actions]), frames, params, actions)
    return _TWINS[key]


def test_items_and_batches_equal_the_twins_and_are_pure(model, world):
    ds = _dataset(model, world)
    sprites = world[0]
    items = [ds[i] for i in range(6)]
    for i, (x, char, anim, meta) in enumerate(items):
        wx, wchar, wanim, frames, params, actions = _twin_item(ds, world, i)
        assert x.dtype == torch.float32 and tuple(x.shape) == (S, 3, 128, 128) and torch.equal(x, wx)
        assert torch.equal(char, wchar) and torch.equal(anim, wanim)
        assert all(np.array_equal(f, w) for f, w in zip(meta["frames"], frames))
        assert meta["frame_paths"] == [sprites.paths[int(k)] for k in params["sprite"]] and meta["actions"] == actions
    got = list(ds.batches(3))
    assert len(got) == 2
    for b, (x, char, anim, metas) in enumerate(got):
        part = items[3 * b:3 * b + 3]
        assert x.is_cuda and x.is_contiguous() and tuple(x.shape) == (3, S, 3, 128, 128)
        assert torch.equal(x.cpu(), torch.stack([it[0] for it in part]))
        assert torch.equal(char.cpu(), torch.stack([it[1] for it in part])) and torch.equal(anim.cpu(), torch.stack([it[2] for it in part]))
    # pure in (seed, epoch, idx): in any order, and after another epoch
    assert torch.equal(ds[4][0], items[4][0]) and torch.equal(ds[0][0], items[0][0])
    ds.set_epoch(1)
    assert not torch.equal(ds[0][0], items[0][0])
    ds.set_epoch(0)
    assert torch.equal(ds[0][0], items[0][0])
    # against sprite_augment=None on the same seed: other pixels, the same labels and stage draws
    plain = _dataset(model, world, sprite_augment=None)
    differ = 0
    for i in range(6):
        px, pchar, panim, pmeta = plain[i]
        assert torch.equal(pchar, items[i][1]) and torch.equal(panim, items[i][2]) and pmeta["frame_paths"] == items[i][3]["frame_paths"]
        assert np.array_equal(plain.sample(i)[0], ds.sample(i)[0])
        differ += not torch.equal(px, items[i][0])
    assert differ == 6


@pytest.mark.parametrize("dim", [32, 97, 256])
def test_other_dimensions(model, world, dim):
    sprites, _, sprite_arrays, _ = world
    rng = np.random.default_rng(dim)
    stage_arrays = [rng.integers(0, 256, (300, 320, 3), dtype=np.uint8)]
    stages = sd.StageBank.from_arrays(model._engine, stage_arrays)
    ds = sd.SynthWindowDataset(model._engine, sprites, stages, animations=ANIMS, num_samples=2, num_frames_per_sample=S, img_dimension=dim,
                               paste_jitter=40, seed=6, sprite_augment={"hard_mode": 0.5, "resize": 0.6})
    for i in range(2):
        x, _, _, meta = ds[i]
        params, aug = ds.sample(i)[0].copy(), ds.sample_sprite_augment(i)
        params["sprite"] = np.arange(S)
        want = sd.composite_reference(list(sa.augment_sprites_reference(sprite_arrays, aug)), stage_arrays, params, dim, "uint8")
        assert tuple(x.shape) == (S, 3, dim, dim) and np.array_equal(np.stack(meta["frames"]), want)
    stages.close()


def test_one_training_step_from_a_device_batch_equals_one_from_the_twins_frames(model, world, state):
    ds = _dataset(model, world)
    batch = next(iter(ds.batches(3)))
    twins = [_twin_item(ds, world, i) for i in range(3)]
    host_batch = (torch.stack([t[0] for t in twins]), torch.stack([t[1] for t in twins]), torch.stack([t[2] for t in twins]), None)
    m_dev, m_host = _model(state), _model(state)
    loss_dev = m_dev.train().training_step(batch, 0)
    loss_host = m_host.train().training_step(host_batch, 0)
    assert loss_dev.is_cuda and float(loss_dev) > 0
    assert torch.equal(loss_dev.cpu().view(torch.int32), loss_host.cpu().view(torch.int32))
    sd_dev, sd_host = m_dev.state_dict(), m_host.state_dict()
    changed = 0
    for k in sd_dev:
        assert np.ascontiguousarray(sd_dev[k]).tobytes() == np.ascontiguousarray(sd_host[k]).tobytes(), k
        changed += not np.array_equal(np.asarray(sd_dev[k]), np.asarray(state[k]))
    assert changed >= 1
