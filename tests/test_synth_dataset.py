"""``synth_dataset.SynthWindowDataset`` on the device against the numpy twin on the host: items, batches, and one training step
of ``CNNActionDetector`` from a batch in the model layout -- the consumer that layout exists for. S = 3, A = 5; a tiny bank of
two characters, three actions (one outside the action list: "Unknown"), 5 to 9 frames each of 40..200 px sprites, two 200 x 160
stages."""
import numpy as np
import pytest
import torch

from playaid_core_amd import synth
from playaid_core_amd import synth_dataset as sd

pytestmark = pytest.mark.gpu

S, A = 3, 5
ACTIONS = ["Jab", "Dash", "Unknown", "Shield", "Roll"]   # the model's five classes
ANIMS = ACTIONS[:3]   # the dataset's list: the bank has Jab and Dash, and Grab outside the list (the reference's get_synth raises
                      # KeyError when its stand-in draw hits a listed action the character lacks, so every listed one exists)


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
                s[..., 3] = np.clip((1.2 - inside) * 400, 0, 255).astype(np.uint8)   # an opaque ellipse with a soft edge
                frames.append(s)
            tree[char][action] = {"c00": {f"{action.lower()}_raw": {"90": frames}}}
    stage_arrays = [rng.integers(0, 256, (160, 200, 3), dtype=np.uint8) for _ in range(2)]
    sprites = sd.SpriteBank.from_arrays(model._engine, tree)
    stages = sd.StageBank.from_arrays(model._engine, stage_arrays)
    sprite_arrays = [f for char in tree.values() for a in char.values() for f in a["c00"][next(iter(a["c00"]))]["90"]]
    assert len(sprite_arrays) == len(sprites) and sprites.shapes == [f.shape[:2] for f in sprite_arrays]
    yield sprites, stages, sprite_arrays, stage_arrays
    sprites.close()
    stages.close()


def _dataset(model, world, **kw):
    sprites, stages = world[:2]
    args = dict(animations=ANIMS, num_samples=8, num_frames_per_sample=S, move_stage_background=True, paste_jitter=40, seed=4)
    args.update(kw)
    return sd.SynthWindowDataset(model._engine, sprites, stages, **args)


def _twin_item(ds, world, idx):
    """Item ``idx`` built on the host: the same draw, the twin's frames, the reference's conversions."""
    _, _, sprite_arrays, stage_arrays = world
    params, char_label, actions, _ = ds.sample(idx)
    frames = sd.composite_reference(sprite_arrays, stage_arrays, params, 128, "uint8")
    return (torch.tensor(frames).permute(0, 3, 1, 2).float() / 255.0, torch.tensor(char_label),
            torch.tensor([ANIMS.index(a) for a in actions]), frames, params, actions)


def test_items_and_batches_equal_the_twin(model, world):
    ds = _dataset(model, world)
    sprites = world[0]
    assert len(ds) == 8
    items = [ds[i] for i in range(8)]
    labels = set()
    for i, (x, char, anim, meta) in enumerate(items):
        wx, wchar, wanim, frames, params, actions = _twin_item(ds, world, i)
        assert x.dtype == torch.float32 and tuple(x.shape) == (S, 3, 128, 128) and torch.equal(x, wx)
        assert torch.equal(char, wchar) and torch.equal(anim, wanim) and anim.dtype == torch.int64
        assert meta["char"] == ds.characters[int(char)] and meta["actions"] == actions
        assert len(meta["frames"]) == S and all(np.array_equal(f, w) for f, w in zip(meta["frames"], frames))
        assert meta["frame_paths"] == [sprites.paths[int(k)] for k in params["sprite"]]
        assert not np.array_equal(frames[0], frames[1])   # (frames, not copies of one stage crop)
        labels.update(anim.tolist())
    assert labels <= {0, 1, 2} and len(labels) >= 2
    got = list(ds.batches(4))
    assert len(got) == 2
    for b, (x, char, anim, metas) in enumerate(got):
        assert x.is_cuda and char.is_cuda and anim.is_cuda and x.is_contiguous() and tuple(x.shape) == (4, S, 3, 128, 128)
        part = items[4 * b:4 * b + 4]
        assert torch.equal(x.cpu(), torch.stack([it[0] for it in part]))
        assert torch.equal(char.cpu(), torch.stack([it[1] for it in part])) and torch.equal(anim.cpu(), torch.stack([it[2] for it in part]))
        assert [m["actions"] for m in metas] == [it[3]["actions"] for it in part]
        assert [m["frame_paths"] for m in metas] == [it[3]["frame_paths"] for it in part]
    ds.set_epoch(1)
    assert not torch.equal(ds[0][0], items[0][0])
    ds.set_epoch(0)
    assert torch.equal(ds[0][0], items[0][0])
    assert len(list(_dataset(model, world, num_samples=5).batches(4))[1][0]) == 1   # the last batch is what is left


def test_simple_item_is_the_fixed_frame_form(model, world):
    ds = _dataset(model, world)
    sprites, _, sprite_arrays, stage_arrays = world
    mario_dash = sprites.tree["mario"]["Dash"]["c00"]["dash_raw"]["90"]
    link_grab = sprites.tree["link"]["Grab"]["c00"]["grab_raw"]["90"]
    link_jab = sprites.tree["link"]["Jab"]["c00"]["jab_raw"]["90"]
    batch_1, batch_2 = [mario_dash[0], link_grab[1], mario_dash[2]], [link_jab[0], mario_dash[1], link_jab[2]]
    for idx in (0, 1, 2, 3):
        x, char, anim, meta = ds.simple_item(idx, [batch_1, batch_2])
        frames = batch_1 if idx % 2 else batch_2   # the reference's parity (ult_action_dataset.py:398)
        params = np.zeros(3, dtype=sd.PARAMS_DTYPE)
        params["sprite"] = frames   # stage 0, origin (0, 0), centred
        want = sd.composite_reference(sprite_arrays, stage_arrays, params, 128, "uint8")
        assert torch.equal(x, torch.tensor(want).permute(0, 3, 1, 2).float() / 255.0)
        assert meta["frame_paths"] == ["0.png", "1.png", "2.png"]
        if idx % 2:   # the first frame's character and action label all three
            assert meta["char"] == "mario" and int(char) == 0 and anim.tolist() == [1, 1, 1] and meta["actions"] == ["Dash"] * 3
        else:
            assert meta["char"] == "link" and int(char) == 1 and anim.tolist() == [0, 0, 0] and meta["actions"] == ["Jab"] * 3
    x, _, anim, _ = ds.simple_item(5, batch_2)   # a plain list is taken as it is, whatever idx
    assert anim.tolist() == [0, 0, 0] and tuple(x.shape) == (3, 3, 128, 128)
    with pytest.raises(ValueError):   # Grab is outside the list: the reference's animations.index(action) raises
        ds.simple_item(0, [link_grab[0], mario_dash[1], link_grab[2]])
    with pytest.raises(ValueError):
        ds.simple_item(0, [batch_1, batch_2, batch_1])


def test_one_training_step_from_a_device_batch_equals_one_from_the_twins_frames(model, world, state):
    """Two fresh models from the same state dict, one step each: the batch ``batches(4)`` composed on the device in the model
    layout, and the twin's frames converted on the host as the reference's ``__getitem__`` converts them. Bit-equal losses and
    head weights tie the new layout to ``pa_backbone_windows``."""
    ds = _dataset(model, world)
    batch = next(iter(ds.batches(4)))
    twins = [_twin_item(ds, world, i) for i in range(4)]
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
    assert changed >= 1   # (the step moved the head: the equality is not of two untouched copies)


def test_synth_difficulty_is_refused_by_name(model, world):
    for level in (1, 2):
        with pytest.raises(NotImplementedError, match="augment_synth_char_crop"):
            _dataset(model, world, synth_difficulty=level)
