"""Augmented training through the public surface: ``AIRunner.fit_head(synth_difficulty=...)`` and
``ClipWindowDataset(synth_difficulty=...)`` on a synthetic clip of 12 frames, 2 fighters, S = 7, A = 5 (the kernel itself is
pinned to its numpy twin in tests/test_augment.py)."""
import numpy as np
import pytest
import torch

from playaid_core_amd import augment, synth
from playaid_core_amd.dataset_utils import action_sample_from_frame_middle_out

pytestmark = pytest.mark.gpu

S, A, N = 7, 5, 12
ACTIONS = [f"action{i}" for i in range(A)]
LOGP_TOL = 1e-4   # tests/test_head_train.py: log-probabilities, hence a step's loss


@pytest.fixture(scope="module")
def sd():
    return synth.make_state_dict(seed=21, num_actions=A, sequence_length=S)


def _runner(sd, tmp_path, name="out"):
    from playaid_core_amd.ai_runner import AIRunner, ClipSource
    from playaid_core_amd.cnn_action_detector import CNNActionDetector

    model = CNNActionDetector(ACTIONS, sequence_length=S, state_dict=sd, max_batch_frames=16, max_clip_frames=64, max_frame_height=96,
                              max_frame_width=128, freeze_encoder=True, learning_rate=1e-3)
    return AIRunner(ClipSource.synthetic(N, 96, 128), model=model, output_dir=str(tmp_path / name), crop_mode="square", crop_jpeg_quality=0,
                    num_frames_per_sample=S)


def _truth(runner):
    """The untrained model's own predictions with fighter 0's second half moved to the next class (as test_head_train_model)."""
    runner.run_action_recognition()
    n = runner.max_frames
    pred = np.array([[ACTIONS.index(runner.ai_output_data[f][i].action) for i in range(n - 1)] for f in runner.fighters])
    truth = pred.copy()
    truth[0, n // 2:] = (truth[0, n // 2:] + 1) % A
    return [[ACTIONS[a] for a in row] for row in truth], pred


def _weights(runner):
    return {k: v.clone() for k, v in runner.model.configure_optimizers().read("weights").items()}


def _same(a, b):
    return all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in a)


def test_level_0_is_the_present_path(sd, tmp_path):
    a, b = _runner(sd, tmp_path, "a"), _runner(sd, tmp_path, "b")
    gt, _ = _truth(a)
    ha = a.fit_head(actions=gt, epochs=2, batch_size=8, seed=3)
    hb = b.fit_head(actions=gt, epochs=2, batch_size=8, seed=3, synth_difficulty=0, raise_difficulty=False)
    assert _same(_weights(a), _weights(b))
    assert ha == hb and [h["synth_difficulty"] for h in ha] == [0, 0]
    for bad in (3, -1, 1.5):
        with pytest.raises(ValueError):
            a.fit_head(actions=gt, synth_difficulty=bad)


def test_augmented_fit_is_a_function_of_the_seed(sd, tmp_path):
    runs = []
    for name, seed in (("a", 3), ("b", 3), ("c", 4)):
        r = _runner(sd, tmp_path, name)
        gt, _ = _truth(r)
        start = _weights(r)
        hist = r.fit_head(actions=gt, epochs=2, batch_size=8, seed=seed, synth_difficulty=2)
        assert [h["synth_difficulty"] for h in hist] == [2, 2] and all(h["windows"] == 2 * (N - 1) for h in hist)
        assert not r.model.training
        runs.append(_weights(r))
        assert not _same(start, runs[-1])
    assert _same(runs[0], runs[1]) and not _same(runs[0], runs[2])


def test_first_steps_loss_is_a_training_step_on_the_twins_crops(sd, tmp_path):
    """One epoch in one minibatch: its loss (taken before the update) against ``training_step`` of an untrained copy of the
    model fed what the numpy twin makes of the same crops with the same draw."""
    level, seed = 2, 5
    r = _runner(sd, tmp_path, "a")
    gt, _ = _truth(r)
    crops = r._run_clip()["crops_rgb"][: N - 1].copy()
    F = crops.shape[1]
    hist = r.fit_head(actions=gt, epochs=1, batch_size=32, seed=seed, synth_difficulty=level)
    # the same draw: fit_head's windows in label_table's order, its permutation, then the minibatch's records
    from playaid_core_amd.ult_action_dataset import label_table
    table = label_table(r, gt, ACTIONS)
    idx = np.argwhere(table != -100)
    assert len(idx) == 2 * (N - 1) <= 32
    wins = np.array([[(f - 1) * F + p for f in action_sample_from_frame_middle_out(int(i) + 1, num_frames_per_sample=S, frame_delta=r.frame_delta,
                                                                                 max_frames=N, min_frame=1)] for i, p in idx])
    labels = table[idx[:, 0], idx[:, 1]]
    rng = np.random.default_rng(seed)
    order = rng.permutation(len(idx))
    params = augment.sample_params(len(order) * S, level, rng, src=wins[order].ravel())
    x = augment.augment_reference(crops.reshape(-1, 128, 128, 3), params, "model").reshape(len(order), S, 3, 128, 128)
    fresh = _runner(sd, tmp_path, "b").model.train()
    action_label = np.full((len(order), S), -100, dtype=np.int64)
    action_label[:, S // 2] = labels[order]
    loss = float(fresh.training_step((torch.from_numpy(x).cuda(), None, torch.from_numpy(action_label), None), 0))
    print(f"fit_head step 0 loss {hist[0]['loss']:.7f}, training_step on the twin's crops {loss:.7f}")
    assert abs(hist[0]["loss"] - loss) <= LOGP_TOL
    # and the augmentation mattered: the plain crops give another loss
    plain = float(_runner(sd, tmp_path, "c").model.train().training_step(
        (torch.from_numpy(crops.reshape(-1, 128, 128, 3)[wins[order].ravel()]).permute(0, 3, 1, 2).float().div(255).view(len(order), S, 3, 128, 128).cuda(),
         None, torch.from_numpy(action_label), None), 0))
    assert abs(plain - loss) > 10 * LOGP_TOL


def test_raise_difficulty_follows_the_epochs_accuracy(sd, tmp_path):
    """Ground truth = the model's own predictions: the first epoch (level 0, the plain crops through the augmented path) is
    all correct, so the second runs at level 1; the level never falls and stops at 2."""
    r = _runner(sd, tmp_path, "a")
    _, pred = _truth(r)
    gt = [[ACTIONS[a] for a in row] for row in pred]
    hist = r.fit_head(actions=gt, epochs=4, batch_size=8, seed=1, synth_difficulty=0, raise_difficulty=True)
    levels = [h["synth_difficulty"] for h in hist]
    assert hist[0]["accuracy"] > 0.85 and levels[:2] == [0, 1]
    assert all(0 <= b - a <= 1 for a, b in zip(levels, levels[1:])) and max(levels) <= 2


def test_dataset_items(sd, tmp_path):
    from playaid_core_amd.ult_action_dataset import ClipWindowDataset

    r = _runner(sd, tmp_path, "a")
    gt, _ = _truth(r)
    plain = ClipWindowDataset(r, actions=gt, animations=ACTIONS)
    level0 = ClipWindowDataset(r, actions=gt, animations=ACTIONS, synth_difficulty=0, seed=9)
    level1 = ClipWindowDataset(r, actions=gt, animations=ACTIONS, synth_difficulty=1, seed=9)
    crops = r._run_clip()["crops_rgb"][: N - 1]
    F = crops.shape[1]
    flat = np.ascontiguousarray(crops).reshape(-1, 128, 128, 3)
    assert len(level1) == len(plain) == 2 * (N - 1)
    for idx in (0, 5, N - 2, N - 1, 2 * (N - 1) - 1):
        a, b, c = plain[idx], level0[idx], level1[idx]
        assert torch.equal(a[0], b[0]) and torch.equal(a[2], b[2]) and all(np.array_equal(u, v) for u, v in zip(a[3]["frames"], b[3]["frames"]))
        p, frame = idx // (N - 1), 1 + idx % (N - 1)
        frame_nums = action_sample_from_frame_middle_out(frame, num_frames_per_sample=S, frame_delta=r.frame_delta, max_frames=N, min_frame=1)
        params = augment.sample_params(S, 1, np.random.default_rng([9, 0, idx]), src=[(f - 1) * F + p for f in frame_nums])
        want = augment.augment_reference(flat, params, "uint8")
        assert np.array_equal(np.array(c[3]["frames"]), want)
        assert torch.equal(c[0], torch.from_numpy(augment.augment_reference(flat, params, "model")))
        assert torch.equal(c[2], a[2]) and c[3]["actions"] == a[3]["actions"] and not torch.equal(c[0], a[0])
        assert torch.equal(level1[idx][0], c[0])   # a pure function of (seed, epoch, idx)
    first = level1[3][0]
    level1.set_epoch(1)
    assert not torch.equal(level1[3][0], first)
    level1.set_epoch(0)
    assert torch.equal(level1[3][0], first)
    assert not torch.equal(ClipWindowDataset(r, actions=gt, animations=ACTIONS, synth_difficulty=1, seed=10)[3][0], first)


def test_make_synth_more_challenging_stops_at_2(sd, tmp_path):
    from playaid_core_amd.ult_action_dataset import ClipWindowDataset

    r = _runner(sd, tmp_path, "a")
    ds = ClipWindowDataset(r, animations=ACTIONS + ["Undefined"])
    seen = []
    for _ in range(4):
        seen.append(ds.synth_difficulty)
        ds.make_synth_more_challenging()
    assert seen == [0, 1, 2, 2] and ds.synth_difficulty == 2
    with pytest.raises(ValueError, match="5.8c"):
        ClipWindowDataset(r, animations=ACTIONS + ["Undefined"], crop_size=64, synth_difficulty=1)
    with pytest.raises(ValueError):
        ClipWindowDataset(r, animations=ACTIONS + ["Undefined"], synth_difficulty=3)
    sized = ClipWindowDataset(r, animations=ACTIONS + ["Undefined"], crop_size=64)
    with pytest.raises(ValueError, match="5.8c"):
        sized.make_synth_more_challenging()
    assert sized.synth_difficulty == 0
