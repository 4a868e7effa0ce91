"""Training of the temporal head through the public interface: ``CNNActionDetector(freeze_encoder=True)`` --
``train()``, ``training_step``, ``state_dict`` / ``save_checkpoint`` -- and ``AIRunner.fit_head`` on a small synthetic clip.
S = 3, A = 5; the kernels themselves are pinned in tests/test_head_train.py."""
import numpy as np
import pytest
import torch

from playaid_core_amd import synth

pytestmark = pytest.mark.gpu

S, A = 3, 5
ACTIONS = [f"action{i}" for i in range(A)]


def _model(sd=None, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from playaid_core_amd.cnn_action_detector import CNNActionDetector

    sd = synth.make_state_dict(seed=21, num_actions=A, sequence_length=S) if sd is None else sd
    kw.setdefault("freeze_encoder", True)
    return CNNActionDetector(ACTIONS, sequence_length=S, state_dict=sd, max_batch_frames=16, max_clip_frames=64,
                             max_frame_height=96, max_frame_width=128, **kw)


def test_training_step_lowers_the_loss_and_the_checkpoint_round_trips(tmp_path):
    from playaid_core_amd.cnn_action_detector import CNNActionDetector

    model = _model()
    g = torch.Generator().manual_seed(3)
    x = torch.rand(8, S, 3, 128, 128, generator=g)
    action_label = torch.randint(0, A, (8, S), generator=g)
    batch = (x.cuda(), torch.zeros(8, dtype=torch.long), action_label, None)
    before = model(x)
    with pytest.raises(RuntimeError):
        model.training_step(batch, 0)            # eval mode
    assert model.train() is model and model.training
    losses = [model.training_step(batch, i) for i in range(10)]
    assert all(l.is_cuda and l.dim() == 0 and l.dtype == torch.float32 for l in losses)
    losses = [float(l) for l in losses]
    print("losses", " ".join(f"{l:.4f}" for l in losses))
    centre = action_label[:, S // 2]
    assert abs(losses[0] + float(before[torch.arange(8), centre].mean())) <= 1e-4   # step 0 reports the untrained model's NLL
    assert losses[-1] < losses[0]
    trainer = model.configure_optimizers()
    assert trainer is model.configure_optimizers() and trainer.steps == 10
    stats = trainer.epoch_stats()
    assert stats["windows"] == 80 and abs(stats["loss"] - float(np.mean(losses))) <= 1e-6
    model.eval()
    after = model(x)
    assert float((after - before).abs().max()) > 1e-3    # inference reads the trained weights
    with pytest.raises(ValueError):
        model.metrics("train")                            # (pinned elsewhere: the running figures live on the trainer)
    sd = model.state_dict()
    assert set(sd) == set(model._state_dict) and not np.array_equal(sd["model.cnn1d.0.weight"], model._state_dict["model.cnn1d.0.weight"])
    assert np.array_equal(sd["model.cnn2d.conv1.weight"], model._state_dict["model.cnn2d.conv1.weight"])
    path = str(tmp_path / "trained.ckpt")
    model.save_checkpoint(path)
    loaded = CNNActionDetector.load_from_checkpoint(path, actions=ACTIONS, max_batch_frames=16, max_clip_frames=64)
    assert loaded.freeze_encoder and loaded.sequence_length == S
    assert torch.equal(loaded(x).view(torch.int32), after.view(torch.int32))


def test_training_the_encoder_is_still_refused():
    model = _model(freeze_encoder=False)
    with pytest.raises(NotImplementedError):
        model.train()
    with pytest.raises(NotImplementedError):
        model.configure_optimizers()
    assert model.train(False) is model and not model.training


def test_fit_head_on_a_synthetic_clip(tmp_path):
    """Ground truth = the untrained model's own predictions with a third of them moved to the next class: the model starts at
    about 2/3 accuracy on it and must end higher; one history row per epoch. The third is one contiguous run -- the first
    fighter's frames from a third of the clip on, 16 of the 46 windows -- as a corrected ground-truth CSV relabels a stretch of
    frames. (Flipping every third window instead asks the head to tell neighbouring frames of one fighter apart, whose
    features are nearly equal: torch's own Adam on the same features stays at 30 / 46 with the loss at the entropy of a
    1/3 : 2/3 mix, 0.625, after these 30 epochs, and reaches 42 / 46 on the contiguous run.)"""
    from playaid_core_amd.ai_runner import AIRunner, ClipSource

    model = _model(learning_rate=1e-3)
    runner = AIRunner(ClipSource.synthetic(24, 96, 128), model=model, output_dir=str(tmp_path / "out"), crop_mode="square",
                      crop_jpeg_quality=0, num_frames_per_sample=S)
    runner.run_action_recognition()
    n, F = runner.max_frames, len(runner.fighters)
    pred = np.array([[ACTIONS.index(runner.ai_output_data[f][i].action) for i in range(n - 1)] for f in runner.fighters])
    truth = pred.copy()
    flip = (n - 1) // 3
    truth[0, flip:] = (truth[0, flip:] + 1) % A
    assert abs((truth != pred).mean() - 1 / 3) < 0.02
    gt = [[ACTIONS[a] for a in row] for row in truth]
    acc0 = runner.evaluate(actions=gt)["accuracy"]
    assert abs(acc0 - (pred == truth).mean()) < 1e-9
    hist = runner.fit_head(actions=gt, epochs=30, batch_size=16, seed=1)
    assert [h["epoch"] for h in hist] == list(range(30)) and all(h["windows"] == truth.size for h in hist)
    assert hist[-1]["loss"] < hist[0]["loss"]
    assert not model.training
    out = runner.evaluate(actions=gt)
    print(f"accuracy {acc0:.3f} -> {out['accuracy']:.3f}, epoch loss {hist[0]['loss']:.4f} -> {hist[-1]['loss']:.4f}")
    assert out["accuracy"] > acc0
    assert runner.fit_head(actions=gt, epochs=1, batch_size=16, seed=1)[0]["epoch"] == 0
    with pytest.raises(ValueError):
        runner.fit_head(actions=gt, ground_truth_csv="x.csv")
