"""Training of the encoder head through the public interface: ``ResnetTransformerDetector(freeze_encoder=True)`` -- ``train()``,
``training_step``, ``configure_optimizers``, ``state_dict`` / ``save_checkpoint``. A = 5, 8 windows of 4 frames of 64 x 64 pixels,
no dropout; the kernels themselves are pinned in tests/test_encoder_train.py."""
import numpy as np
import pytest
import torch

from playaid_core_amd import synth

pytestmark = pytest.mark.gpu

A, B, S, CROP = 5, 8, 4, 64
ACTIONS = [f"action{i}" for i in range(A)]
LOGP_TOL = 1e-4
# A tenth of the model's default rate. Adam's first steps move every weight by about lr whatever the gradient's size, and the front
# projection sums 2048 features of a random-weight ResNet-50 (mean |x| 1.2): at 2e-4 one step shifts each of its outputs by up to
# lr * sum|x| ~ 0.5, as much as the outputs themselves, and ten steps on these 32 rows overshoot before they descend -- in torch's
# float64 Adam on the same features exactly as on the device (3.53, 14.01, 14.12, ..., 3.76 in both). At 2e-5 they descend.
LR = 2e-5


def _model(**kw):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from playaid_core_amd.resnet_transformer_detector import ResnetTransformerDetector

    kw.setdefault("freeze_encoder", True)
    return ResnetTransformerDetector(ACTIONS, sequence_length=S, state_dict=synth.make_resformer_state_dict(seed=21, num_actions=A, sequence_length=S),
                                     max_rows=64, crop_size=CROP, dropout=0.0, learning_rate=LR, **kw)


def test_training_step_lowers_the_loss_and_the_checkpoint_round_trips(tmp_path):
    from playaid_core_amd import encoder_trainer
    from playaid_core_amd.resnet_transformer_detector import ResnetTransformerDetector

    model = _model()
    try:
        g = torch.Generator().manual_seed(3)
        x = torch.rand(B, S, 3, CROP, CROP, generator=g)
        action_label = torch.randint(0, A, (B, S), generator=g)
        batch = (x.cuda(), torch.zeros(B, dtype=torch.long), action_label, None)
        before = model(x)
        with pytest.raises(RuntimeError):
            model.training_step(batch, 0)            # eval mode
        assert model.train() is model and model.training
        losses = [model.training_step(batch, i) for i in range(10)]
        assert all(l.is_cuda and l.dim() == 0 and l.dtype == torch.float32 for l in losses)
        losses = [float(l) for l in losses]
        print("losses", " ".join(f"{l:.4f}" for l in losses))
        nll = -float(before.double().reshape(B * S, A)[torch.arange(B * S), action_label.view(B * S)].mean())
        assert abs(losses[0] - nll) <= LOGP_TOL   # step 0 reports the untrained model's NLL over all rows
        assert losses[-1] < losses[0]
        trainer = model.configure_optimizers()
        assert trainer is model.configure_optimizers() and trainer.steps == 10
        assert isinstance(trainer, encoder_trainer.EncoderTrainer) and trainer.dropout == 0.0 and trainer.lr == model.learning_rate == LR
        stats = trainer.epoch_stats()
        assert stats["windows"] == 10 * B * S == 320 and abs(stats["loss"] - float(np.mean(losses))) <= 1e-6
        assert model.eval() is model and not model.training
        after = model(x)
        assert float((after - before).abs().max()) > 1e-3    # inference reads the trained weights
        sd = model.state_dict()
        assert set(sd) == set(model._state_dict)
        trained = set(trainer.keys)
        assert trained <= set(sd) and len(trained) == 2 + 12 * 3 + 2
        assert any(k.startswith("model.resnet_classifier.") for k in sd) and "model.freq_encoding" in sd
        for k, v in sd.items():
            same = np.array_equal(v.numpy(), np.asarray(model._state_dict[k]))
            assert same == (k not in trained), k   # the ResNet-50, the encoding and the unused tensors as loaded, every trained tensor changed
        path = str(tmp_path / "trained.ckpt")
        model.save_checkpoint(path)
        loaded = ResnetTransformerDetector.load_from_checkpoint(path, max_rows=64)
        try:
            assert loaded.freeze_encoder is True and loaded.actions == ACTIONS and loaded.crop_size == CROP
            assert torch.equal(loaded(x).view(torch.int32), after.view(torch.int32))
        finally:
            loaded.close()
    finally:
        model.close()


def test_training_the_encoder_is_still_refused():
    model = _model(freeze_encoder=False)
    try:
        with pytest.raises(NotImplementedError):
            model.train()
        with pytest.raises(NotImplementedError):
            model.configure_optimizers()
        assert model.train(False) is model and not model.training
        assert model.eval() is model
    finally:
        model.close()
