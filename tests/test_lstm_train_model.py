"""Training of the LSTM head through the public interface: ``RNNActionDetector(freeze_encoder=True)`` -- ``train()``,
``training_step``, ``configure_optimizers``, ``state_dict`` / ``save_checkpoint``. A = 5, 8 windows of 4 frames; the kernels
themselves are pinned in tests/test_lstm_train.py."""
import numpy as np
import pytest
import torch

from playaid_core_amd import synth

pytestmark = pytest.mark.gpu

A, B, S = 5, 8, 4
ACTIONS = [f"action{i}" for i in range(A)]
LOGP_TOL = 1e-4


def _model(**kw):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from playaid_core_amd.rnn_action_detector import RNNActionDetector

    kw.setdefault("freeze_encoder", True)
    return RNNActionDetector("byleth", ACTIONS, state_dict=synth.make_rnn_state_dict(seed=21, num_actions=A), max_rows=64, **kw)


def test_training_step_lowers_the_loss_and_the_checkpoint_round_trips(tmp_path):
    from playaid_core_amd.rnn_action_detector import RNNActionDetector

    model = _model()
    try:
        g = torch.Generator().manual_seed(3)
        x = torch.rand(B, S, 3, 128, 128, generator=g)
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
        nll = -float(before.double()[torch.arange(B * S), action_label.view(B * S)].mean())
        assert abs(losses[0] - nll) <= LOGP_TOL   # step 0 reports the untrained model's NLL over all rows
        assert losses[-1] < losses[0]
        trainer = model.configure_optimizers()
        assert trainer is model.configure_optimizers() and trainer.steps == 10
        stats = trainer.epoch_stats()
        assert stats["windows"] == 10 * B * S == 320 and abs(stats["loss"] - float(np.mean(losses))) <= 1e-6
        assert model.eval() is model and not model.training
        after = model(x)
        assert float((after - before).abs().max()) > 1e-3    # inference reads the trained weights
        model.check()
        sd = model.state_dict()
        assert set(sd) == set(model._state_dict)
        for k, v in sd.items():
            same = np.array_equal(v.numpy(), np.asarray(model._state_dict[k]))
            assert same == k.startswith("resnet."), k   # the encoder as loaded, every LSTM and decoder tensor changed
        path = str(tmp_path / "trained.ckpt")
        model.save_checkpoint(path)
        loaded = RNNActionDetector.load_from_checkpoint(path, max_rows=64)
        try:
            assert loaded.freeze_encoder and loaded.actions == ACTIONS
            assert torch.equal(loaded(x).view(torch.int32), after.view(torch.int32))
        finally:
            loaded.close()
        model.check()
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
