"""``RNNActionDetector`` -- the reference's alternative temporal model.

Mirror of ``playaid/models/rnn_action_detector.py:14-95`` for inference: torchvision ``resnet18`` with
``fc = Sequential(Linear(512, 300))`` per frame, ``nn.LSTM(300, 512, num_layers=3)``, ``Linear(512, 128)`` + ReLU,
``Linear(128, A)``, ``log_softmax``; ``model(x)`` with ``x: float32[B,S,3,128,128]`` -> ``float32[B*S, A]``, one row
per (window, frame) (``:74-95``). The reference gives the LSTM a ``[B, S, 300]`` tensor without ``batch_first``, so
the recurrence runs over the WINDOWS of a call and the frames of a window are its batch; that is kept as is.

The backbone runs on the engine's convolution kernels (``pa_backbone_windows``: the fc rows are zero-padded from 300
to the engine's 1000, the Conv1d head of the engine is unused), the recurrent head and decoder in
``csrc/lstm.hip`` (``pa_lstm_forward``). No PyTorch fallback.

Scoring is mirrored (``validation_step`` / ``test_step``, ``:132-160``): this model's reference scores EVERY row of its
``[B*S, A]`` output against ``action_label.view(B * S)`` (not the centre label the CNN model scores) -- NLL loss and multiclass
top-1 accuracy, accumulated on the device (``metrics.EvalState``) with nothing read back per step; ``metrics(split)`` is the
one read (``val_action_loss``, ``val_action_acc``, ... plus confusion matrix and mean confidence), ``reset_metrics(split)``
clears a split.

Training is mirrored for the recurrent head with the encoder frozen (``freeze_encoder=True``; ``lstm_trainer.LSTMTrainer``,
csrc/lstm_train.hip): ``train()``, ``configure_optimizers()`` (the reference's ``torch.optim.Adam(lr=self.learning_rate)``,
``:162-164``), ``training_step`` (``:97-117``: NLL over every row against ``action_label.view(B * S)``), ``state_dict()`` and
``save_checkpoint()``. ``resnet.*`` -- ``resnet.fc.0`` included -- stays as loaded and runs on the inference kernels with
eval-mode BatchNorm. Not mirrored: training the encoder and its BatchNorm statistics, ``training_epoch_end`` and the data hooks
(``:119-130, 166-260``).
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, List, Mapping, Optional

import numpy as np
import torch

from . import _lib
from .engine import Engine, EngineError, _ptr
from .metrics import SplitMetrics
from .synth import resnet18_param_shapes

INPUT_DIM, HIDDEN_DIM, NUM_LAYERS = 300, 512, 3


def _np(v) -> np.ndarray:
    return v if isinstance(v, np.ndarray) else v.detach().cpu().numpy()


def backbone_state_dict(state_dict: Mapping) -> Dict[str, np.ndarray]:
    """``resnet.*`` tensors re-keyed for ``Engine`` (``model.cnn2d.*``): fc zero-padded 300 -> 1000 rows, a zero
    one-tap Conv1d head and classifier (never run)."""
    out: Dict[str, np.ndarray] = {}
    for key, shape in resnet18_param_shapes():
        if key.startswith("fc."):
            continue
        a = np.ascontiguousarray(_np(state_dict["resnet." + key]), dtype=np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"resnet.{key}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
        out["model.cnn2d." + key] = a
    w = np.ascontiguousarray(_np(state_dict["resnet.fc.0.weight"]), dtype=np.float32)
    b = np.ascontiguousarray(_np(state_dict["resnet.fc.0.bias"]), dtype=np.float32)
    if w.shape != (INPUT_DIM, 512) or b.shape != (INPUT_DIM,):
        raise ValueError(f"resnet.fc.0: expected (300, 512) / (300,), got {w.shape} / {b.shape}")
    fw = np.zeros((1000, 512), dtype=np.float32)
    fb = np.zeros((1000,), dtype=np.float32)
    fw[:INPUT_DIM] = w
    fb[:INPUT_DIM] = b
    out["model.cnn2d.fc.weight"] = fw
    out["model.cnn2d.fc.bias"] = fb
    out["model.cnn1d.0.weight"] = np.zeros((512, 1000, 1), dtype=np.float32)
    out["model.cnn1d.0.bias"] = np.zeros((512,), dtype=np.float32)
    out["model.classifier.0.weight"] = np.zeros((128, 512), dtype=np.float32)
    out["model.classifier.0.bias"] = np.zeros((128,), dtype=np.float32)
    out["model.classifier.2.weight"] = np.zeros((1, 128), dtype=np.float32)
    out["model.classifier.2.bias"] = np.zeros((1,), dtype=np.float32)
    return out


def pack_lstm_blob(state_dict: Mapping, num_actions: int) -> np.ndarray:
    """-> uint8 blob of ``pa_lstm_create`` (layout: include/playaid_hip.h)."""
    parts = [np.array([_lib.PA_LSTM_MAGIC, 1, INPUT_DIM, HIDDEN_DIM, NUM_LAYERS, num_actions, 0, 0], dtype=np.int32).view(np.uint8)]

    def take(key, shape):
        if key not in state_dict:
            raise KeyError(f"state_dict is missing {key}")
        a = np.ascontiguousarray(_np(state_dict[key]), dtype=np.float32)
        if tuple(a.shape) != tuple(shape):
            raise ValueError(f"{key}: expected shape {tuple(shape)}, got {tuple(a.shape)}")
        parts.append(a.reshape(-1).view(np.uint8))

    for layer in range(NUM_LAYERS):
        in_dim = INPUT_DIM if layer == 0 else HIDDEN_DIM
        take(f"lstm.weight_ih_l{layer}", (4 * HIDDEN_DIM, in_dim))
        take(f"lstm.weight_hh_l{layer}", (4 * HIDDEN_DIM, HIDDEN_DIM))
        take(f"lstm.bias_ih_l{layer}", (4 * HIDDEN_DIM,))
        take(f"lstm.bias_hh_l{layer}", (4 * HIDDEN_DIM,))
    take("action_decoder.0.weight", (128, HIDDEN_DIM))
    take("action_decoder.0.bias", (128,))
    take("action_decoder.2.weight", (num_actions, 128))
    take("action_decoder.2.bias", (num_actions,))
    return np.concatenate(parts)


class RNNActionDetector:
    def __init__(
        self,
        fighter_name: str,
        actions: List[str],
        batch_size: int = 8,
        learning_rate: float = 2e-4,
        num_samples: int = 1024,
        freeze_encoder=False,
        state_dict: Optional[Mapping] = None,
        device: str = "cuda:0",
        max_rows: int = 1024,
        **kwargs,
    ):
        if state_dict is None:
            raise ValueError("RNNActionDetector needs weights: use load_from_checkpoint() or pass state_dict=")
        a = int(_np(state_dict["action_decoder.2.weight"]).shape[0])
        if a != len(actions):
            raise ValueError(f"checkpoint has {a} action logits but {len(actions)} actions were given")
        self.fighter_name = fighter_name
        self.actions = list(actions)
        self.num_actions = a
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.num_samples = num_samples
        self.dataset_kwargs = kwargs
        self.freeze_encoder = bool(freeze_encoder)
        self.training = False
        self._trainer = None
        self._state_dict = {k: v for k, v in state_dict.items()}   # (resnet.* as loaded: state_dict() hands it back)
        self.max_rows = max_rows
        # (compute_dtype: beyond the reference's arguments -- "emulated_f32" puts the backbone's stride-2 openers and branch GEMMs on the
        # emulated-fp32 kernels, PA_DTYPE_EMULATED_F32; never the default)
        self._engine = Engine(backbone_state_dict(state_dict), device=device, num_fighters=1, frame_delta=1,
                              max_batch_frames=min(max_rows, 128), max_clip_frames=1, compute_dtype=kwargs.get("compute_dtype", "f32"))
        self._lib = self._engine._lib
        blob = pack_lstm_blob(state_dict, a)
        assert blob.nbytes == self._lib.pa_lstm_blob_bytes(INPUT_DIM, HIDDEN_DIM, NUM_LAYERS, a)
        h = C.c_void_p()
        rc = self._lib.pa_lstm_create(self._engine.device.index or 0, INPUT_DIM, HIDDEN_DIM, NUM_LAYERS, a, max_rows,
                                      blob.ctypes.data_as(C.c_void_p), blob.nbytes, C.byref(h))
        self._h = h
        if rc != 0:
            msg = self._lib.pa_lstm_last_error(h).decode() if h else "bad argument"
            self.close()
            raise EngineError(rc, msg)
        self._feats = torch.zeros((max_rows, _lib.PA_FEATURE_STRIDE), dtype=torch.float32, device=self._engine.device)

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path: str, map_location=None, **kwargs):
        """Lightning ``.ckpt`` (``state_dict`` + ``hyper_parameters``; keyword arguments override the saved ones,
        as in ``visualizations/rnn_action_detector_vis.py:79-84``)."""
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        if "state_dict" not in ckpt:
            raise KeyError(f"{checkpoint_path} has no 'state_dict' (not a Lightning checkpoint)")
        hparams = dict(ckpt.get("hyper_parameters", {}) or {})
        hparams.update(kwargs)
        return cls(state_dict=ckpt["state_dict"], **hparams)

    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode and not self.freeze_encoder:
            raise NotImplementedError("only the LSTM head trains: build the model with freeze_encoder=True")
        self.training = bool(mode)
        return self

    # -- training (rnn_action_detector.py:97-117, 162-164; the encoder frozen) -------------
    def configure_optimizers(self):
        """The reference's ``torch.optim.Adam(self.parameters(), lr=self.learning_rate)`` for what trains here: the one
        ``LSTMTrainer`` on this model's handle (made once; it owns the Adam moments and the running epoch statistics)."""
        if not self.freeze_encoder:
            raise NotImplementedError("only the LSTM head trains: build the model with freeze_encoder=True")
        if self._trainer is None:
            from .lstm_trainer import LSTMTrainer

            self._trainer = LSTMTrainer(self, lr=self.learning_rate)
        return self._trainer

    def training_step(self, batch, batch_idx):
        """``batch = (input [B,S,3,128,128], char_label, action_label [B,S], ...)``: the ResNet-18 features of every frame
        (``pa_backbone_windows``), then one ``pa_lstm_train_step`` with ``action_label.view(B * S)`` (``-100`` = no ground
        truth). -> the loss before the update, a 0-dim float32 device tensor; nothing waits."""
        if not self.training:
            raise RuntimeError("training_step in eval mode: call train() first")
        input, action_label = batch[0], batch[2]
        if input.dim() != 5 or tuple(input.shape[2:]) != (3, 128, 128):
            raise ValueError(f"expected [B,S,3,128,128], got {tuple(input.shape)}")
        b, s = int(input.shape[0]), int(input.shape[1])
        if b * s > self.max_rows:
            raise ValueError(f"{b} x {s} rows exceed max_rows={self.max_rows}")
        trainer = self.configure_optimizers()
        eng = self._engine
        xd = eng._dev(input, torch.float32)
        eng._check(self._lib.pa_backbone_windows(eng._h, _ptr(xd), b * s, _ptr(self._feats), eng._stream()))
        labels = action_label.reshape(b * s) if isinstance(action_label, torch.Tensor) else np.asarray(action_label).reshape(b * s)
        stats = trainer.step(self._feats[:b * s], b, s, labels)
        return trainer.loss_of(stats)

    def state_dict(self) -> Dict[str, torch.Tensor]:
        """The key set the model was built from: ``resnet.*`` (and anything else it carried) as loaded, the trained tensors as
        they are on the device now (CPU tensors; waits for the read when a trainer exists)."""
        out = {k: (v.detach().cpu() if isinstance(v, torch.Tensor) else torch.from_numpy(np.array(v))) for k, v in self._state_dict.items()}
        if self._trainer is not None:
            for k, v in self._trainer.read("weights").items():
                out[k] = v.cpu()
        return out

    def save_checkpoint(self, path: str):
        """A Lightning-shaped ``.ckpt`` (``state_dict`` + ``hyper_parameters``) that ``load_from_checkpoint`` reads back."""
        hparams = dict(fighter_name=self.fighter_name, actions=list(self.actions), batch_size=self.batch_size,
                       learning_rate=self.learning_rate, num_samples=self.num_samples, freeze_encoder=self.freeze_encoder)
        hparams.update(self.dataset_kwargs)
        torch.save({"state_dict": self.state_dict(), "hyper_parameters": hparams}, path)

    def close(self):
        if getattr(self, "_trainer", None) is not None:
            self._trainer.close()   # (before the handle whose weights it borrows)
            self._trainer = None
        if getattr(self, "_h", None):
            self._lib.pa_lstm_destroy(self._h)
            self._h = None
        if getattr(self, "_metrics", None) is not None:
            self._metrics.close()
            self._metrics = None
        if getattr(self, "_engine", None) is not None:
            self._engine.close()
            self._engine = None

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [batch_size, frames_per_sequence, channel, height, width] -> log-probabilities [batch * frames, A]."""
        if x.dim() != 5 or tuple(x.shape[2:]) != (3, 128, 128):
            raise ValueError(f"expected [B,S,3,128,128], got {tuple(x.shape)}")
        b, s = int(x.shape[0]), int(x.shape[1])
        if b * s > self.max_rows:
            raise ValueError(f"{b} x {s} rows exceed max_rows={self.max_rows}")
        eng = self._engine
        xd = eng._dev(x, torch.float32)
        out = torch.empty((b * s, self.num_actions), dtype=torch.float32, device=eng.device)
        eng._check(self._lib.pa_backbone_windows(eng._h, _ptr(xd), b * s, _ptr(self._feats), eng._stream()))
        rc = self._lib.pa_lstm_forward(self._h, _ptr(self._feats), _lib.PA_FEATURE_STRIDE, b, s, _ptr(out), eng._stream())
        if rc != 0:
            raise EngineError(rc, self._lib.pa_lstm_last_error(self._h).decode())
        if x.is_cuda:
            return out  # (enqueued only: should the per-layer kernel's barrier ever give up, these rows are NaN; check() says why)
        res = out.cpu()  # synchronises
        self.check()
        return res

    def check(self):
        """After the stream of a ``forward`` has been synchronised: raises if the per-layer LSTM kernel's grid barrier
        timed out in that call (``pa_lstm_last_status``)."""
        rc = self._lib.pa_lstm_last_status(self._h)
        if rc != 0:
            raise EngineError(rc, self._lib.pa_lstm_last_error(self._h).decode())

    __call__ = forward

    # -- scoring (rnn_action_detector.py:132-160) -----------------------------------
    def _split_metrics(self) -> SplitMetrics:
        if getattr(self, "_metrics", None) is None:
            self._metrics = SplitMetrics(self.num_actions, self._engine.device)
        return self._metrics

    def _score(self, split: str, batch):
        input, char_label, action_label, _ = batch
        batch_size, seq_length = input.shape[0], input.shape[1]
        action_label = action_label.reshape(batch_size * seq_length)
        logp = self.forward(self._engine._dev(input, torch.float32))  # a device input: the rows stay on the device, nothing waits
        self._split_metrics().step(split, logp, action_label)

    def validation_step(self, batch, batch_idx):
        self._score("val", batch)

    def test_step(self, batch, batch_idx):
        self._score("test", batch)

    def metrics(self, split: str = "val"):
        """The epoch's figures so far (``metrics.finish``) plus ``<split>_action_loss`` / ``<split>_action_acc``; waits."""
        out = self._split_metrics().metrics(split)
        self.check()  # (the read synchronised the stream: a barrier time-out of any step's LSTM kernel shows here)
        return out

    def reset_metrics(self, split: str = None):
        self._split_metrics().reset(split)
