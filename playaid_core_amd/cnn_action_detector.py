"""``CNNActionDetector`` -- the operator boundary (b1 in SURVEY.md section 8b).

Mirror of ``playaid/models/cnn_action_detector.py:46-92`` for inference:
``load_from_checkpoint(path, actions=[...])``, ``.eval()``, ``model(x)`` with
``x: float32[B,S,3,128,128]`` in [0,1] -> ``float32[B,len(actions)]``
log-probabilities, ``.actions``. The arithmetic (ResNet-18 per frame, Conv1d
over the S features, MLP, log_softmax) runs in the HIP library through
``pa_infer_windows``; there is no PyTorch fallback.

Scoring is mirrored too (it is inference): ``validation_step`` / ``test_step``
(``:131-163``) score the window's CENTRE label -- NLL loss and multiclass top-1
accuracy -- into a device accumulator (``metrics.EvalState``, ``pa_eval_*``)
without reading anything back per step; ``metrics("val" | "test")`` is the one
read and returns the figures under the reference's log names
(``val_action_loss``, ``val_action_acc``, ...) plus the confusion matrix and
mean confidence of ``visualizations/cnn_action_detector_vis.py:89-153``;
``reset_metrics(split)`` starts a new epoch.

Training is mirrored for the temporal head with the encoder frozen (``freeze_encoder=True``; ``head_trainer.HeadTrainer``,
csrc/head_train.hip): ``train()``, ``configure_optimizers()`` (the reference's ``torch.optim.Adam(lr=self.learning_rate)``,
``:165-167``, as a device trainer), ``training_step`` (``:94-116``: centre label, NLL loss; the ResNet-18 features come from the
existing inference kernels, eval-mode BatchNorm), ``state_dict()`` and ``save_checkpoint()``. The head's weights are updated
in place where inference reads them. Not mirrored: training the encoder (``train()`` with ``freeze_encoder=False`` raises
``NotImplementedError``), ``training_epoch_end`` and the data hooks (``:118-129,169-207``).
"""
from __future__ import annotations

from typing import List, Mapping, Optional

import torch

from .engine import Engine
from .metrics import SplitMetrics
from .weights import infer_geometry


class CNNActionDetector:
    def __init__(
        self,
        actions: List[str],
        batch_size: int = 64,
        sequence_length: int = 4,
        learning_rate: float = 2e-4,
        num_samples: int = 1024,
        freeze_encoder=False,
        state_dict: Optional[Mapping] = None,
        device: str = "cuda:0",
        **kwargs,
    ):
        if state_dict is None:
            raise ValueError(
                "CNNActionDetector needs weights: use load_from_checkpoint() or pass state_dict= "
                "(the reference's resnet18(pretrained=True) download is not available offline)"
            )
        s, a = infer_geometry(state_dict)
        if a != len(actions):
            raise ValueError(f"checkpoint has {a} action logits but {len(actions)} actions were given")
        self.actions = list(actions)
        self.num_actions = len(self.actions)
        self.sequence_length = s
        self.batch_size = batch_size
        self.learning_rate = learning_rate
        self.num_samples = num_samples
        self.dataset_kwargs = kwargs
        self.freeze_encoder = bool(freeze_encoder)
        self.training = False
        self._state_dict = state_dict
        self._trainer = None
        # (beyond the reference's arguments: the engine's capacities and, never by default, the arithmetic of the fp32 path --
        # compute_dtype="emulated_f32", PA_DTYPE_EMULATED_F32)
        self._engine = Engine(state_dict, device=device, **{k: v for k, v in kwargs.items() if k.startswith("max_") or k == "compute_dtype"})

    @classmethod
    def load_from_checkpoint(cls, checkpoint_path: str, map_location=None, **kwargs):
        """Lightning-1.6.5 ``.ckpt``: ``state_dict`` (keys ``model.cnn2d.*``,
        ``model.cnn1d.0.*``, ``model.classifier.{0,2}.*``) plus
        ``hyper_parameters``; keyword arguments override the saved ones like
        ``LightningModule.load_from_checkpoint`` (``ai_runner.py:164-167``)."""
        ckpt = torch.load(checkpoint_path, map_location="cpu", weights_only=False)
        if "state_dict" not in ckpt:
            raise KeyError(f"{checkpoint_path} has no 'state_dict' (not a Lightning checkpoint)")
        hparams = dict(ckpt.get("hyper_parameters", {}) or {})
        hparams.update(kwargs)
        if "actions" not in hparams:
            raise TypeError("load_from_checkpoint() missing 'actions' (ai_runner.py:166 passes list(MOVE_TO_CLASS_ID))")
        return cls(state_dict=ckpt["state_dict"], **hparams)

    # -- nn.Module-like surface -------------------------------------------------
    def eval(self):
        self.training = False
        return self

    def train(self, mode: bool = True):
        if mode and not self.freeze_encoder:
            raise NotImplementedError("training is out of scope for the MI355X inference path "
                                      "(only the temporal head trains: build the model with freeze_encoder=True)")
        self.training = bool(mode)
        return self

    # -- training of the head (cnn_action_detector.py:94-116, 165-167; encoder frozen) ------------
    def configure_optimizers(self):
        """The reference's ``torch.optim.Adam(self.parameters(), lr=self.learning_rate)`` for the head's six tensors, as a
        ``HeadTrainer`` on this model's engine (made once; it owns the Adam moments and the running epoch statistics)."""
        if not self.freeze_encoder:
            raise NotImplementedError("only the temporal head trains: build the model with freeze_encoder=True")
        if self._trainer is None:
            from .head_trainer import MAX_BATCH, HeadTrainer

            self._trainer = HeadTrainer(self._engine, lr=self.learning_rate, max_batch=MAX_BATCH)
        return self._trainer

    def training_step(self, batch, batch_idx):
        """One optimiser step on ``batch = (input[B,S,3,128,128], char_label, action_label[B,S], meta)``: the centre label of
        every window (``-100`` = none), the ResNet-18 features of its crops (``pa_backbone_windows``), one ``pa_head_train_step``.
        -> the loss before the update as a 0-dim device tensor; nothing is read back."""
        if not self.training:
            raise RuntimeError("training_step needs train() (and freeze_encoder=True)")
        input, char_label, action_label, _ = batch
        eng = self._engine
        if input.dim() != 5 or input.shape[1] != eng.S or tuple(input.shape[2:]) != (3, 128, 128):
            raise ValueError(f"expected [B,{eng.S},3,128,128], got {tuple(input.shape)}")
        trainer = self.configure_optimizers()
        b, s = int(input.shape[0]), int(input.shape[1])
        labels = torch.as_tensor(action_label)[:, s // 2].to(torch.int32)
        xd = eng._dev(input, torch.float32)
        feats = torch.empty((b * s, 1024), dtype=torch.float32, device=eng.device)
        eng._check(eng._lib.pa_backbone_windows(eng._h, xd.data_ptr(), b * s, feats.data_ptr(), eng._stream()))
        gather = torch.arange(b * s, dtype=torch.int32, device=eng.device).view(b, s)
        stats = trainer.step(feats, gather, labels)
        return trainer.loss_of(stats)

    def state_dict(self):
        """The state dict the model was built from with the six head tensors as they are now (numpy; waits for the device)."""
        out = dict(self._state_dict)
        if self._trainer is not None:
            for k, v in self._trainer.read("weights").items():
                out[k] = v.cpu().numpy()
        return out

    def save_checkpoint(self, path: str):
        """Writes the Lightning-shaped ``.ckpt`` that ``load_from_checkpoint`` reads: ``state_dict`` + ``hyper_parameters``."""
        sd = {k: torch.as_tensor(v).detach().cpu().clone() for k, v in self.state_dict().items()}
        hparams = {"batch_size": self.batch_size, "sequence_length": self.sequence_length, "learning_rate": self.learning_rate,
                   "num_samples": self.num_samples, "freeze_encoder": self.freeze_encoder}
        torch.save({"state_dict": sd, "hyper_parameters": hparams, "pytorch-lightning_version": "1.6.5", "epoch": 0,
                    "global_step": int(self._trainer.steps) if self._trainer is not None else 0}, path)

    @property
    def engine(self) -> Engine:
        return self._engine

    def forward(self, x: torch.Tensor) -> torch.Tensor:
        """x [batch, frames_per_sequence, channel, height, width] -> log-probabilities."""
        out = self._engine.infer_windows(x)
        return out if x.is_cuda else out.cpu()

    __call__ = forward

    # -- scoring (cnn_action_detector.py:131-163) ---------------------------------
    def _split_metrics(self) -> SplitMetrics:
        if getattr(self, "_metrics", None) is None:
            self._metrics = SplitMetrics(self.num_actions, self._engine.device)
        return self._metrics

    def _score(self, split: str, batch):
        input, char_label, action_label, _ = batch
        centered_action_label = action_label[:, input.shape[1] // 2]
        logp = self._engine.infer_windows(input)  # stays on the device: nothing is read back per step
        self._split_metrics().step(split, logp, centered_action_label)

    def validation_step(self, batch, batch_idx):
        self._score("val", batch)

    def test_step(self, batch, batch_idx):
        self._score("test", batch)

    def metrics(self, split: str = "val"):
        """The epoch's figures so far (``metrics.finish``) plus ``<split>_action_loss`` / ``<split>_action_acc``; waits."""
        return self._split_metrics().metrics(split)

    def reset_metrics(self, split: str = None):
        self._split_metrics().reset(split)
