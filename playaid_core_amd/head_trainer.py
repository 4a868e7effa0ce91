"""Training of ``CNNActionDetector``'s temporal head on the device (``pa_head_train_*``, csrc/head_train.hip).

The reference trains the whole model (``playaid/models/cnn_action_detector.py:94-116, 165-167``: ``training_step`` takes the
window's centre label, ``F.nll_loss``; ``configure_optimizers`` is ``torch.optim.Adam(lr=self.learning_rate)``). This package
trains the head with the encoder frozen (the reference's ``freeze_encoder=True``): ``cnn1d.0``, ``classifier.0`` and
``classifier.2``, on feature rows the engine has already computed. ``HeadTrainer`` updates the engine's weights IN PLACE, in
the layouts its inference kernels read, so ``model(x)``, clip lanes, captured graphs and ``weights_arena()`` see every step at
once; the two Adam moments belong to the trainer.

Nothing here waits for the device except ``epoch_stats()`` (one read) and whatever the caller does with the tensors it is
handed. Like the rest of the product path there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from . import _lib, trainer_base
from .trainer_base import _WHICH, IGNORE, AdamTrainer, check_labels  # noqa: F401  (IGNORE: part of this module's interface)

MAX_BATCH = 256
TENSOR_KEYS = ("model.cnn1d.0.weight", "model.cnn1d.0.bias", "model.classifier.0.weight", "model.classifier.0.bias",
               "model.classifier.2.weight", "model.classifier.2.bias")


def tensor_shapes(sequence_length: int, num_actions: int) -> Tuple[Tuple[int, ...], ...]:
    """PyTorch shapes of the six trained tensors, in blob order (``TENSOR_KEYS``)."""
    return ((512, 1000, sequence_length), (512,), (128, 512), (128,), (num_actions, 128), (num_actions,))


def tensor_floats(sequence_length: int, num_actions: int) -> int:
    return sum(int(np.prod(s)) for s in tensor_shapes(sequence_length, num_actions))


def check_adam(lr: float, betas: Sequence[float], eps: float, max_batch: int):
    """What ``pa_head_trainer_create`` refuses, refused with a message first."""
    trainer_base.check_adam(lr, betas, eps)
    if not 1 <= int(max_batch) <= MAX_BATCH or int(max_batch) != max_batch:
        raise ValueError(f"max_batch must be an integer in 1..{MAX_BATCH}, got {max_batch!r}")


def check_batch(gather, labels, n_rows: int, sequence_length: int, num_actions: int, max_batch: int) -> int:
    """Shapes of ``gather`` [B, S] and ``labels`` [B] and, where they are host data (numpy arrays, lists, CPU tensors), their
    values: row indices in ``[0, n_rows)``, labels as ``check_labels`` has them. Device tensors are not read -- that would wait
    for the device; the kernels clamp indices and ignore labels outside the range. -> B."""
    gs = tuple(gather.shape) if hasattr(gather, "shape") else np.asarray(gather).shape
    ls = tuple(labels.shape) if hasattr(labels, "shape") else np.asarray(labels).shape
    if len(gs) != 2 or gs[1] != sequence_length:
        raise ValueError(f"gather is int32[B, {sequence_length}], got shape {tuple(gs)}")
    b = int(gs[0])
    if not 1 <= b <= max_batch:
        raise ValueError(f"batch of {b} windows outside 1..{max_batch}")
    if tuple(ls) != (b,):
        raise ValueError(f"labels are int32[{b}], got shape {tuple(ls)}")
    if n_rows < 1:
        raise ValueError("feats has no rows")
    if isinstance(gather, torch.Tensor):
        g = None if gather.is_cuda else gather.numpy()
    else:
        g = np.asarray(gather)
    if g is not None and not np.issubdtype(g.dtype, np.integer):
        raise ValueError(f"gather must be integers, got {g.dtype}")
    if g is not None and g.size and (g.min() < 0 or g.max() >= n_rows):
        raise ValueError(f"gather indices outside [0, {n_rows})")
    check_labels(labels, b, num_actions)
    return b


class HeadTrainer(AdamTrainer):
    """Adam on the head of ``engine`` (``pa_head_trainer_create`` / ``pa_head_trainer_destroy``)."""

    PREFIX = "pa_head_trainer"

    def __init__(self, engine, lr: float = 2e-4, betas: Sequence[float] = (0.9, 0.999), eps: float = 1e-8, max_batch: int = 64):
        check_adam(lr, betas, eps, max_batch)
        cfg = self._begin(lr, betas, eps)
        self.engine = engine   # (kept alive: the trainer borrows its weights)
        self.device = engine.device
        self.S, self.A = engine.S, engine.A
        self.max_batch = int(max_batch)
        self.keys, self.shapes = TENSOR_KEYS, tensor_shapes(self.S, self.A)
        self._created(self._lib.pa_head_trainer_create(engine._h, C.byref(cfg), self.max_batch, C.byref(self._h)))

    # -- one step ---------------------------------------------------------------
    def _inputs(self, feats, gather, labels):
        if not isinstance(feats, torch.Tensor) or feats.dtype != torch.float32 or not feats.is_cuda or not feats.is_contiguous():
            raise ValueError("feats is a contiguous float32 device tensor [..., 1024] (pa_features_export / pa_backbone_windows rows)")
        if feats.shape[-1] != _lib.PA_FEATURE_STRIDE:
            raise ValueError(f"feature rows are {_lib.PA_FEATURE_STRIDE} floats wide, got {feats.shape[-1]}")
        n_rows = feats.numel() // _lib.PA_FEATURE_STRIDE
        b = check_batch(gather, labels, n_rows, self.S, self.A, self.max_batch)
        gd = self.engine._dev(gather, torch.int32)
        ld = self.engine._dev(labels, torch.int32)
        return n_rows, b, gd, ld

    def _run(self, feats, gather, labels, apply: bool, grads):
        n_rows, b, gd, ld = self._inputs(feats, gather, labels)
        stats = torch.empty(4, dtype=torch.int32, device=self.device)
        self._check(self._lib.pa_head_train_step(self._h, C.c_void_p(feats.data_ptr()), n_rows, C.c_void_p(gd.data_ptr()),
                                                 C.c_void_p(ld.data_ptr()), b, int(apply),
                                                 C.c_void_p(grads.data_ptr()) if grads is not None else C.c_void_p(0),
                                                 C.c_void_p(stats.data_ptr()), self._stream()))
        return stats

    def step(self, feats, gather, labels) -> torch.Tensor:
        """One optimiser step on windows ``gather`` int32[B, S] (rows of ``feats``) with centre labels ``labels`` int32[B]
        (``-100`` = no ground truth). -> the step's ``pa_train_stats`` as a device tensor int32[4]: ``[0]`` the loss before the
        update (float32 bits: ``stats[:1].view(torch.float32)``), ``[1]`` labelled windows, ``[2]`` of them predicted right."""
        stats = self._run(feats, gather, labels, True, None)
        self.engine._head_trained = True   # (Engine.reconfigured: the state dict the engine was built from is stale now)
        self._count(stats)
        return stats

    def grads(self, feats, gather, labels) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
        """The six gradients of the batch's loss in PyTorch layouts (device tensors under ``TENSOR_KEYS``) and the stats;
        weights, moments and the step count stay as they are."""
        flat = torch.empty(self._floats, dtype=torch.float32, device=self.device)
        stats = self._run(feats, gather, labels, False, flat)
        return self._split(flat), stats

    def read_raw(self, which: str = "weights") -> Tuple[torch.Tensor, ...]:
        """The set as it lies on the device, padding included (``PA_TRAIN_RAW``): float32 device tensors [512, S, 1024], [512],
        [512, 128] (k-major), [128], [128, 64] (k-major), [A]."""
        if which not in _WHICH:
            raise ValueError(f"which must be one of {sorted(_WHICH)}")
        shapes = ((512, self.S, _lib.PA_FEATURE_STRIDE), (512,), (512, 128), (128,), (128, 64), (self.A,))
        total = sum(int(np.prod(s)) for s in shapes)
        flat = torch.empty(total, dtype=torch.float32, device=self.device)
        self._check(self._lib.pa_head_trainer_read(self._h, _WHICH[which] | _lib.PA_TRAIN_RAW, C.c_void_p(flat.data_ptr()), total,
                                                   self._stream()))
        out, off = [], 0
        for s in shapes:
            n = int(np.prod(s))
            out.append(flat[off:off + n].view(s))
            off += n
        return tuple(out)
