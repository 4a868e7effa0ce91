"""Training of ``ResnetTransformerDetector``'s transformer-encoder head on the device (``pa_encoder_train_*``,
csrc/encoder_train.hip).

The reference trains the whole model (``playaid/models/resnet_transformer_detector.py:143-164, 207-209``: ``training_step``
scores every row of the ``[B, S, A]`` output against ``action_label`` flattened to ``B * S`` rows with ``F.nll_loss``, in train
mode -- the encoder layers' ``dropout=0.1`` is part of the step --; ``configure_optimizers`` is
``torch.optim.Adam(lr=self.learning_rate)``). This package trains the head with the ResNet-50 frozen: ``resnet_ffn``, every
transformer layer and the classifier, on feature rows the backbone has already computed. ``EncoderTrainer`` updates the
``pa_encoder`` handle's weights IN PLACE, where ``pa_encoder_forward`` reads them, so ``model(x)`` sees every step at once; the
two Adam moments and the saved activations belong to the trainer.

The dropout masks are this project's own counter-based function (``include/playaid_hip.h``, next to
``pa_encoder_trainer_create``), not torch's generator; ``dropout_keep`` is its numpy twin.

Nothing here waits for the device except ``epoch_stats()`` (one read) and whatever the caller does with the tensors it is
handed. Like the rest of the product path there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .trainer_base import IGNORE, AdamTrainer, check_adam, check_labels  # noqa: F401  (IGNORE: part of this module's interface)

MAX_WINDOWS = 64   # windows (the attention's sequence) of one step, at most (``pa_encoder_trainer_max_windows`` of a large handle)
_LAYER_KEYS = ("self_attn.in_proj_weight", "self_attn.in_proj_bias", "self_attn.out_proj.weight", "self_attn.out_proj.bias",
               "linear1.weight", "linear1.bias", "linear2.weight", "linear2.bias", "norm1.weight", "norm1.bias", "norm2.weight",
               "norm2.bias")


def tensor_keys(layers: int) -> Tuple[str, ...]:
    """PyTorch keys of the trained tensors in blob order."""
    keys = ["model.resnet_ffn.weight", "model.resnet_ffn.bias"]
    for l in range(layers):
        keys += [f"model.transformer.layers.{l}.{k}" for k in _LAYER_KEYS]
    return tuple(keys) + ("model.classifier.weight", "model.classifier.bias")


TENSOR_KEYS = tensor_keys(3)   # the served model's


def tensor_shapes(in_dim: int, hidden: int, enc_dim: int, layers: int, ff: int, actions: int) -> Tuple[Tuple[int, ...], ...]:
    """PyTorch shapes of the trained tensors, in blob order (``tensor_keys(layers)``)."""
    d = hidden + enc_dim
    shapes = [(hidden, in_dim), (hidden,)]
    for _ in range(layers):
        shapes += [(3 * d, d), (3 * d,), (d, d), (d,), (ff, d), (ff,), (d, ff), (d,), (d,), (d,), (d,), (d,)]
    return tuple(shapes) + ((actions, d), (actions,))


def tensor_floats(in_dim: int, hidden: int, enc_dim: int, layers: int, ff: int, actions: int) -> int:
    return sum(int(np.prod(s)) for s in tensor_shapes(in_dim, hidden, enc_dim, layers, ff, actions))


def check_dropout(dropout: float):
    if not (isinstance(dropout, (int, float)) and math.isfinite(dropout) and 0.0 <= dropout < 1.0):
        raise ValueError(f"dropout must be in [0, 1), got {dropout!r}")


def _mix(x: np.ndarray) -> np.ndarray:
    x = x ^ (x >> np.uint32(16))
    x = x * np.uint32(0x7FEB352D)
    x = x ^ (x >> np.uint32(15))
    x = x * np.uint32(0x846CA68B)
    return x ^ (x >> np.uint32(16))


def dropout_keep(seed: int, step: int, layer: int, site: int, count: int, p: float) -> np.ndarray:
    """The numpy twin of the kernels' ``keep(seed, step, layer, site, i)`` for ``i`` in ``[0, count)`` -> ``bool[count]``
    (``include/playaid_hip.h``). ``site``: 0 the attention probabilities ``[batch * heads][L][L]``, 1 the attention block's
    output ``[rows][D]``, 2 the feed-forward activation ``[rows][ff]``, 3 the feed-forward output ``[rows][D]``; ``step`` is the
    trainer's step count before the call; ``p`` the trainer's ``dropout`` (rounded to float32 as the handle holds it). Kept
    elements are scaled by ``float32(1) / (float32(1) - float32(p))``."""
    check_dropout(p)
    thr = int(float(np.float32(p)) * 4294967296.0)
    if thr == 0:
        return np.ones(int(count), dtype=bool)
    seed, step = int(seed) & (2 ** 64 - 1), int(step) & (2 ** 64 - 1)
    with np.errstate(over="ignore"):
        one = lambda v: np.array([v & 0xFFFFFFFF], dtype=np.uint32)
        key = _mix(one(seed) + np.uint32(0x9E3779B9))
        key = _mix(key ^ one(seed >> 32))
        key = _mix(key ^ one(step))
        key = _mix(key ^ one(step >> 32))
        key = _mix(key ^ (one(layer * 4 + site + 1) * np.uint32(0x85EBCA6B)))
        i = np.arange(int(count), dtype=np.uint32)
        r = _mix(_mix(i ^ key) + key)
    return r >= np.uint32(thr)


def check_step(feats_shape, seq_len: int, batch: int, labels, in_dim: int, slots: int, actions: int, max_windows: int) -> int:
    """What ``pa_encoder_train_step`` refuses with ``PA_ERR_INVALID_ARG``, refused with a message first, and the labels as
    ``check_labels`` has them (more windows than ``max_windows`` are the C call's ``PA_ERR_CAPACITY``). -> the number of rows."""
    if int(seq_len) != seq_len or seq_len < 1:
        raise ValueError(f"seq_len must be a positive integer, got {seq_len!r}")
    if int(batch) != batch or batch != slots:
        raise ValueError(f"batch must be the model's {slots} frame slots, got {batch!r}")
    rows = int(seq_len) * int(batch)
    feats_shape = tuple(feats_shape)
    if len(feats_shape) < 2 or feats_shape[-1] < in_dim or int(np.prod(feats_shape[:-1])) != rows:
        raise ValueError(f"feats is float32[{rows} rows, >= {in_dim}], got shape {feats_shape}")
    check_labels(labels, rows, actions)
    return rows


class EncoderTrainer(AdamTrainer):
    """Adam on the encoder head of a ``ResnetTransformerDetector`` -- or of a bare ``pa_encoder`` handle (a
    ``ctypes.c_void_p``), then with ``dims=(in_dim, hidden, slots, enc_dim, heads, layers, ff, actions)`` and optionally
    ``device=`` -- (``pa_encoder_trainer_create`` / ``pa_encoder_trainer_destroy``). ``dropout`` is the encoder layers' (the
    reference's 0.1), ``seed`` that of its masks. Close the trainer before the model or handle it borrows."""

    PREFIX = "pa_encoder_trainer"

    def __init__(self, model_or_handle, lr: float = 2e-4, betas: Sequence[float] = (0.9, 0.999), eps: float = 1e-8, *,
                 dropout: float = 0.1, seed: int = 0, dims: Optional[Tuple[int, ...]] = None, device=None):
        check_adam(lr, betas, eps)
        check_dropout(dropout)
        if int(seed) != seed or not 0 <= seed < 2 ** 64:
            raise ValueError(f"seed must be an integer in [0, 2^64), got {seed!r}")
        if isinstance(model_or_handle, (C.c_void_p, int)):
            if dims is None or len(dims) != 8:
                raise ValueError("a bare pa_encoder handle needs dims=(in_dim, hidden, slots, enc_dim, heads, layers, ff, actions)")
            handle = model_or_handle if isinstance(model_or_handle, C.c_void_p) else C.c_void_p(model_or_handle)
            self.model = None
            self.device = torch.device(device if device is not None else "cuda:0")
        else:
            from .resnet_transformer_detector import FF_DIM, HIDDEN_DIM, NUM_FREQ, NUM_HEADS, NUM_LAYERS

            self.model = model_or_handle   # (kept alive: the trainer borrows its handle's weights)
            handle = model_or_handle._h
            dims = (2048, HIDDEN_DIM, model_or_handle.sequence_length, 1 + 2 * NUM_FREQ, NUM_HEADS, NUM_LAYERS, FF_DIM,
                    model_or_handle.num_actions)
            self.device = model_or_handle.device
        cfg = self._begin(lr, betas, eps)
        self.in_dim, self.hidden, self.slots, self.enc_dim, self.heads, self.layers, self.ff, self.actions = (int(d) for d in dims)
        self.dropout, self.seed = float(dropout), int(seed)
        self.keys = tensor_keys(self.layers)
        self.shapes = tensor_shapes(self.in_dim, self.hidden, self.enc_dim, self.layers, self.ff, self.actions)
        # (no trainer handle came back: the refusal's text is on the pa_encoder handle)
        self._created(self._lib.pa_encoder_trainer_create(handle, C.byref(cfg), C.c_float(self.dropout), C.c_uint64(self.seed),
                                                          C.byref(self._h)),
                      lambda: self._lib.pa_encoder_last_error(handle).decode())
        self.max_windows = int(self._lib.pa_encoder_trainer_max_windows(handle))
        if self._floats != int(self._lib.pa_encoder_trainer_floats(handle)):
            self.close()
            raise ValueError(f"dims {tuple(dims)} are not the handle's")

    # -- one step ---------------------------------------------------------------
    def _run(self, feats, seq_len, batch, labels, apply: bool, grads):
        if not isinstance(feats, torch.Tensor) or feats.dtype != torch.float32 or not feats.is_cuda or not feats.is_contiguous():
            raise ValueError("feats is a contiguous float32 device tensor [seq_len * batch rows, ld] (the ResNet-50's pooled features)")
        check_step(feats.shape, seq_len, batch, labels, self.in_dim, self.slots, self.actions, self.max_windows)
        if isinstance(labels, torch.Tensor):
            ld = labels.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        else:
            ld = torch.from_numpy(np.ascontiguousarray(labels).reshape(-1)).to(device=self.device, dtype=torch.int32)
        stats = torch.empty(4, dtype=torch.int32, device=self.device)
        self._check(self._lib.pa_encoder_train_step(self._h, C.c_void_p(feats.data_ptr()), int(feats.shape[-1]), int(seq_len), int(batch),
                                                    C.c_void_p(ld.data_ptr()), int(apply),
                                                    C.c_void_p(grads.data_ptr()) if grads is not None else C.c_void_p(0),
                                                    C.c_void_p(stats.data_ptr()), self._stream()))
        return stats

    def step(self, feats, seq_len: int, batch: int, labels) -> torch.Tensor:
        """One optimiser step on ``seq_len`` windows of ``batch`` frame slots of ``feats`` (row ``r = l * batch + n``), with one
        label per row (``-100`` = no ground truth). -> the step's ``pa_train_stats`` as a device tensor int32[4]: ``[0]`` the loss
        before the update (float32 bits: ``loss_of(stats)``), ``[1]`` labelled rows, ``[2]`` of them predicted right."""
        stats = self._run(feats, seq_len, batch, labels, True, None)
        self._count(stats)
        return stats

    def grads(self, feats, seq_len: int, batch: int, labels) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
        """The gradients of the batch's loss in PyTorch layouts (device tensors under the PyTorch keys) and the stats, under the
        dropout masks the next ``step`` will use; weights, moments and the step count stay as they are."""
        flat = torch.empty(self._floats, dtype=torch.float32, device=self.device)
        stats = self._run(feats, seq_len, batch, labels, False, flat)
        return self._split(flat), stats
