"""Training of ``RNNActionDetector``'s LSTM head on the device (``pa_lstm_train_*``, csrc/lstm_train.hip).

The reference trains the whole model (``playaid/models/rnn_action_detector.py:97-117, 162-164``: ``training_step`` scores every
row of the ``[B * S, A]`` output against ``action_label.view(B * S)`` with ``F.nll_loss``; ``configure_optimizers`` is
``torch.optim.Adam(lr=self.learning_rate)``). This package trains the recurrent head with the encoder frozen (the reference's
``freeze_encoder=True``): every ``lstm.*`` tensor, ``action_decoder.0`` and ``action_decoder.2``, on feature rows the backbone has
already computed. ``LSTMTrainer`` updates the ``pa_lstm`` handle's weights IN PLACE, where ``pa_lstm_forward`` reads them, so
``model(x)`` sees every step at once; the two Adam moments and the saved activations belong to the trainer.

Nothing here waits for the device except ``epoch_stats()`` (one read) and whatever the caller does with the tensors it is
handed. Like the rest of the product path there is no CPU fallback.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib
from .trainer_base import IGNORE, AdamTrainer, check_adam, check_labels  # noqa: F401  (IGNORE: part of this module's interface)

MAX_BATCH = 16   # rows of a time step (``pa_lstm_forward``'s limit)
_DECODER_KEYS = ("action_decoder.0.weight", "action_decoder.0.bias", "action_decoder.2.weight", "action_decoder.2.bias")


def tensor_keys(layers: int) -> Tuple[str, ...]:
    """PyTorch keys of the trained tensors in blob order."""
    keys = []
    for l in range(layers):
        keys += [f"lstm.weight_ih_l{l}", f"lstm.weight_hh_l{l}", f"lstm.bias_ih_l{l}", f"lstm.bias_hh_l{l}"]
    return tuple(keys) + _DECODER_KEYS


TENSOR_KEYS = tensor_keys(3)   # the served model's


def tensor_shapes(input_dim: int, hidden: int, layers: int, actions: int) -> Tuple[Tuple[int, ...], ...]:
    """PyTorch shapes of the trained tensors, in blob order (``tensor_keys(layers)``)."""
    shapes = []
    for l in range(layers):
        shapes += [(4 * hidden, input_dim if l == 0 else hidden), (4 * hidden, hidden), (4 * hidden,), (4 * hidden,)]
    return tuple(shapes) + ((128, hidden), (128,), (actions, 128), (actions,))


def tensor_floats(input_dim: int, hidden: int, layers: int, actions: int) -> int:
    return sum(int(np.prod(s)) for s in tensor_shapes(input_dim, hidden, layers, actions))


def check_step(x_shape, seq_len: int, batch: int, labels, input_dim: int, actions: int, max_rows: int) -> int:
    """What ``pa_lstm_train_step`` refuses, refused with a message first, and the labels as ``check_labels`` has them. -> the
    number of rows."""
    if int(seq_len) != seq_len or seq_len < 1:
        raise ValueError(f"seq_len must be a positive integer, got {seq_len!r}")
    if int(batch) != batch or not 1 <= batch <= MAX_BATCH:
        raise ValueError(f"batch must be an integer in 1..{MAX_BATCH}, got {batch!r}")
    rows = int(seq_len) * int(batch)
    if rows > max_rows:
        raise ValueError(f"{seq_len} x {batch} rows exceed max_rows={max_rows}")
    x_shape = tuple(x_shape)
    if len(x_shape) < 2 or x_shape[-1] < input_dim or int(np.prod(x_shape[:-1])) != rows:
        raise ValueError(f"x is float32[{rows} rows, >= {input_dim}], got shape {x_shape}")
    check_labels(labels, rows, actions)
    return rows


class LSTMTrainer(AdamTrainer):
    """Adam on the LSTM head of an ``RNNActionDetector`` -- or of a bare ``pa_lstm`` handle (a ``ctypes.c_void_p``), then with
    ``dims=(input_dim, hidden, layers, actions)``, ``max_rows=`` and optionally ``device=`` -- (``pa_lstm_trainer_create`` /
    ``pa_lstm_trainer_destroy``). Close the trainer before the model or handle it borrows."""

    PREFIX = "pa_lstm_trainer"

    def __init__(self, model_or_handle, lr: float = 2e-4, betas: Sequence[float] = (0.9, 0.999), eps: float = 1e-8, *,
                 dims: Optional[Tuple[int, int, int, int]] = None, max_rows: Optional[int] = None, device=None):
        check_adam(lr, betas, eps)
        cfg = self._begin(lr, betas, eps)
        if isinstance(model_or_handle, (C.c_void_p, int)):
            if dims is None or max_rows is None:
                raise ValueError("a bare pa_lstm handle needs dims=(input_dim, hidden, layers, actions) and max_rows=")
            handle = model_or_handle if isinstance(model_or_handle, C.c_void_p) else C.c_void_p(model_or_handle)
            self.model = None
            self.device = torch.device(device if device is not None else "cuda:0")
        else:
            from .rnn_action_detector import HIDDEN_DIM, INPUT_DIM, NUM_LAYERS

            self.model = model_or_handle   # (kept alive: the trainer borrows its handle's weights)
            handle = model_or_handle._h
            dims = (INPUT_DIM, HIDDEN_DIM, NUM_LAYERS, model_or_handle.num_actions)
            max_rows = model_or_handle.max_rows
            self.device = model_or_handle._engine.device
        self.input_dim, self.hidden, self.layers, self.actions = (int(d) for d in dims)
        self.max_rows = int(max_rows)
        self.keys = tensor_keys(self.layers)
        self.shapes = tensor_shapes(*dims)
        # (no trainer handle came back: the refusal's text is on the pa_lstm handle)
        self._created(self._lib.pa_lstm_trainer_create(handle, C.byref(cfg), C.byref(self._h)),
                      lambda: self._lib.pa_lstm_last_error(handle).decode())
        if self._floats != int(self._lib.pa_lstm_trainer_floats(handle)):
            self.close()
            raise ValueError(f"dims {tuple(dims)} are not the handle's")

    # -- one step ---------------------------------------------------------------
    def _run(self, x, seq_len, batch, labels, apply: bool, grads):
        if not isinstance(x, torch.Tensor) or x.dtype != torch.float32 or not x.is_cuda or not x.is_contiguous():
            raise ValueError("x is a contiguous float32 device tensor [seq_len * batch rows, ld] (pa_backbone_windows rows)")
        check_step(x.shape, seq_len, batch, labels, self.input_dim, self.actions, self.max_rows)
        if isinstance(labels, torch.Tensor):
            ld = labels.to(device=self.device, dtype=torch.int32).reshape(-1).contiguous()
        else:
            ld = torch.from_numpy(np.ascontiguousarray(labels).reshape(-1)).to(device=self.device, dtype=torch.int32)
        stats = torch.empty(4, dtype=torch.int32, device=self.device)
        self._check(self._lib.pa_lstm_train_step(self._h, C.c_void_p(x.data_ptr()), int(x.shape[-1]), int(seq_len), int(batch),
                                                 C.c_void_p(ld.data_ptr()), int(apply),
                                                 C.c_void_p(grads.data_ptr()) if grads is not None else C.c_void_p(0),
                                                 C.c_void_p(stats.data_ptr()), self._stream()))
        return stats

    def step(self, x, seq_len: int, batch: int, labels) -> torch.Tensor:
        """One optimiser step on ``seq_len`` time steps (windows) of ``batch`` rows (frames) of ``x``, with one label per row
        (``-100`` = no ground truth). -> the step's ``pa_train_stats`` as a device tensor int32[4]: ``[0]`` the loss before the
        update (float32 bits: ``loss_of(stats)``), ``[1]`` labelled rows, ``[2]`` of them predicted right."""
        stats = self._run(x, seq_len, batch, labels, True, None)
        self._count(stats)
        return stats

    def grads(self, x, seq_len: int, batch: int, labels) -> Tuple[Dict[str, torch.Tensor], torch.Tensor]:
        """The gradients of the batch's loss in PyTorch layouts (device tensors under the PyTorch keys) and the stats; weights,
        moments and the step count stay as they are."""
        flat = torch.empty(self._floats, dtype=torch.float32, device=self.device)
        stats = self._run(x, seq_len, batch, labels, False, flat)
        return self._split(flat), stats
