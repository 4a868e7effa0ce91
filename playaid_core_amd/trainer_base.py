"""What the device trainers share on the Python side (``head_trainer.HeadTrainer``, ``lstm_trainer.LSTMTrainer``): the checks
of Adam's hyper-parameters and of a batch's labels, and ``AdamTrainer``, which owns a ``pa_*_trainer`` handle -- its creation's
failure path, errors, stream, life time, step count, the read-out of the tensor sets and the running epoch statistics. A
subclass names its C symbols (``PREFIX``), sets ``self.keys`` / ``self.shapes`` and keeps what differs: its inputs, ``_run``,
``step`` and ``grads``.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Callable, Dict, Optional, Sequence

import numpy as np
import torch

from . import _lib

IGNORE = _lib.PA_EVAL_IGNORE
_WHICH = {"weights": _lib.PA_TRAIN_WEIGHTS, "m": _lib.PA_TRAIN_M, "v": _lib.PA_TRAIN_V}


def check_adam(lr: float, betas: Sequence[float], eps: float):
    """What every ``pa_*_trainer_create`` refuses in its ``pa_adam_config``, refused with a message first."""
    if not (math.isfinite(lr) and lr > 0):
        raise ValueError(f"lr must be finite and positive, got {lr!r}")
    if not (math.isfinite(eps) and eps > 0):
        raise ValueError(f"eps must be finite and positive, got {eps!r}")
    if len(betas) != 2 or not all(0.0 <= b < 1.0 for b in betas):
        raise ValueError(f"betas must be two values in [0, 1), got {betas!r}")


def check_labels(labels, count: int, actions: int):
    """``count`` integer labels and, where they are host data (numpy arrays, lists, CPU tensors), their values:
    ``{-100} | [0, actions)``. Device tensors are checked for size and type only -- reading them would wait for the device; the
    kernels ignore labels outside the range."""
    if isinstance(labels, torch.Tensor):
        host = None if labels.is_cuda else labels.numpy()
        n, integral = labels.numel(), not (labels.is_floating_point() or labels.is_complex() or labels.dtype == torch.bool)
    else:
        host = np.asarray(labels)
        n, integral = host.size, np.issubdtype(host.dtype, np.integer)
    if n != count:
        raise ValueError(f"labels are int32[{count}], got {n} values")
    if not integral:
        raise ValueError(f"labels must be integers, got {labels.dtype if hasattr(labels, 'dtype') else host.dtype}")
    if host is not None and not np.all((host == IGNORE) | ((host >= 0) & (host < actions))):
        raise ValueError(f"labels must be {IGNORE} or in [0, {actions})")


class AdamTrainer:
    PREFIX = ""   # of the C symbols: PREFIX_create, _destroy, _last_error, _steps, _read

    def _c(self, name: str):
        return getattr(self._lib, f"{self.PREFIX}_{name}")

    def _begin(self, lr: float, betas: Sequence[float], eps: float):
        """Before ``PREFIX_create``: the library, a null handle for its result, the hyper-parameters -> the ``pa_adam_config``."""
        self._h = C.c_void_p(0)
        self._lib = _lib.load()
        self.lr, self.betas, self.eps = float(lr), (float(betas[0]), float(betas[1])), float(eps)
        return _lib.pa_adam_config(self.lr, self.betas[0], self.betas[1], self.eps)

    def _created(self, rc: int, no_handle_error: Optional[Callable[[], str]] = None):
        """After ``PREFIX_create`` (``self.keys`` / ``self.shapes`` set). A creation that failed raises with the trainer's own
        error text where a handle came back (and destroys it), else with ``no_handle_error()`` or, where that is missing or
        empty, the status string."""
        if rc != _lib.PA_OK:
            if self._h:
                msg = self._c("last_error")(self._h).decode()
            else:
                msg = (no_handle_error() if no_handle_error else "") or self._lib.pa_status_string(rc).decode()
            self.close()
            self._raise(rc, msg)
        self._floats = sum(int(np.prod(s)) for s in self.shapes)
        # running epoch statistics on the device: sum of loss * valid, valid, correct (float64, exact for the counts)
        self._epoch = torch.zeros(3, dtype=torch.float64, device=self.device)

    @staticmethod
    def _raise(rc: int, msg: str):
        from .engine import EngineError

        raise EngineError(rc, msg)

    def _check(self, rc: int):
        if rc != _lib.PA_OK:
            self._raise(rc, self._c("last_error")(self._h).decode())

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None):
            self._c("destroy")(self._h)
            self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @property
    def steps(self) -> int:
        return int(self._c("steps")(self._h))

    @staticmethod
    def loss_of(stats: torch.Tensor) -> torch.Tensor:
        """The loss of a ``step`` / ``grads`` result as a 0-dim float32 device tensor (no read)."""
        return stats[:1].view(torch.float32)[0]

    def _split(self, flat: torch.Tensor) -> Dict[str, torch.Tensor]:
        out, off = {}, 0
        for key, shape in zip(self.keys, self.shapes):
            n = int(np.prod(shape))
            out[key] = flat[off:off + n].view(shape)
            off += n
        return out

    def read(self, which: str = "weights") -> Dict[str, torch.Tensor]:
        """``"weights"`` | ``"m"`` | ``"v"`` -> the trained tensors in PyTorch layouts (device tensors under ``self.keys``)."""
        if which not in _WHICH:
            raise ValueError(f"which must be one of {sorted(_WHICH)}")
        flat = torch.empty(self._floats, dtype=torch.float32, device=self.device)
        self._check(self._c("read")(self._h, _WHICH[which], C.c_void_p(flat.data_ptr()), self._floats, self._stream()))
        return self._split(flat)

    # -- running statistics -------------------------------------------------------
    def _count(self, stats: torch.Tensor):
        """Adds an applied step's ``pa_train_stats`` to the epoch's (device arithmetic, no read)."""
        valid = stats[1].to(torch.float64)
        self._epoch += torch.stack((self.loss_of(stats).to(torch.float64) * valid, valid, stats[2].to(torch.float64)))

    def epoch_stats(self, reset: bool = True) -> Dict[str, float]:
        """Loss (mean over the labelled rows -- the head's windows -- of the steps since the last reset, each step's loss taken
        before its update) and accuracy of the epoch so far: ONE read. ``"windows"`` counts the labelled rows."""
        s = self._epoch.cpu().numpy()
        if reset:
            self._epoch.zero_()
        n = float(s[1])
        return {"loss": float(s[0]) / n if n else float("nan"), "accuracy": float(s[2]) / n if n else float("nan"), "windows": int(n)}
