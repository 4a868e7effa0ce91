"""Scoring on the device: NLL loss, top-1 accuracy, confusion matrix, mean confidence (``pa_eval_*``, csrc/metrics.hip).

What the reference computes in ``validation_step`` / ``test_step`` (``playaid/models/cnn_action_detector.py:131-163``:
``F.nll_loss`` and a torchmetrics multiclass ``Accuracy``) and in ``visualizations/cnn_action_detector_vis.py:89-153``
(row-normalised confusion matrix, "% correct", "mean confidence"). ``EvalState`` accumulates on the device over any
number of ``update`` calls without waiting for any of them; ``totals()`` is the one read. Finishing the figures
(``finish``) and adding the parts of several states (``merge``) are host arithmetic in float64 on the totals.

Like the rest of the product path there is no CPU fallback: ``EvalState`` needs the HIP library and a device.
"""
from __future__ import annotations

import ctypes as C
from typing import Dict, Iterable, Optional, Tuple

import numpy as np
import torch

from . import _lib

IGNORE = _lib.PA_EVAL_IGNORE
TOTAL_FIELDS = ("rows", "correct", "ignored", "bad_labels", "nll_sum", "conf_sum")


class BadLabelsError(ValueError):
    """Labels outside ``[0, num_actions)`` (other than ``IGNORE``) were met; ``totals`` / ``confusion`` hold what was read."""

    def __init__(self, totals: Dict, confusion: np.ndarray):
        super().__init__(f"{totals['bad_labels']} labels outside [0, {confusion.shape[0]}) were skipped "
                         f"({_lib.PA_ERR_BAD_LABELS}: use {IGNORE} for rows without ground truth)")
        self.totals = totals
        self.confusion = confusion


def _totals_dict(t) -> Dict:
    if isinstance(t, dict):
        return {k: t[k] for k in TOTAL_FIELDS}
    return {k: getattr(t, k) for k in TOTAL_FIELDS}


def finish(totals, confusion) -> Dict:
    """The finished figures from raw totals (a ``pa_eval_totals`` or a dict of its fields) and ``confusion`` int64[A, A]
    (row = actual, column = predicted). Pure float64 host arithmetic; ``rows == 0`` gives NaN, not an exception."""
    t = _totals_dict(totals)
    cm = np.asarray(confusion, dtype=np.int64)
    rows = int(t["rows"])
    nan = float("nan")
    sums = cm.sum(axis=1)
    norm = np.zeros(cm.shape, dtype=np.float64)
    has = sums > 0
    norm[has] = cm[has].astype(np.float64) / sums[has, None].astype(np.float64)   # sklearn normalize="true"; an empty row stays 0
    per_class = np.where(has, np.diagonal(norm), np.nan)
    return {
        "loss": float(t["nll_sum"]) / rows if rows else nan,                    # F.nll_loss(reduction="mean") over the scored rows
        "accuracy": int(t["correct"]) / rows if rows else nan,                   # Accuracy(task="multiclass"): micro, top-1
        "mean_confidence": 100.0 * float(t["conf_sum"]) / rows if rows else nan,  # cnn_action_detector_vis.py:111,148
        "confusion": cm,
        "confusion_normalized": norm,
        "per_class_accuracy": per_class,
        "rows": rows,
        "ignored": int(t["ignored"]),
    }


def merge(parts: Iterable[Tuple[object, np.ndarray]]) -> Tuple[Dict, np.ndarray]:
    """Element-wise sum of ``(totals, confusion)`` parts -> ``(totals dict, confusion)``: the clip score of a
    frame-parallel run from its ranks' parts. The double sums are added in list order."""
    parts = list(parts)
    if not parts:
        raise ValueError("merge: no parts")
    out = {k: (0.0 if k.endswith("_sum") else 0) for k in TOTAL_FIELDS}
    cm = None
    for t, c in parts:
        t = _totals_dict(t)
        for k in TOTAL_FIELDS:
            out[k] = out[k] + (float(t[k]) if k.endswith("_sum") else int(t[k]))
        c = np.asarray(c, dtype=np.int64)
        if cm is None:
            cm = c.copy()
        elif c.shape != cm.shape:
            raise ValueError(f"merge: confusion matrices of {cm.shape} and {c.shape}")
        else:
            cm = cm + c
    return out, cm


class EvalState:
    """One accumulator on one device (``pa_eval_create`` / ``pa_eval_destroy``); usable as a context manager."""

    def __init__(self, num_actions: int, device="cuda:0"):
        self._h = C.c_void_p(0)
        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no HIP device visible to PyTorch-ROCm; this path has no CPU fallback")
        self.device = torch.device(device)
        if self.device.index is None:
            self.device = torch.device(self.device.type, torch.cuda.current_device())
        self.num_actions = int(num_actions)
        rc = self._lib.pa_eval_create(self.device.index or 0, self.num_actions, C.byref(self._h))
        if rc != _lib.PA_OK:
            self.close()
            self._fail(rc, "pa_eval_create")

    def _fail(self, rc: int, what: str):
        from .engine import EngineError

        raise EngineError(rc, f"{what}: {self._lib.pa_status_string(rc).decode()}")

    def _stream(self):
        return C.c_void_p(torch.cuda.current_stream(self.device).cuda_stream)

    def close(self):
        if getattr(self, "_h", None):
            self._lib.pa_eval_destroy(self._h)
            self._h = C.c_void_p(0)

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def reset(self):
        rc = self._lib.pa_eval_reset(self._h, self._stream())
        if rc != _lib.PA_OK:
            self._fail(rc, "pa_eval_reset")

    def update(self, logp: torch.Tensor, labels: torch.Tensor, label_stride: int = 1):
        """logp float32[n, >= A] (device, rows contiguous; a row pitch above A is taken from the stride), labels int32 device:
        row i is scored against ``labels.view(-1)[i * label_stride]``. Enqueued on the current stream, nothing is waited for.
        ``label_stride=4`` with ``records[..., 1:]`` flattened = a ``pa_record`` array's ``action_id`` (``Engine.agreement``)."""
        if logp.dim() != 2 or logp.dtype != torch.float32 or logp.device != self.device or (logp.numel() > 0 and logp.stride(1) != 1):
            raise ValueError(f"update: logp is a float32[n, A] tensor on {self.device} with contiguous rows")
        n = int(logp.shape[0])
        ld = int(logp.stride(0)) if n > 1 else int(logp.shape[1])
        if logp.shape[1] < self.num_actions or ld < self.num_actions:
            raise ValueError(f"update: logp rows hold {logp.shape[1]} values, the state scores {self.num_actions} actions")
        if labels.dtype != torch.int32 or labels.device != self.device or not labels.is_contiguous():
            raise ValueError(f"update: labels is a contiguous int32 tensor on {self.device}")
        if label_stride < 1 or (n > 0 and labels.numel() < (n - 1) * label_stride + 1):
            raise ValueError(f"update: {labels.numel()} labels at stride {label_stride} for {n} rows")
        if n == 0:
            return
        rc = self._lib.pa_eval_update(self._h, C.c_void_p(logp.data_ptr()), ld, n, C.c_void_p(labels.data_ptr()), int(label_stride),
                                      self._stream())
        if rc != _lib.PA_OK:
            self._fail(rc, "pa_eval_update")

    def totals(self, strict: bool = True):
        """The one read (waits for the stream) -> ``(pa_eval_totals, confusion int64[A, A])``. Labels outside the range raise
        ``BadLabelsError`` (``PA_ERR_BAD_LABELS``; the error carries what was read), unless ``strict=False``."""
        t = _lib.pa_eval_totals()
        cm = np.zeros((self.num_actions, self.num_actions), dtype=np.int64)
        rc = self._lib.pa_eval_read(self._h, C.byref(t), cm.ctypes.data_as(C.c_void_p), self._stream())
        if rc == _lib.PA_ERR_BAD_LABELS:
            if strict:
                raise BadLabelsError(_totals_dict(t), cm)
        elif rc != _lib.PA_OK:
            self._fail(rc, "pa_eval_read")
        return t, cm

    def compute(self, strict: bool = True) -> Dict:
        return finish(*self.totals(strict=strict))


class SplitMetrics:
    """The lazily created ``"val"`` / ``"test"`` states behind a model's ``validation_step`` / ``test_step`` /
    ``metrics`` / ``reset_metrics`` (shared by the three detector mirrors)."""

    SPLITS = ("val", "test")

    def __init__(self, num_actions: int, device):
        self.num_actions = num_actions
        self.device = device
        self._states: Dict[str, EvalState] = {}

    def state(self, split: str) -> EvalState:
        if split not in self.SPLITS:
            raise ValueError(f"split is one of {self.SPLITS}")
        if split not in self._states:
            self._states[split] = EvalState(self.num_actions, self.device)
        return self._states[split]

    def step(self, split: str, logp: torch.Tensor, labels: torch.Tensor):
        """``logp`` [rows, A] on the device (as the model enqueued it), ``labels`` [rows] of any integer type, anywhere."""
        st = self.state(split)
        st.update(logp.reshape(-1, logp.shape[-1]), labels.reshape(-1).to(device=st.device, dtype=torch.int32).contiguous())

    def metrics(self, split: str) -> Dict:
        out = self.state(split).compute()
        out[f"{split}_action_loss"] = out["loss"]   # the reference's log names (cnn_action_detector.py:145-146,162-163)
        out[f"{split}_action_acc"] = out["accuracy"]
        return out

    def reset(self, split: Optional[str] = None):
        for s in ([split] if split is not None else list(self._states)):
            if s not in self.SPLITS:
                raise ValueError(f"split is one of {self.SPLITS}")
            if s in self._states:
                self._states[s].reset()

    def close(self):
        for st in self._states.values():
            st.close()
        self._states = {}
