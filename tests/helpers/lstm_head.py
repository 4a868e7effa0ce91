"""Shared by tests/test_lstm_head.py and its knob child (tests/helpers/lstm_knob_worker.py): seeded weights of any
``(input_dim, H, layers, actions)``, the ``pa_lstm_create`` blob, the float64 recurrence and decoder (a generalised
``oracle.rnn.lstm_literal``, with the named faults the sensitivity test injects), and one GPU run of the C ABI on features
supplied by the test.

Bar (log-probabilities, absolute): ``BAR = 1e-5``. Derivation from the fp32 arithmetic, u = 2^-24, at the served shape
(input 300, H 512, 3 layers, 63 actions; every operand of the recurrence is bounded: |x| <= 1, |W| <= 1.5 / sqrt(H) =
0.066, |h| < 1):
  * a gate pre-activation is a length-(in + H) fp32 dot product plus two biases, summed in chains of at most 512 terms
    (the kernels split K into 4 - 64 partial sums). Its rounding error is <= gamma_K sum |w_k a_k|, gamma_K ~ K u; with
    random-sign roundings it grows as sqrt(K) u sum|.|/sqrt(K): ~ 30 * 6e-8 * 0.03 ~ 1e-7 per gate for these inputs.
  * sigmoid / tanh have slope <= 1 and expf / tanhf are within a few ulp, so h(t), c(t) carry ~1e-7. The recurrence is
    contracting for these weights (a relative input perturbation of 1e-7 moves no log-probability by more than 5e-8 in
    float64), so the error of a long sequence stays at the single-step level instead of growing with the step count:
    the 520-step case checks that.
  * decoder: Linear(H, 128) + ReLU, Linear(128, A), |w2| <= 4 sqrt(3 / 128) = 0.61: a logit is a 128-term sum whose
    rounding is ~ sqrt(128) u |logit| ~ 1e-6 at |logit| <= 15; an error of 1e-7 in h reaches the logits scaled by
    |w2| |w1| sqrt(128 H) / 3 ~ 5, i.e. 5e-7. log_softmax subtracts the max and a log-sum-exp of <= 64 terms: a few
    ulp of |logit| <= 15, <= 4e-6 (1 ulp at 8..16 is 9.5e-7).
  Total ~5e-6 in the worst row (measured on an MI355X: 1.1e-6 at most, every case and form); BAR = 1e-5 is 10x tighter than the end-to-end bar of 1e-4. It has to be this tight for
  the weakest named fault (one hidden unit's four W_hh rows rounded to bf16: 2.5e-5 at most on these inputs, from unit
  250 of the top layer) to stand 3x above it.
"""
from __future__ import annotations

import ctypes as C
import math
from typing import Dict, Optional

import numpy as np

BAR = 1e-5
BF16_UNIT = (2, 250)  # (layer, unit) whose bf16-rounded recurrent rows move the served case most (CPU search)
LD = 1024            # floats per feature row, as the mirror's PA_FEATURE_STRIDE
W_SCALE = 1.5        # recurrent / input weights ~ U(+-W_SCALE / sqrt(H)): torch's init x 1.5, so that one rounded row shows


def make_weights(input_dim: int, hidden: int, layers: int, actions: int, seed: int) -> Dict[str, np.ndarray]:
    rng = np.random.default_rng([seed, input_dim, hidden, layers, actions])
    k = W_SCALE / math.sqrt(hidden)
    w: Dict[str, np.ndarray] = {}

    def u(shape, a):
        return rng.uniform(-a, a, shape).astype(np.float32)

    for l in range(layers):
        in_l = input_dim if l == 0 else hidden
        w[f"w_ih{l}"] = u((4 * hidden, in_l), k)
        w[f"w_hh{l}"] = u((4 * hidden, hidden), k)
        w[f"b_ih{l}"] = u((4 * hidden,), k)
        w[f"b_hh{l}"] = u((4 * hidden,), k)
    w["w1"] = u((128, hidden), math.sqrt(3.0 / hidden))
    w["b1"] = u((128,), 0.05)
    w["w2"] = u((actions, 128), 4.0 * math.sqrt(3.0 / 128))
    w["b2"] = u((actions,), 0.5)
    return w


def pack_blob(w: Dict[str, np.ndarray], input_dim: int, hidden: int, layers: int, actions: int) -> np.ndarray:
    from playaid_core_amd import _lib

    hdr = np.array([_lib.PA_LSTM_MAGIC, 1, input_dim, hidden, layers, actions, 0, 0], np.int32)
    parts = [hdr.view(np.uint8)]
    for l in range(layers):
        for key in ("w_ih", "w_hh", "b_ih", "b_hh"):
            parts.append(np.ascontiguousarray(w[f"{key}{l}"], np.float32).reshape(-1).view(np.uint8))
    for key in ("w1", "b1", "w2", "b2"):
        parts.append(np.ascontiguousarray(w[key], np.float32).reshape(-1).view(np.uint8))
    return np.concatenate(parts)


def make_features(seq_len: int, batch: int, input_dim: int, seed: int) -> np.ndarray:
    """float32[seq_len, batch, LD]: U(-1, 1) in the first input_dim columns, NaN after them (a read past input_dim poisons
    the row)."""
    rng = np.random.default_rng([seed, seq_len, batch, input_dim])
    x = np.full((seq_len, batch, LD), np.nan, np.float32)
    x[..., :input_dim] = rng.uniform(-1.0, 1.0, (seq_len, batch, input_dim)).astype(np.float32)
    return x


def rne_bf16(a):
    m, e = np.frexp(np.asarray(a, np.float64))
    return np.ldexp(np.round(np.ldexp(m, 8)), e - 8)


def _sig(v):
    return 1.0 / (1.0 + np.exp(-v))


def lstm_ref(x: np.ndarray, w: Dict[str, np.ndarray], layers: int, fault: Optional[dict] = None, c0=None):
    """x [L, N, in] -> (top-layer h float64[L, N, H], final c per layer). Plain loops (torch's gate order i, f, g, o, as
    oracle.rnn.lstm_literal). fault (sensitivity tests only): {"stale": (layer, t)} step t of that layer reads h(t-2)
    instead of h(t-1); {"bf16_unit": (layer, j)} the four W_hh rows (i, f, g, o) of hidden unit j rounded to bf16;
    {"swap_fg": True}; {"no_bhh": True}. c0: per-layer initial c (default zero)."""
    fault = fault or {}
    x = np.asarray(x, np.float64)
    H = w["w_hh0"].shape[1]
    finals = []
    for l in range(layers):
        w_ih = w[f"w_ih{l}"].astype(np.float64)
        w_hh = w[f"w_hh{l}"].astype(np.float64)
        if fault.get("bf16_unit") and fault["bf16_unit"][0] == l:
            w_hh = w_hh.copy()
            j = fault["bf16_unit"][1]
            w_hh[j::H] = rne_bf16(w_hh[j::H])
        b = w[f"b_ih{l}"].astype(np.float64) + (0.0 if fault.get("no_bhh") else w[f"b_hh{l}"].astype(np.float64))
        pre = x @ w_ih.T + b
        h = np.zeros((x.shape[1], H))
        c = np.zeros((x.shape[1], H)) if c0 is None else np.array(c0[l], np.float64)
        hs = []
        for t in range(x.shape[0]):
            hp = h
            if fault.get("stale") == (l, t) and t >= 2:
                hp = hs[t - 2]
            g = pre[t] + hp @ w_hh.T
            i, f, gg, o = _sig(g[:, :H]), _sig(g[:, H:2 * H]), np.tanh(g[:, 2 * H:3 * H]), _sig(g[:, 3 * H:])
            if fault.get("swap_fg"):
                f, gg = _sig(g[:, 2 * H:3 * H]), np.tanh(g[:, H:2 * H])
            c = f * c + i * gg
            h = o * np.tanh(c)
            hs.append(h)
        finals.append(c)
        x = np.stack(hs)
    return x, finals


def decode_ref(h: np.ndarray, w: Dict[str, np.ndarray]) -> np.ndarray:
    """top-layer h [L, N, H] -> log-probabilities float64[L * N, A]."""
    y = h.reshape(-1, h.shape[-1])
    y = np.maximum(y @ w["w1"].astype(np.float64).T + w["b1"], 0.0)
    y = y @ w["w2"].astype(np.float64).T + w["b2"]
    y = y - y.max(1, keepdims=True)
    return y - np.log(np.exp(y).sum(1, keepdims=True))


def reference(x: np.ndarray, w, input_dim: int, layers: int, **kw) -> np.ndarray:
    h, _ = lstm_ref(x[..., :input_dim], w, layers, **kw)
    return decode_ref(h, w)


def ratio(got, ref) -> float:
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / BAR)


class Head:
    """One ``pa_lstm`` handle driven through the C ABI on device features."""

    def __init__(self, input_dim, hidden, layers, actions, max_rows, w):
        from playaid_core_amd import _lib

        self.lib = _lib.load()
        self.layers, self.actions = layers, actions
        blob = pack_blob(w, input_dim, hidden, layers, actions)
        assert blob.nbytes == self.lib.pa_lstm_blob_bytes(input_dim, hidden, layers, actions)
        self.h = C.c_void_p()
        rc = self.lib.pa_lstm_create(0, input_dim, hidden, layers, actions, max_rows, blob.ctypes.data_as(C.c_void_p), blob.nbytes,
                                     C.byref(self.h))
        if rc != 0:
            msg = self.lib.pa_lstm_last_error(self.h).decode() if self.h else "bad argument"
            self.close()
            raise RuntimeError(f"pa_lstm_create: {rc} {msg}")

    def forward(self, x: np.ndarray) -> np.ndarray:
        import torch

        from playaid_core_amd.engine import _ptr

        seq, batch, ld = x.shape
        xd = torch.from_numpy(np.ascontiguousarray(x)).cuda()
        out = torch.full((seq * batch, self.actions), float("nan"), dtype=torch.float32, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = self.lib.pa_lstm_forward(self.h, _ptr(xd), ld, seq, batch, _ptr(out), stream)
        assert rc == 0, self.lib.pa_lstm_last_error(self.h).decode()
        torch.cuda.synchronize()
        assert self.lib.pa_lstm_last_status(self.h) == 0, self.lib.pa_lstm_last_error(self.h).decode()
        return out.cpu().numpy()

    def forms(self):
        from playaid_core_amd import _lib

        f = (C.c_int32 * self.layers)()
        assert self.lib.pa_lstm_layer_forms(self.h, f, self.layers) == 0
        return [_lib.LSTM_FORMS[v] for v in f]

    def close(self):
        if self.h:
            self.lib.pa_lstm_destroy(self.h)
            self.h = None


# (name, input_dim, H, layers, actions, seq_len, batch); forms at the default knobs on an MI355X
CASES = {
    "served 64x7": (300, 512, 3, 63, 64, 7),
    "1 window": (300, 512, 3, 63, 1, 7),
    "batch 1": (300, 512, 3, 63, 24, 1),
    "batch 16": (300, 512, 3, 63, 8, 16),
    "520 steps": (300, 512, 3, 63, 520, 1),
    "rows 63": (300, 512, 3, 63, 9, 7),
    "rows 64": (300, 512, 3, 63, 16, 4),
    "rows 65": (300, 512, 3, 63, 13, 5),
    "input 512": (512, 512, 3, 63, 10, 7),
    "H 200": (300, 200, 3, 63, 12, 7),
    "H 8": (300, 8, 2, 63, 10, 7),
    "1 layer": (300, 512, 1, 63, 10, 7),
    "5 layers": (300, 512, 5, 63, 10, 7),
    "1 action": (300, 512, 3, 1, 10, 7),
    "64 actions": (300, 512, 3, 64, 10, 7),
}


def run_case(name: str, seed: int = 77):
    """-> (worst ratio to BAR, forms, logp). Asserts the bar."""
    input_dim, hidden, layers, actions, seq, batch = CASES[name]
    w = make_weights(input_dim, hidden, layers, actions, seed)
    x = make_features(seq, batch, input_dim, seed + 1)
    head = Head(input_dim, hidden, layers, actions, seq * batch, w)
    try:
        got = head.forward(x)
        forms = head.forms()
    finally:
        head.close()
    ref = reference(x, w, input_dim, layers)
    r = ratio(got, ref)
    assert np.isfinite(got).all() and r <= 1.0, f"{name}: max |dlogp| = {r:.3g} x the {BAR:g} bar (forms {forms})"
    return r, forms, got
