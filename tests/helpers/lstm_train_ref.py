"""Reference for the LSTM trainer (tests/test_lstm_train*.py): the reference model's recurrent head -- ``nn.LSTM(in, H, layers)``
fed ``[T, N, in]`` without ``batch_first`` (T windows are the time steps, N frames the batch, zero initial state),
``Linear(H, 128)`` + ReLU, ``Linear(128, A)``, ``F.log_softmax``, ``F.nll_loss(ignore_index=-100)`` over every row
(``playaid/models/rnn_action_detector.py:57-65, 97-117``) -- with torch autograd and ``torch.optim.Adam`` (``:162-164``) on the
CPU, in float64 (the reference) or float32 (the yardstick of what fp32 arithmetic costs against it). Weights and features come
from tests/helpers/lstm_head.py; inputs are seeded and shared by the tests; nothing here is changed by a test.
"""
import numpy as np
import torch
import torch.nn.functional as F
from torch import nn

from . import lstm_head as LH
from .adam_ref import adam_step_f64  # noqa: F401  (the tests reach it through this module)

IGNORE = -100
ROW_TOL = 2e-5    # fp32 rows against float64, relative to the tensor's largest entry (tests/test_head_train.py)
LOGP_TOL = 1e-4   # log-probabilities, hence the loss

SERVED = (300, 512, 3, 63)
SMALL = (21, 32, 2, 5)
ONE_LAYER = (33, 64, 1, 3)
STEPS = [(1, 7), (8, 4), (5, 16), (9, 1), (37, 7)]
# (dims, (T, N)): every (T, N) on the served dimensions, a subset on the small ones
CASES = [(SERVED, tn) for tn in STEPS] + [(SMALL, (8, 4)), (SMALL, (9, 1)), (SMALL, (37, 7)), (ONE_LAYER, (5, 16)), (ONE_LAYER, (1, 7))]


def case_id(case):
    (i, h, l, a), (t, n) = case
    return f"in{i}-H{h}-L{l}-A{a}-T{t}-N{n}"


def keys(layers):
    out = []
    for l in range(layers):
        out += [f"lstm.weight_ih_l{l}", f"lstm.weight_hh_l{l}", f"lstm.bias_ih_l{l}", f"lstm.bias_hh_l{l}"]
    return tuple(out) + ("action_decoder.0.weight", "action_decoder.0.bias", "action_decoder.2.weight", "action_decoder.2.bias")


def blob_order(w, layers):
    """The weights of ``lstm_head.make_weights`` as a list in blob order (``keys(layers)``)."""
    out = []
    for l in range(layers):
        out += [w[f"w_ih{l}"], w[f"w_hh{l}"], w[f"b_ih{l}"], w[f"b_hh{l}"]]
    return out + [w["w1"], w["b1"], w["w2"], w["b2"]]


def from_blob_order(tensors, layers):
    """The inverse: a list in blob order -> the dictionary ``lstm_head.pack_blob`` takes."""
    w, it = {}, iter(tensors)
    for l in range(layers):
        for key in ("w_ih", "w_hh", "b_ih", "b_hh"):
            w[f"{key}{l}"] = np.asarray(next(it), np.float32)
    for key in ("w1", "b1", "w2", "b2"):
        w[key] = np.asarray(next(it), np.float32)
    return w


class Net(nn.Module):
    def __init__(self, dims, w, dtype=torch.float64):
        super().__init__()
        input_dim, hidden, layers, actions = dims
        self.layers = layers
        self.lstm = nn.LSTM(input_dim, hidden, num_layers=layers)
        self.action_decoder = nn.Sequential(nn.Linear(hidden, 128), nn.ReLU(), nn.Linear(128, actions))
        self.to(dtype)
        with torch.no_grad():
            for p, a in zip(self.ordered(), blob_order(w, layers)):
                assert tuple(p.shape) == tuple(a.shape)
                p.copy_(torch.as_tensor(np.asarray(a), dtype=dtype))

    def ordered(self):
        """Parameters in blob order."""
        named = dict(self.named_parameters())
        return [named[k] for k in keys(self.layers)]

    def forward(self, x):
        """x [T, N, in] -> log-probabilities [T * N, A]."""
        h, _ = self.lstm(x)
        return F.log_softmax(self.action_decoder(h.reshape(-1, h.shape[-1])), dim=1)

    def loss(self, x, labels):
        labels = torch.as_tensor(np.asarray(labels), dtype=torch.long).reshape(-1)
        logp = self(x)
        if not bool((labels != IGNORE).any()):
            return logp.sum() * 0.0   # the stated departure: no labelled row -> loss 0, gradients 0 (torch: NaN)
        return F.nll_loss(logp, labels, ignore_index=IGNORE)


def _x(x, dims, dtype):
    return torch.as_tensor(np.asarray(x)[..., :dims[0]], dtype=dtype)


def make_labels(T, N, A, seed):
    """int32[T * N]: random classes; with T * N > 4 every fifth row has no ground truth."""
    rng = np.random.default_rng([seed, T, N, A])
    labels = rng.integers(0, A, size=T * N).astype(np.int32)
    if T * N > 4:
        labels[::5] = IGNORE
    return labels


def make_case(case, seed=31):
    """-> (weights dict, x float32[T, N, LD] with NaN past input_dim, labels int32[T * N])."""
    dims, (T, N) = case
    return LH.make_weights(*dims, seed), LH.make_features(T, N, dims[0], seed + 1), make_labels(T, N, dims[3], seed + 2)


def loss_and_grads(dims, w, x, labels, dtype=torch.float64):
    """-> (loss float, [gradients in blob order as numpy arrays of ``dtype``], log-probabilities as numpy)."""
    net = Net(dims, w, dtype)
    xs = _x(x, dims, dtype)
    loss = net.loss(xs, labels)
    grads = torch.autograd.grad(loss, net.ordered())
    with torch.no_grad():
        logp = net(xs).numpy()
    return float(loss.detach()), [g.numpy() for g in grads], logp


def train(dims, w, batches, lr, dtype=torch.float64, betas=(0.9, 0.999), eps=1e-8):
    """``torch.optim.Adam`` over ``batches`` = [(x, labels), ...] -> (losses before each step, [parameters in blob order after
    each step as numpy])."""
    net = Net(dims, w, dtype)
    opt = torch.optim.Adam(net.ordered(), lr=lr, betas=betas, eps=eps)
    losses, traj = [], []
    for x, labels in batches:
        opt.zero_grad()
        loss = net.loss(_x(x, dims, dtype), labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        traj.append([p.detach().numpy().copy() for p in net.ordered()])
    return losses, traj


TOY_LR = 1e-2


def toy_problem(seed=13, T=8, N=4):
    """The trajectory test's separable problem on SMALL: row (t, n) is 0.6 * prototype of class (t + n) % A + 0.2 * noise,
    clipped to [-1, 1], labelled with its class. -> (weights, x float32[T, N, LD], labels int32[T * N])."""
    input_dim, _, _, A = SMALL
    rng = np.random.default_rng(seed)
    protos = rng.uniform(-1.0, 1.0, (A, input_dim))
    cls = (np.arange(T)[:, None] + np.arange(N)[None, :]) % A
    x = np.full((T, N, LH.LD), np.nan, np.float32)
    x[..., :input_dim] = np.clip(0.6 * protos[cls] + 0.2 * rng.standard_normal((T, N, input_dim)), -1.0, 1.0).astype(np.float32)
    return LH.make_weights(*SMALL, seed), x, cls.reshape(-1).astype(np.int32)
