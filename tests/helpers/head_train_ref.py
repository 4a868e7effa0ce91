"""Reference for the head trainer (tests/test_head_train*.py): the reference model's temporal head --
``nn.Conv1d(1000, 512, kernel_size=S)`` + ReLU, ``Linear(512, 128)`` + ReLU, ``Linear(128, A)``, ``F.log_softmax``,
``F.nll_loss(ignore_index=-100)`` on the centre labels (``playaid/models/cnn_action_detector.py:22-27, 94-116``) -- with torch
autograd and ``torch.optim.Adam`` (``:165-167``) on the CPU, in float64 (the reference) or float32 (the yardstick of what fp32
arithmetic costs against it). Inputs are seeded and shared by the tests; nothing here is changed by a test.
"""
import numpy as np
import torch
import torch.nn.functional as F

from playaid_core_amd import synth

from .adam_ref import adam_step_f64  # noqa: F401  (the tests reach it through this module)

KEYS = ("model.cnn1d.0.weight", "model.cnn1d.0.bias", "model.classifier.0.weight", "model.classifier.0.bias",
        "model.classifier.2.weight", "model.classifier.2.bias")
IGNORE = -100


def head_params(state_dict, dtype=torch.float64, requires_grad=True):
    """The six head tensors of a state dict as fresh leaf tensors, in ``KEYS`` order."""
    return [torch.tensor(np.asarray(state_dict[k]), dtype=dtype).clone().requires_grad_(requires_grad) for k in KEYS]


def make_feats(n_rows, seed):
    """float32[n_rows, 1024]: 0.5 * max(N(0, 1), -0.5) in the 1000 used columns (mostly positive like ReLU-fed fc outputs, with
    a negative floor so that signs matter), zeros in the padding."""
    g = torch.Generator().manual_seed(seed)
    f = torch.zeros(n_rows, 1024, dtype=torch.float32)
    f[:, :1000] = 0.5 * torch.clamp(torch.randn(n_rows, 1000, generator=g), min=-0.5)
    return f


def make_batch(n_rows, B, S, A, seed):
    """(gather int32[B, S], labels int32[B]): random rows with repeats; window 0 uses ONE row in all its slots; with B > 4 every
    fifth label is -100."""
    rng = np.random.default_rng(seed)
    gather = rng.integers(0, n_rows, size=(B, S)).astype(np.int32)
    gather[0, :] = gather[0, 0]
    if B > 1:
        gather[1, -1] = gather[1, 0]   # a repeated row inside a window
    labels = rng.integers(0, A, size=B).astype(np.int32)
    if B > 4:
        labels[::5] = IGNORE
    return gather, labels


def forward(params, feats, gather):
    """-> log-probabilities [B, A]; feats [n_rows, >= 1000], gather [B, S]."""
    w1, b1, w2, b2, w3, b3 = params
    x = feats[:, :1000].to(w1.dtype)[torch.as_tensor(np.asarray(gather), dtype=torch.long)]   # [B, S, 1000]
    h1 = torch.relu(F.conv1d(x.permute(0, 2, 1), w1, b1)).flatten(1)                       # [B, 512]
    h2 = torch.relu(F.linear(h1, w2, b2))
    return F.log_softmax(F.linear(h2, w3, b3), dim=1)


def loss_of(params, feats, gather, labels):
    labels = torch.as_tensor(np.asarray(labels), dtype=torch.long)
    logp = forward(params, feats, gather)
    if not bool((labels != IGNORE).any()):
        return logp.sum() * 0.0   # the stated departure: no labelled window -> loss 0, gradients 0 (torch: NaN)
    return F.nll_loss(logp, labels, ignore_index=IGNORE)


def loss_and_grads(state_dict, feats, gather, labels, dtype=torch.float64):
    """-> (loss float, [six gradients as numpy arrays of ``dtype``])."""
    params = head_params(state_dict, dtype)
    loss = loss_of(params, feats, gather, labels)
    grads = torch.autograd.grad(loss, params)
    return float(loss.detach()), [g.numpy() for g in grads]


def train(state_dict, batches, lr, dtype=torch.float64, betas=(0.9, 0.999), eps=1e-8):
    """``torch.optim.Adam`` over ``batches`` = [(feats, gather, labels), ...] -> (losses before each step, [parameters after
    each step as numpy])."""
    params = head_params(state_dict, dtype)
    opt = torch.optim.Adam(params, lr=lr, betas=betas, eps=eps)
    losses, traj = [], []
    for feats, gather, labels in batches:
        opt.zero_grad()
        loss = loss_of(params, feats, gather, labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        traj.append([p.detach().numpy().copy() for p in params])
    return losses, traj


def toy_problem(A=5, S=3, B=32, seed=11):
    """The trajectory test's separable problem, laid out as a one-fighter clip of B + 1 frames so that the engine's own head
    (``features_import`` + ``head_frames``, frame_delta 1) sees the same windows: row r is 0.5 * max(prototype of class r % A +
    0.5 * noise, 0); window b is the runner's sample around frame b + 1 and is labelled with its centre row's class.
    -> (state_dict, feats float32[B + 1, 1024], gather int32[B, S], labels int32[B])."""
    from playaid_core_amd.dataset_utils import action_sample_from_frame_middle_out

    g = torch.Generator().manual_seed(seed)
    n = B + 1
    protos = torch.randn(A, 1000, generator=g)
    cls = torch.arange(n) % A
    feats = torch.zeros(n, 1024, dtype=torch.float32)
    feats[:, :1000] = 0.5 * torch.clamp(protos[cls] + 0.5 * torch.randn(n, 1000, generator=g), min=0.0)
    gather = np.array([action_sample_from_frame_middle_out(f, S, 1, n, min_frame=1) for f in range(1, n)], dtype=np.int32) - 1
    labels = (gather[:, S // 2] % A).astype(np.int32)
    sd = synth.make_state_dict(seed=77, num_actions=A, sequence_length=S)
    return sd, feats, gather, labels
