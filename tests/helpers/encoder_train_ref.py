"""Reference for the encoder trainer (tests/test_encoder_train*.py): the head of the reference's ``ResnetTransformerDetector``
(``playaid/models/resnet_transformer_detector.py:25-93, 136-164``) written out with torch ops -- ``F.linear``, softmax,
``F.layer_norm`` and mask multiplies -- under autograd, so that the dropout masks are inputs: Linear(in, hidden), the time
encoding appended, post-norm encoder layers over [L windows, N slots, D] (no ``batch_first``: attention mixes the same slot of
different windows), Linear(D, A), ``log_softmax``, ``F.nll_loss(ignore_index=-100)`` over every row; ``torch.optim.Adam``. On the
CPU, in float64 (the reference) or float32 (the yardstick of what fp32 arithmetic costs against it).

Weights are tests/test_encoder_head.py's ``make_weights`` (the inference tests' scaling), features U(0, 1) with NaN behind
them. ``make_case`` clears the ReLU kinks (see KINK). Cases are cached and shared by the tests; nothing here is changed by a
test.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

import test_encoder_head as EH

from .adam_ref import adam_step_f64  # noqa: F401  (the tests reach it through this module)

IGNORE = -100
ROW_TOL = 2e-5    # fp32 rows against float64, relative to the tensor's largest entry (tests/test_head_train.py)
LOGP_TOL = 1e-4   # log-probabilities, hence the loss
# A feed-forward pre-activation within fp32 error of zero flips its ReLU derivative between two correct fp32 evaluations: a
# condition of the inputs, not an error of either. KINK = 100 x the fp32 error of those 256-term sums (~1e-6 at |z| ~ 1).
KINK = 1e-4
PAD = EH.PAD

# (in, hidden, slots, enc, heads, layers, ff, A)
SERVED = (2048, 247, 7, 9, 8, 3, 2048, 63)
SMALL = (96, 55, 3, 9, 2, 2, 128, 5)
ONE_LAYER = (64, 64, 4, 0, 2, 1, 64, 3)
CASES = [(SERVED, L) for L in (1, 8, 37, 64)] + [(SMALL, L) for L in (1, 9, 64)] + [(ONE_LAYER, L) for L in (5, 16)]
DROPOUT_CASES = [(SMALL, 9, 0.1), (SMALL, 9, 0.5), (SERVED, 8, 0.1)]
LAYER_KEYS = ("in_w", "in_b", "out_w", "out_b", "l1_w", "l1_b", "l2_w", "l2_b", "n1_g", "n1_b", "n2_g", "n2_b")
NAMES = {"SERVED": SERVED, "SMALL": SMALL, "ONE_LAYER": ONE_LAYER}


def case_id(case):
    dims, L = case[0], case[1]
    name = next(k for k, v in NAMES.items() if v == dims)
    return f"{name}-L{L}" + (f"-p{case[2]}" if len(case) > 2 else "")


def keys(layers):
    """The trained tensors in blob order, under ``make_weights``' names."""
    out = ["ffn_w", "ffn_b"]
    for l in range(layers):
        out += [f"{l}.{k}" for k in LAYER_KEYS]
    return tuple(out) + ("cls_w", "cls_b")


def blob_order(w, layers):
    return [w[k] for k in keys(layers)]


def from_blob_order(tensors, layers, enc):
    """The inverse: a list in blob order (+ the encoding) -> the dictionary ``test_encoder_head.pack_blob`` takes."""
    w = {k: np.asarray(a, np.float32) for k, a in zip(keys(layers), tensors)}
    w["enc"] = np.asarray(enc, np.float32)
    return w


def mask_shapes(dims, L):
    """(layer, site) -> the shape of the site's mask in torch's layout (``include/playaid_hip.h``)."""
    _, hidden, N, enc, heads, layers, ff, _ = dims
    D = hidden + enc
    out = {}
    for l in range(layers):
        out[(l, 0)] = (N * heads, L, L)
        out[(l, 1)] = (L * N, D)
        out[(l, 2)] = (L * N, ff)
        out[(l, 3)] = (L * N, D)
    return out


def make_masks(dims, L, p, seed=0, step=0):
    """The trainer's masks for (seed, step), scaled as the kernels scale them: float64 arrays, or None at p = 0."""
    if p == 0:
        return None
    from playaid_core_amd.encoder_trainer import dropout_keep

    scale = float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))
    return {(l, s): dropout_keep(seed, step, l, s, int(np.prod(shape)), p).reshape(shape).astype(np.float64) * scale
            for (l, s), shape in mask_shapes(dims, L).items()}


# ---- the head, written out ------------------------------------------------------------------------------------------------------
def _mask(y, masks, l, site, fault):
    if masks is None:
        return y
    k = torch.as_tensor(masks[(l, site)], dtype=y.dtype).reshape(y.shape)
    if fault == "mask_fwd_only":
        return y + (y * k - y).detach()
    return y * k


def attn_block(x, P, l, dims, masks, fault=None):
    """x [L, N, D] -> the layer's x1 = LN1(x + dropout1(out_proj(attention)))."""
    N, heads = dims[2], dims[4]
    L, D = x.shape[0], x.shape[2]
    hd = D // heads
    qkv = F.linear(x, P[f"{l}.in_w"], P[f"{l}.in_b"])
    q, k, v = (qkv[..., i * D:(i + 1) * D].reshape(L, N, heads, hd) for i in range(3))
    scale = 1.0 if fault == "noscale" else 1.0 / math.sqrt(hd)
    if fault == "slots":
        s = torch.einsum("lihd,ljhd->lhij", q, k) * scale
        o = torch.einsum("lhij,ljhd->lihd", torch.softmax(s, -1), v).reshape(L, N, D)
    else:
        s = torch.einsum("inhd,jnhd->nhij", q, k) * scale            # [N, heads, L, L]
        p = torch.softmax(s, -1).reshape(N * heads, L, L)
        p = _mask(p, masks, l, 0, fault).reshape(N, heads, L, L)
        o = torch.einsum("nhij,jnhd->inhd", p, v).reshape(L, N, D)
    y = F.linear(o, P[f"{l}.out_w"], P[f"{l}.out_b"])
    eps = 1e-6 if fault == "eps" else 1e-5
    if fault == "residual_first":
        r = _mask((x + y).reshape(L * N, D), masks, l, 1, None).reshape(L, N, D)
    else:
        r = x + _mask(y.reshape(L * N, D), masks, l, 1, fault).reshape(L, N, D)
    return F.layer_norm(r, (D,), P[f"{l}.n1_g"], P[f"{l}.n1_b"], eps)


def ff_block(x1, P, l, dims, masks, fault=None):
    """x1 [L, N, D] -> (the layer's output LN2(x1 + dropout3(linear2(dropout2(relu(z1))))), z1 [L * N, ff])."""
    L, N, D = x1.shape
    z1 = F.linear(x1, P[f"{l}.l1_w"], P[f"{l}.l1_b"]).reshape(L * N, -1)
    f = _mask(torch.relu(z1), masks, l, 2, fault)
    y = F.linear(f, P[f"{l}.l2_w"], P[f"{l}.l2_b"])
    eps = 1e-6 if fault == "eps" else 1e-5
    r = x1 + _mask(y, masks, l, 3, fault).reshape(L, N, D)
    return F.layer_norm(r, (D,), P[f"{l}.n2_g"], P[f"{l}.n2_b"], eps), z1


def front(x, P, enc):
    """x [L, N, in] -> [L, N, D]: the projection with the slot's encoding appended."""
    h = F.linear(x, P["ffn_w"], P["ffn_b"])
    L, N = h.shape[0], h.shape[1]
    return torch.cat([h, enc.to(h.dtype)[None].expand(L, N, enc.shape[1])], dim=2)


def forward(x, P, enc, dims, masks=None, fault=None):
    """-> (log-probabilities [L * N, A], [z1 of every layer])."""
    h = front(x, P, enc)
    z1s = []
    for l in range(dims[5]):
        h, z1 = ff_block(attn_block(h, P, l, dims, masks, fault), P, l, dims, masks, fault)
        z1s.append(z1)
    return F.log_softmax(F.linear(h.reshape(-1, h.shape[-1]), P["cls_w"], P["cls_b"]), dim=1), z1s


def nll(logp, labels):
    labels = torch.as_tensor(np.asarray(labels), dtype=torch.long).reshape(-1)
    if not bool((labels != IGNORE).any()):
        return logp.sum() * 0.0   # the stated departure: no labelled row -> loss 0, gradients 0 (torch: NaN)
    return F.nll_loss(logp, labels, ignore_index=IGNORE)


def params(w, layers, dtype, grad=True):
    return {k: torch.tensor(np.asarray(w[k]), dtype=dtype, requires_grad=grad) for k in keys(layers)}


def _x(x, dims, dtype):
    return torch.as_tensor(np.asarray(x)[..., :dims[0]], dtype=dtype)


def loss_and_grads(dims, w, x, labels, masks=None, dtype=torch.float64, fault=None):
    """-> (loss float, [gradients in blob order as numpy arrays of ``dtype``], log-probabilities numpy, min |z1| over the layers)."""
    P = params(w, dims[5], dtype)
    logp, z1s = forward(_x(x, dims, dtype), P, torch.as_tensor(np.asarray(w["enc"])), dims, masks, fault)
    loss = nll(logp, labels)
    grads = torch.autograd.grad(loss, [P[k] for k in keys(dims[5])])
    return float(loss.detach()), [g.numpy() for g in grads], logp.detach().numpy(), min(float(z.detach().abs().min()) for z in z1s)


def make_labels(L, N, A, seed):
    """int32[L * N]: random classes; with more than four rows every fifth row has no ground truth."""
    rng = np.random.default_rng([seed, L, N, A])
    labels = rng.integers(0, A, size=L * N).astype(np.int32)
    if L * N > 4:
        labels[::5] = IGNORE
    return labels


def clear_kinks(dims, w, x, masks):
    """Layer by layer, in float64, with the masks applied: moves ``linear1.bias[j]`` by a multiple of 3 KINK until every row
    has |z1[r][j]| >= KINK. Changes ``w`` in place. -> the number of biases moved."""
    moved = 0
    enc = torch.as_tensor(np.asarray(w["enc"]))
    with torch.no_grad():
        h = None
        for l in range(dims[5]):
            P = params(w, dims[5], torch.float64, grad=False)
            h = front(_x(x, dims, torch.float64), P, enc) if l == 0 else h
            x1 = attn_block(h, P, l, dims, masks)
            z1 = ff_block(x1, P, l, dims, masks)[1].numpy()
            bias = np.asarray(w[f"{l}.l1_b"], np.float64).copy()
            for j in np.nonzero(np.abs(z1).min(0) < 1.01 * KINK)[0]:
                for m in (i * s for i in range(1, 1000) for s in (1, -1)):
                    if np.abs(z1[:, j] + m * 3 * KINK).min() >= 1.01 * KINK:
                        bias[j] += m * 3 * KINK
                        moved += 1
                        break
                else:
                    raise AssertionError("no shift clears the unit")
            w[f"{l}.l1_b"] = bias.astype(np.float32)
            P = params(w, dims[5], torch.float64, grad=False)
            h = ff_block(x1, P, l, dims, masks)[0]
    return moved


@functools.lru_cache(maxsize=None)
def make_case(dims, L, p=0.0, seed=31, mask_seed=0, step=0):
    """-> (weights dict with the kinks cleared, x float32[L, N, in + PAD] with NaN past in, labels int32[L * N], masks or None,
    biases moved). Cached: the tests share it and leave it unchanged."""
    in_dim, hidden, N, enc, heads, layers, ff, A = dims
    w = EH.make_weights(in_dim, hidden, N, enc, layers, ff, A, seed)
    x = EH.make_features(L, N, in_dim, seed + 1)
    masks = make_masks(dims, L, p, mask_seed, step)
    moved = clear_kinks(dims, w, x, masks)
    return w, x, make_labels(L, N, A, seed + 2), masks, moved


@functools.lru_cache(maxsize=None)
def reference(dims, L, p=0.0, dtype=torch.float64):
    """``loss_and_grads`` of ``make_case(dims, L, p)``, computed once per session."""
    w, x, labels, masks, _ = make_case(dims, L, p)
    return loss_and_grads(dims, w, x, labels, masks, dtype)


def train(dims, w, batches, lr, dtype=torch.float64, betas=(0.9, 0.999), eps=1e-8):
    """``torch.optim.Adam`` over ``batches`` = [(x, labels), ...] without dropout -> (losses before each step, [parameters in
    blob order after each step as numpy])."""
    P = params(w, dims[5], dtype)
    ordered = [P[k] for k in keys(dims[5])]
    enc = torch.as_tensor(np.asarray(w["enc"]))
    opt = torch.optim.Adam(ordered, lr=lr, betas=betas, eps=eps)
    losses, traj = [], []
    for x, labels in batches:
        opt.zero_grad()
        loss = nll(forward(_x(x, dims, dtype), P, enc, dims)[0], labels)
        loss.backward()
        opt.step()
        losses.append(float(loss.detach()))
        traj.append([q.detach().numpy().copy() for q in ordered])
    return losses, traj


TOY_LR = 1e-3


def toy_problem(seed=13, L=8):
    """The trajectory test's separable problem on SMALL: row (l, n) is 0.5 + 0.3 * prototype of class (l + n) % A + 0.1 * noise,
    clipped to [0, 1], labelled with its class. -> (weights, x float32[L, N, in + PAD], labels int32[L * N])."""
    in_dim, hidden, N, enc, heads, layers, ff, A = SMALL
    rng = np.random.default_rng(seed)
    protos = rng.uniform(-1.0, 1.0, (A, in_dim))
    cls = (np.arange(L)[:, None] + np.arange(N)[None, :]) % A
    x = np.full((L, N, in_dim + PAD), np.nan, np.float32)
    x[..., :in_dim] = np.clip(0.5 + 0.3 * protos[cls] + 0.1 * rng.standard_normal((L, N, in_dim)), 0.0, 1.0).astype(np.float32)
    return EH.make_weights(in_dim, hidden, N, enc, layers, ff, A, seed), x, cls.reshape(-1).astype(np.int32)
