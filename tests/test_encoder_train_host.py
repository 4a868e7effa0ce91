"""The encoder trainer's reference and host side, on the CPU (csrc/encoder_train.hip, ``pa_encoder_train_*``; the kernels are pinned
in tests/test_encoder_train.py on these very inputs):

1. the written-out head of tests/helpers/encoder_train_ref.py is ``nn.TransformerEncoder`` + projection + classifier (p = 0);
2. the GPU test's bars are reachable in fp32 and the ReLU kinks are gone on every case;
3. the bars are not idle: named faults move some gradient by >= 3 x ROW_TOL;
4. ``dropout_keep``: deterministic, the right share, independent streams and neighbours (binomial bounds);
5. the toy problem halves its loss;
6. the Python wrapper and the C ABI refuse bad arguments before any device call.
"""
import ctypes as C
import math
import os
import re
import sys

import numpy as np
import pytest
import torch
from torch import nn

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import encoder_train_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL_CASES = [c + (0.0,) for c in R.CASES] + R.DROPOUT_CASES


@pytest.fixture(scope="module")
def lib():
    from playaid_core_amd import _build, _lib

    _build.build()
    return _lib.load()


def _rel(got, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(got, np.float64) - ref).max() / max(np.abs(ref).max(), 1e-300))


# -- 1 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dims, L", [(R.SMALL, 9), (R.ONE_LAYER, 5), (R.SERVED, 8)], ids=["small", "one_layer", "served"])
def test_written_out_head_is_torchs_transformer_encoder(dims, L):
    in_dim, hidden, N, enc, heads, layers, ff, A = dims
    D = hidden + enc
    w, x, labels, _, _ = R.make_case(dims, L)
    loss, grads, logp, _ = R.loss_and_grads(dims, w, x, labels)
    ffn, cls = nn.Linear(in_dim, hidden), nn.Linear(D, A)
    encoder = nn.TransformerEncoder(nn.TransformerEncoderLayer(D, heads, ff, dropout=0.0), layers, enable_nested_tensor=False)
    net = nn.ModuleList([ffn, encoder, cls]).double()
    names = {"in_w": "self_attn.in_proj_weight", "in_b": "self_attn.in_proj_bias", "out_w": "self_attn.out_proj.weight",
             "out_b": "self_attn.out_proj.bias", "l1_w": "linear1.weight", "l1_b": "linear1.bias", "l2_w": "linear2.weight",
             "l2_b": "linear2.bias", "n1_g": "norm1.weight", "n1_b": "norm1.bias", "n2_g": "norm2.weight", "n2_b": "norm2.bias"}
    named = dict(net.named_parameters())
    ordered = [named["0.weight"], named["0.bias"]]
    for l in range(layers):
        ordered += [named[f"1.layers.{l}.{names[k]}"] for k in R.LAYER_KEYS]
    ordered += [named["2.weight"], named["2.bias"]]
    with torch.no_grad():
        for p, a in zip(ordered, R.blob_order(w, layers)):
            assert tuple(p.shape) == tuple(a.shape)
            p.copy_(torch.as_tensor(np.asarray(a), dtype=torch.float64))
    xs = torch.as_tensor(x[..., :in_dim], dtype=torch.float64)
    h = torch.cat([ffn(xs), torch.as_tensor(w["enc"], dtype=torch.float64)[None].expand(L, N, enc)], dim=2)
    out = torch.log_softmax(cls(encoder(h).reshape(L * N, D)), dim=1)
    ref_loss = nn.functional.nll_loss(out, torch.as_tensor(labels, dtype=torch.long), ignore_index=R.IGNORE)
    ref_grads = torch.autograd.grad(ref_loss, ordered)
    assert abs(loss - float(ref_loss.detach())) <= 1e-10
    np.testing.assert_allclose(logp, out.detach().numpy(), rtol=0, atol=1e-10)
    for k, g, rg in zip(R.keys(layers), grads, ref_grads):
        assert np.abs(g - rg.numpy()).max() <= 1e-10, k


# -- 2 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ALL_CASES, ids=R.case_id)
def test_the_gpu_bars_are_reachable_and_the_kinks_are_gone(case):
    dims, L, p = case
    w, x, labels, masks, moved = R.make_case(dims, L, p)
    loss, grads, _, zmin = R.reference(dims, L, p)
    assert zmin >= R.KINK, f"min |z1| = {zmin:.3g}"
    loss32, grads32, _, _ = R.loss_and_grads(dims, w, x, labels, masks, torch.float32)
    worst = max(_rel(g32, g) for g32, g in zip(grads32, grads))
    print(f"{R.case_id(case)}: torch fp32 gradients {worst:.3g} of the largest entry, loss gap {abs(loss32 - loss):.3g}, min |z1| {zmin:.3g}, "
          f"{moved} biases moved")
    assert abs(loss32 - loss) <= R.LOGP_TOL / 4
    for k, g32, g in zip(R.keys(dims[5]), grads32, grads):
        assert _rel(g32, g) <= R.ROW_TOL / 4, k


# -- 3 ---------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("fault, p", [("slots", 0.0), ("noscale", 0.0), ("mask_fwd_only", 0.1), ("residual_first", 0.1), ("eps", 0.0)])
def test_the_bars_reject_named_faults(fault, p):
    dims, L = R.SMALL, 9
    w, x, labels, masks, _ = R.make_case(dims, L, p)
    _, grads, _, _ = R.reference(dims, L, p)
    _, bad, _, _ = R.loss_and_grads(dims, w, x, labels, masks, fault=fault)
    worst = max(_rel(b, g) for b, g in zip(bad, grads))
    print(f"{fault}: {worst / R.ROW_TOL:.1f} x ROW_TOL")
    assert worst >= 3 * R.ROW_TOL


# -- 4 ---------------------------------------------------------------------------------------------------------------------------
def test_dropout_keep_is_a_fair_counter_based_coin():
    from playaid_core_amd.encoder_trainer import dropout_keep

    n, p = 1 << 20, 0.1
    base = dropout_keep(5, 3, 1, 2, n, p)
    assert base.dtype == bool and base.shape == (n,)
    assert np.array_equal(base, dropout_keep(5, 3, 1, 2, n, p))                  # deterministic
    assert np.array_equal(base[:1000], dropout_keep(5, 3, 1, 2, 1000, p))        # a pure function of the index
    assert dropout_keep(5, 3, 1, 2, n, 0.0).all()
    tol1 = 4 * math.sqrt(0.09 / n)
    for layer in range(3):
        for site in range(4):
            share = dropout_keep(5, 3, layer, site, n, p).mean()
            assert abs(share - 0.9) <= tol1, (layer, site, share)
    tol2 = 4 * math.sqrt(0.01 * 0.99 / n)
    others = {"step": dropout_keep(5, 4, 1, 2, n, p), "layer": dropout_keep(5, 3, 2, 2, n, p), "site": dropout_keep(5, 3, 1, 3, n, p),
              "seed": dropout_keep(6, 3, 1, 2, n, p), "seed high word": dropout_keep(5 + (1 << 32), 3, 1, 2, n, p)}
    for name, other in others.items():
        both = (~base & ~other).mean()
        assert abs(both - 0.01) <= tol2, (name, both)
    both = (~base[:-1] & ~base[1:]).mean()
    assert abs(both - 0.01) <= tol2, ("neighbours", both)


def test_header_specifies_the_mask_function():
    """The numpy twin is written from include/playaid_hip.h: the constants it uses are the header's."""
    text = open(os.path.join(ROOT, "include", "playaid_hip.h")).read()
    block = text[text.index("keep(seed, step, layer, site, i)"):]
    for const in ("0x7feb352d", "0x846ca68b", "0x9e3779b9", "0x85ebca6b", "4294967296.0"):
        assert const in block, const


# -- 5 ---------------------------------------------------------------------------------------------------------------------------
def test_the_toy_halves_its_loss_in_float64():
    w, x, labels = R.toy_problem()
    losses, _ = R.train(R.SMALL, w, [(x, labels)] * 30, R.TOY_LR)
    print("toy losses", " ".join(f"{l:.4f}" for l in losses))
    assert losses[-1] < 0.5 * losses[0]


# -- 6 ---------------------------------------------------------------------------------------------------------------------------
def test_new_symbols_are_declared_bound_and_exported(lib):
    from playaid_core_amd import _lib

    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "playaid_hip.h")).read(), flags=re.S)
    new = ["pa_encoder_trainer_create", "pa_encoder_trainer_destroy", "pa_encoder_trainer_last_error", "pa_encoder_trainer_steps",
           "pa_encoder_train_step", "pa_encoder_trainer_read", "pa_encoder_trainer_floats", "pa_encoder_trainer_max_windows"]
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in new:
        assert re.search(r"\b%s\s*\(" % name, text) and name in bound and hasattr(lib, name), name
    assert lib.pa_abi_version() == 15   # append-only


def _handle(lib, dims, max_rows):
    import test_encoder_head as EH

    in_dim, hidden, slots, enc, heads, layers, ff, A = dims
    w = EH.make_weights(in_dim, hidden, slots, enc, layers, ff, A, 3)
    blob = EH.pack_blob(w, in_dim, hidden, slots, enc, heads, layers, ff, A)
    h = C.c_void_p(0)
    rc = lib.pa_encoder_create(0, in_dim, hidden, slots, enc, heads, layers, ff, A, max_rows, blob.ctypes.data_as(C.c_void_p), blob.nbytes,
                               C.byref(h))
    assert h, rc   # (without a device the handle comes back for its error text)
    return h


def test_abi_refuses_bad_arguments_before_the_device(lib):
    from playaid_core_amd import _lib

    cfg = _lib.pa_adam_config(2e-4, 0.9, 0.999, 1e-8)
    t = C.c_void_p(0)
    create = lambda h, c, p=0.1: lib.pa_encoder_trainer_create(h, C.byref(c), C.c_float(p), C.c_uint64(0), C.byref(t))  # noqa: E731
    assert lib.pa_encoder_trainer_create(None, C.byref(cfg), C.c_float(0.1), C.c_uint64(0), C.byref(t)) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_encoder_trainer_floats(None) == 0 and lib.pa_encoder_trainer_max_windows(None) == 0
    assert lib.pa_encoder_trainer_steps(None) == -1 and lib.pa_encoder_trainer_last_error(None) == b"null trainer"
    assert lib.pa_encoder_train_step(None, None, 0, 1, 1, None, 1, None, None, None) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_encoder_trainer_read(None, 0, None, 0, None) == _lib.PA_ERR_INVALID_ARG
    lib.pa_encoder_trainer_destroy(None)
    h = _handle(lib, R.SMALL, 64 * 3)
    try:
        from playaid_core_amd import encoder_trainer as ET

        assert lib.pa_encoder_trainer_floats(h) == ET.tensor_floats(96, 55, 9, 2, 128, 5)
        assert lib.pa_encoder_trainer_max_windows(h) == 64
        for bad in (_lib.pa_adam_config(0.0, 0.9, 0.999, 1e-8), _lib.pa_adam_config(2e-4, 1.0, 0.999, 1e-8),
                    _lib.pa_adam_config(2e-4, 0.9, 0.999, 0.0), _lib.pa_adam_config(float("nan"), 0.9, 0.999, 1e-8)):
            assert create(h, bad) == _lib.PA_ERR_INVALID_ARG and not t
        for p in (1.0, -0.1, float("nan")):
            assert create(h, cfg, p) == _lib.PA_ERR_INVALID_ARG and not t
            assert b"dropout" in lib.pa_encoder_last_error(h)
    finally:
        lib.pa_encoder_destroy(h)
    h = _handle(lib, R.SMALL, 10 * 3)
    try:
        assert lib.pa_encoder_trainer_max_windows(h) == 10
    finally:
        lib.pa_encoder_destroy(h)
    h = _handle(lib, R.SERVED[:7] + (100,), 64)
    try:
        assert create(h, cfg) == _lib.PA_ERR_INVALID_ARG and not t
        assert b"num_actions <= 64" in lib.pa_encoder_last_error(h)
    finally:
        lib.pa_encoder_destroy(h)
    h = _handle(lib, (96, 55, 3, 9, 2, 2, 200, 5), 64)
    try:
        assert create(h, cfg) == _lib.PA_ERR_INVALID_ARG and not t
        assert b"multiples of 32" in lib.pa_encoder_last_error(h)
    finally:
        lib.pa_encoder_destroy(h)


def test_encoder_trainer_host_validation():
    from playaid_core_amd import encoder_trainer as ET
    from playaid_core_amd import trainer_base

    assert ET.EncoderTrainer.PREFIX == "pa_encoder_trainer" and issubclass(ET.EncoderTrainer, trainer_base.AdamTrainer)
    assert ET.check_adam is trainer_base.check_adam and ET.check_labels is trainer_base.check_labels
    assert len(ET.TENSOR_KEYS) == 2 + 12 * 3 + 2 and ET.TENSOR_KEYS[0] == "model.resnet_ffn.weight"
    assert ET.TENSOR_KEYS[2] == "model.transformer.layers.0.self_attn.in_proj_weight" and ET.TENSOR_KEYS[-1] == "model.classifier.bias"
    shapes = ET.tensor_shapes(2048, 247, 9, 3, 2048, 63)
    assert shapes[0] == (247, 2048) and shapes[2] == (768, 256) and shapes[6] == (2048, 256) and shapes[-2] == (63, 256)
    handle = C.c_void_p(16)   # never dereferenced: every call below is refused first
    dims = R.SERVED
    for kw in (dict(lr=0.0), dict(lr=float("inf")), dict(eps=0.0), dict(betas=(0.9, 1.0)), dict(betas=(0.9,)), dict(dropout=1.0),
               dict(dropout=-0.1), dict(dropout=float("nan")), dict(seed=-1), dict(seed=1.5), dict(dims=None), dict(dims=(1, 2, 3))):
        with pytest.raises(ValueError):
            ET.EncoderTrainer(handle, **{"dims": dims, **kw})
    good = np.zeros(14, np.int32)
    assert ET.check_step((14, 2048), 2, 7, good, 2048, 7, 63, 64) == 14
    for shape, L, N, labels in (((14, 2048), 2, 7, np.zeros(13, np.int32)), ((14, 2048), 2, 7, np.zeros(14, np.float32)),
                                ((14, 2048), 2, 7, np.full(14, 63, np.int32)), ((14, 2048), 2, 7, np.full(14, -1, np.int32)),
                                ((14, 2048), 2, 7, torch.full((14,), 63)), ((14, 2000), 2, 7, good), ((13, 2048), 2, 7, good),
                                ((14, 2048), 0, 7, good), ((12, 2048), 2, 6, np.zeros(12, np.int32))):
        with pytest.raises(ValueError):
            ET.check_step(shape, L, N, labels, 2048, 7, 63, 64)
    labels = good.copy()
    labels[::5] = ET.IGNORE
    assert ET.check_step((2, 7, 2112), 2, 7, labels, 2048, 7, 63, 64) == 14
    with pytest.raises(ValueError):
        ET.dropout_keep(0, 0, 0, 0, 4, 1.0)
