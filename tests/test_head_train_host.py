"""The head trainer without a GPU: what ``pa_head_trainer_create`` / ``pa_head_train_step`` / ``pa_head_trainer_read`` refuse
before any device call, header / bindings / exports of the new symbols, ``HeadTrainer``'s host-side validation, and the
float64 reference of tests/helpers/head_train_ref.py against central differences."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import head_train_ref as R  # noqa: E402

from playaid_core_amd import synth  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pa_head_trainer_create", "pa_head_trainer_destroy", "pa_head_trainer_last_error", "pa_head_trainer_steps", "pa_head_train_step",
       "pa_head_trainer_read")


@pytest.fixture(scope="module")
def lib():
    from playaid_core_amd import _build, _lib

    _build.build()
    return _lib.load()


def test_new_symbols_are_declared_bound_and_exported(lib):
    from playaid_core_amd import _lib

    hdr = open(os.path.join(ROOT, "include", "playaid_hip.h")).read()
    bound = {name for name, _, _ in _lib.SYMBOLS}
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, hdr) and name in bound and hasattr(lib, name), name
    assert _lib.PA_ABI_VERSION == 15 == lib.pa_abi_version()
    assert ctypes.sizeof(_lib.pa_adam_config) == 16 and ctypes.sizeof(_lib.pa_train_stats) == 16
    for macro, val in (("PA_TRAIN_WEIGHTS", _lib.PA_TRAIN_WEIGHTS), ("PA_TRAIN_M", _lib.PA_TRAIN_M), ("PA_TRAIN_V", _lib.PA_TRAIN_V),
                       ("PA_TRAIN_RAW", _lib.PA_TRAIN_RAW)):
        assert int(re.search(r"#define %s (\d+)" % macro, hdr).group(1)) == val


def test_abi_refuses_bad_arguments_before_the_device(lib):
    from playaid_core_amd import _lib, weights

    z = ctypes.c_void_p(0)
    x = ctypes.c_void_p(4096)   # never dereferenced: every call it is given to is refused first
    h = ctypes.c_void_p(0)
    good = _lib.pa_adam_config(2e-4, 0.9, 0.999, 1e-8)
    assert lib.pa_head_trainer_create(z, ctypes.byref(good), 64, ctypes.byref(h)) == _lib.PA_ERR_INVALID_ARG and not h
    assert lib.pa_head_trainer_create(x, None, 64, ctypes.byref(h)) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_head_trainer_create(x, ctypes.byref(good), 64, None) == _lib.PA_ERR_INVALID_ARG
    for mb in (0, -3, 257):
        assert lib.pa_head_trainer_create(x, ctypes.byref(good), mb, ctypes.byref(h)) == _lib.PA_ERR_INVALID_ARG and not h
    inf, nan = float("inf"), float("nan")
    for bad in ((0.0, 0.9, 0.999, 1e-8), (-1e-3, 0.9, 0.999, 1e-8), (inf, 0.9, 0.999, 1e-8), (nan, 0.9, 0.999, 1e-8),
                (2e-4, 0.9, 0.999, 0.0), (2e-4, 0.9, 0.999, -1e-8), (2e-4, 0.9, 0.999, inf), (2e-4, 0.9, 0.999, nan),
                (2e-4, 1.0, 0.999, 1e-8), (2e-4, -0.1, 0.999, 1e-8), (2e-4, nan, 0.999, 1e-8),
                (2e-4, 0.9, 1.0, 1e-8), (2e-4, 0.9, -0.5, 1e-8), (2e-4, 0.9, nan, 1e-8)):
        cfg = _lib.pa_adam_config(*bad)
        assert lib.pa_head_trainer_create(x, ctypes.byref(cfg), 64, ctypes.byref(h)) == _lib.PA_ERR_INVALID_ARG and not h, bad
    # null handles
    assert lib.pa_head_train_step(z, x, 1, x, x, 1, 1, z, z, z) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_head_trainer_read(z, 0, x, 1, z) == _lib.PA_ERR_INVALID_ARG
    assert lib.pa_head_trainer_steps(z) == -1 and lib.pa_head_trainer_last_error(z) == b"null trainer"
    lib.pa_head_trainer_destroy(z)
    # a real engine handle: without a device its creation stops there and hands the handle back; so does the trainer's
    S, A = 3, 5
    cfg = _lib.pa_config()
    cfg.abi_version = _lib.PA_ABI_VERSION
    cfg.sequence_length, cfg.num_actions, cfg.num_fighters, cfg.frame_delta = S, A, 2, 4
    cfg.max_batch_frames, cfg.max_clip_frames, cfg.max_frame_height, cfg.max_frame_width = 2, 8, 96, 128
    blob = weights.pack_state_dict(synth.make_state_dict(seed=5, num_actions=A, sequence_length=S), S, A)
    e = ctypes.c_void_p(0)
    rc_e = lib.pa_create(ctypes.byref(cfg), blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, ctypes.byref(e))
    assert e, rc_e
    try:
        rc = lib.pa_head_trainer_create(e, ctypes.byref(good), 8, ctypes.byref(h))
        assert h and rc == (_lib.PA_OK if rc_e == _lib.PA_OK else _lib.PA_ERR_NO_DEVICE), (rc_e, rc)
        try:
            assert lib.pa_head_trainer_steps(h) == 0
            for args in ((x, 1, x, x, 0, 1, z), (x, 1, x, x, -2, 1, z), (x, 1, x, x, 9, 1, z),      # batch < 1, > max_batch
                         (z, 1, x, x, 1, 1, z), (x, 1, z, x, 1, 1, z), (x, 1, x, z, 1, 1, z),      # null inputs
                         (x, 0, x, x, 1, 1, z), (x, 1, x, x, 1, 2, z), (x, 1, x, x, 1, 0, z)):     # no rows, apply = 2, no grads_out
                assert lib.pa_head_train_step(h, *args, z, z) == _lib.PA_ERR_INVALID_ARG, args
                assert b"pa_head_train_step" in lib.pa_head_trainer_last_error(h)
            assert lib.pa_head_trainer_read(h, 3, x, 1, z) == _lib.PA_ERR_INVALID_ARG
            assert lib.pa_head_trainer_read(h, 0, z, 512000 * S + 66176 + 129 * A, z) == _lib.PA_ERR_INVALID_ARG
            assert lib.pa_head_trainer_read(h, 0, x, 17, z) == _lib.PA_ERR_INVALID_ARG
            assert lib.pa_head_trainer_steps(h) == 0
        finally:
            lib.pa_head_trainer_destroy(h)
    finally:
        lib.pa_destroy(e)


def test_head_trainer_host_validation():
    from playaid_core_amd import head_trainer as ht

    assert ht.tensor_floats(3, 5) == 512000 * 3 + 66176 + 129 * 5
    assert ht.TENSOR_KEYS == R.KEYS
    ht.check_adam(2e-4, (0.9, 0.999), 1e-8, 256)
    for bad in ((0.0, (0.9, 0.999), 1e-8, 64), (float("nan"), (0.9, 0.999), 1e-8, 64), (2e-4, (1.0, 0.999), 1e-8, 64),
                (2e-4, (0.9,), 1e-8, 64), (2e-4, (0.9, 0.999), 0.0, 64), (2e-4, (0.9, 0.999), 1e-8, 257), (2e-4, (0.9, 0.999), 1e-8, 0)):
        with pytest.raises(ValueError):
            ht.check_adam(*bad)
    S, A, n = 3, 5, 10
    g = np.arange(12, dtype=np.int32).reshape(4, 3) % n
    l = np.array([0, 4, ht.IGNORE, 2], np.int32)
    assert ht.check_batch(g, l, n, S, A, 8) == 4
    assert ht.check_batch(torch.from_numpy(g), torch.from_numpy(l), n, S, A, 8) == 4
    for gg, ll in ((g[:, :2], l), (g, l[:3]), (g.reshape(-1), l), (g.astype(np.float32), l), (np.where(g == 3, n, g), l),
                   (np.where(g == 3, -1, g), l), (g, np.array([0, 5, 1, 2], np.int32)), (g, np.array([0, -1, 1, 2], np.int32)),
                   (g, l.astype(np.float64))):
        with pytest.raises(ValueError):
            ht.check_batch(gg, ll, n, S, A, 8)
    with pytest.raises(ValueError):
        ht.check_batch(g, l, n, S, A, 3)          # more windows than max_batch
    with pytest.raises(ValueError):
        ht.check_batch(g, l, 0, S, A, 8)


def test_reference_gradient_against_central_differences():
    """The helper's float64 autograd gradient, 20 entries per tensor, against (L(w + h) - L(w - h)) / 2h."""
    S, A, B = 3, 5, 7
    sd = synth.make_state_dict(seed=5, num_actions=A, sequence_length=S)
    feats = R.make_feats(50, 3)
    gather, labels = R.make_batch(50, B, S, A, 9)
    _, grads = R.loss_and_grads(sd, feats, gather, labels)
    rng = np.random.default_rng(0)
    h = 1e-6
    for i, key in enumerate(R.KEYS):
        g = grads[i].reshape(-1)
        picks = rng.choice(np.flatnonzero(g), size=min(20, int(np.count_nonzero(g))), replace=False)
        for j in picks:
            vals = []
            for sign in (+1, -1):
                params = R.head_params(sd, requires_grad=False)
                params[i].view(-1)[j] += sign * h
                vals.append(float(R.loss_of(params, feats, gather, labels)))
            fd = (vals[0] - vals[1]) / (2 * h)
            assert abs(fd - g[j]) <= 1e-7 + 1e-5 * abs(g[j]), (key, j, fd, g[j])
    # no labelled window: the stated departure (loss 0, gradients 0)
    loss, grads = R.loss_and_grads(sd, feats, gather, np.full(B, R.IGNORE, np.int32))
    assert loss == 0.0 and all(float(np.abs(g).max()) == 0.0 for g in grads)
