"""The LSTM trainer without a GPU: header / bindings / exports of the new symbols, what ``pa_lstm_trainer_create`` /
``pa_lstm_train_step`` / ``pa_lstm_trainer_read`` refuse before any device call, ``LSTMTrainer``'s host-side validation, the
float64 reference of tests/helpers/lstm_train_ref.py against central differences, and -- on the CPU, for every case the GPU
tests run -- that their bars are not idle: torch's own fp32 run stays within a quarter of the bar and the reference gradient is
not mostly zeros."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import lstm_head as LH  # noqa: E402
from helpers import lstm_train_ref as R  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("pa_lstm_trainer_create", "pa_lstm_trainer_destroy", "pa_lstm_trainer_last_error", "pa_lstm_trainer_steps", "pa_lstm_train_step",
       "pa_lstm_trainer_read", "pa_lstm_trainer_floats")


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


def _handle(lib, dims, max_rows):
    """A pa_lstm handle; without a device its creation stops at PA_ERR_NO_DEVICE and still hands the handle back."""
    w = LH.make_weights(*dims, 3)
    blob = LH.pack_blob(w, *dims)
    h = ctypes.c_void_p(0)
    rc = lib.pa_lstm_create(0, *dims, max_rows, blob.ctypes.data_as(ctypes.c_void_p), blob.nbytes, ctypes.byref(h))
    assert h, rc
    return h, rc


def test_abi_refuses_bad_arguments_before_the_device(lib):
    from playaid_core_amd import _lib

    z = ctypes.c_void_p(0)
    x = ctypes.c_void_p(4096)   # never dereferenced: every call it is given to is refused first
    t = ctypes.c_void_p(0)
    good = _lib.pa_adam_config(2e-4, 0.9, 0.999, 1e-8)
    dims = (21, 32, 2, 5)
    h, rc_h = _handle(lib, dims, 40)
    try:
        assert lib.pa_lstm_trainer_floats(z) == 0
        assert lib.pa_lstm_trainer_floats(h) == sum(int(np.prod(a.shape)) for a in R.blob_order(LH.make_weights(*dims, 3), dims[2]))
        assert lib.pa_lstm_trainer_create(z, ctypes.byref(good), ctypes.byref(t)) == _lib.PA_ERR_INVALID_ARG and not t
        assert lib.pa_lstm_trainer_create(h, None, ctypes.byref(t)) == _lib.PA_ERR_INVALID_ARG and not t
        assert lib.pa_lstm_trainer_create(h, ctypes.byref(good), None) == _lib.PA_ERR_INVALID_ARG
        inf, nan = float("inf"), float("nan")
        for bad in ((0.0, 0.9, 0.999, 1e-8), (-1e-3, 0.9, 0.999, 1e-8), (inf, 0.9, 0.999, 1e-8), (nan, 0.9, 0.999, 1e-8),
                    (2e-4, 0.9, 0.999, 0.0), (2e-4, 0.9, 0.999, -1e-8), (2e-4, 0.9, 0.999, inf), (2e-4, 0.9, 0.999, nan),
                    (2e-4, 1.0, 0.999, 1e-8), (2e-4, -0.1, 0.999, 1e-8), (2e-4, nan, 0.999, 1e-8),
                    (2e-4, 0.9, 1.0, 1e-8), (2e-4, 0.9, -0.5, 1e-8), (2e-4, 0.9, nan, 1e-8)):
            cfg = _lib.pa_adam_config(*bad)
            assert lib.pa_lstm_trainer_create(h, ctypes.byref(cfg), ctypes.byref(t)) == _lib.PA_ERR_INVALID_ARG and not t, bad
        # null trainers
        assert lib.pa_lstm_train_step(z, x, 32, 2, 2, x, 1, z, z, z) == _lib.PA_ERR_INVALID_ARG
        assert lib.pa_lstm_trainer_read(z, 0, x, 1, z) == _lib.PA_ERR_INVALID_ARG
        assert lib.pa_lstm_trainer_steps(z) == -1 and lib.pa_lstm_trainer_last_error(z) == b"null trainer"
        lib.pa_lstm_trainer_destroy(z)
        # hidden sizes that are no multiple of 32 stay inference-only
        for hid in (8, 200):
            h2, _ = _handle(lib, (21, hid, 2, 5), 40)
            try:
                assert lib.pa_lstm_trainer_create(h2, ctypes.byref(good), ctypes.byref(t)) == _lib.PA_ERR_INVALID_ARG and not t
                assert b"multiple of 32" in lib.pa_lstm_last_error(h2)
            finally:
                lib.pa_lstm_destroy(h2)
        # a real handle: where its creation stopped at the device, so does the trainer's, and hands the trainer back
        rc = lib.pa_lstm_trainer_create(h, ctypes.byref(good), ctypes.byref(t))
        assert t and rc == (_lib.PA_OK if rc_h == _lib.PA_OK else _lib.PA_ERR_NO_DEVICE), (rc_h, rc)
        try:
            assert lib.pa_lstm_trainer_steps(t) == 0
            #        x, ld, seq_len, batch, labels, apply, grads_out
            for args in ((z, 32, 2, 2, x, 1, z), (x, 32, 2, 2, z, 1, z),                       # null inputs
                         (x, 32, 0, 2, x, 1, z), (x, 32, -1, 2, x, 1, z),                      # seq_len < 1
                         (x, 32, 2, 0, x, 1, z), (x, 32, 2, 17, x, 1, z), (x, 32, 2, -4, x, 1, z),   # batch outside 1..16
                         (x, 32, 41, 1, x, 1, z), (x, 32, 3, 14, x, 1, z), (x, 32, 2 ** 30, 16, x, 1, z),   # more rows than max_rows
                         (x, 20, 2, 2, x, 1, z),                                               # ld < input_dim
                         (x, 32, 2, 2, x, 2, z), (x, 32, 2, 2, x, -1, x), (x, 32, 2, 2, x, 0, z)):   # apply, no grads_out
                assert lib.pa_lstm_train_step(t, *args, z, z) == _lib.PA_ERR_INVALID_ARG, args
                assert b"pa_lstm_train_step" in lib.pa_lstm_trainer_last_error(t)
            n = lib.pa_lstm_trainer_floats(h)
            assert lib.pa_lstm_trainer_read(t, 3, x, n, z) == _lib.PA_ERR_INVALID_ARG
            assert lib.pa_lstm_trainer_read(t, -1, x, n, z) == _lib.PA_ERR_INVALID_ARG
            assert lib.pa_lstm_trainer_read(t, _lib.PA_TRAIN_RAW, x, n, z) == _lib.PA_ERR_INVALID_ARG
            assert lib.pa_lstm_trainer_read(t, _lib.PA_TRAIN_M | _lib.PA_TRAIN_RAW, x, n, z) == _lib.PA_ERR_INVALID_ARG
            assert lib.pa_lstm_trainer_read(t, 0, z, n, z) == _lib.PA_ERR_INVALID_ARG
            assert lib.pa_lstm_trainer_read(t, 0, x, n - 1, z) == _lib.PA_ERR_INVALID_ARG
            assert lib.pa_lstm_trainer_steps(t) == 0
        finally:
            lib.pa_lstm_trainer_destroy(t)
    finally:
        lib.pa_lstm_destroy(h)


def test_lstm_trainer_host_validation():
    from playaid_core_amd import lstm_trainer as lt

    assert lt.TENSOR_KEYS == R.keys(3) and lt.tensor_keys(1) == R.keys(1)
    shapes = lt.tensor_shapes(300, 512, 3, 63)
    assert len(shapes) == 16 and shapes[0] == (2048, 300) and shapes[4] == (2048, 512) and shapes[5] == (2048, 512)
    assert shapes[2] == shapes[3] == (2048,) and shapes[12:] == ((128, 512), (128,), (63, 128), (63,))
    w = LH.make_weights(21, 32, 2, 5, 3)
    assert lt.tensor_shapes(21, 32, 2, 5) == tuple(tuple(a.shape) for a in R.blob_order(w, 2))
    assert lt.tensor_floats(21, 32, 2, 5) == (LH.pack_blob(w, 21, 32, 2, 5).nbytes - 32) // 4
    with pytest.raises(ValueError):
        lt.LSTMTrainer(ctypes.c_void_p(4096), lr=0.0, dims=(21, 32, 2, 5), max_rows=8)   # (check_adam comes first)
    with pytest.raises(ValueError):
        lt.LSTMTrainer(ctypes.c_void_p(4096), betas=(0.9, 1.0), dims=(21, 32, 2, 5), max_rows=8)
    T, N, A, ld = 4, 3, 5, 1024
    l = np.array([0, 4, lt.IGNORE, 2] * 3, np.int32)
    assert lt.check_step((T, N, ld), T, N, l, 21, A, 12) == 12
    assert lt.check_step((T * N, ld), T, N, torch.from_numpy(l).view(T, N), 21, A, 12) == 12
    assert lt.check_step((T, N, 21), T, N, l.tolist(), 21, A, 12) == 12
    for shape, t, n, ll, rows in (((T, N, ld), 0, N, l, 12), ((T, N, ld), T, 0, l, 12), ((T, 17, ld), T, 17, np.zeros(68, np.int32), 100),
                                  ((T, N, ld), T, N, l, 11),                               # more rows than max_rows
                                  ((T, N, 20), T, N, l, 12), ((T, 2, ld), T, N, l, 12), ((ld,), T, N, l, 12),   # x's shape
                                  ((T, N, ld), T, N, l[:11], 12), ((T, N, ld), T, N, l.astype(np.float32), 12),
                                  ((T, N, ld), T, N, np.where(l == 4, 5, l), 12), ((T, N, ld), T, N, np.where(l == 4, -1, l), 12),
                                  ((T, N, ld), T, N, torch.from_numpy(l).double(), 12), ((T, N, ld), 1.5, N, l, 12)):
        with pytest.raises(ValueError):
            lt.check_step(shape, t, n, ll, 21, A, rows)


def test_both_trainers_take_their_scaffolding_and_label_check_from_trainer_base():
    """``HeadTrainer`` and ``LSTMTrainer`` define none of the shared scaffolding themselves -- it is ``AdamTrainer``'s --, their
    modules hold no constants or label check of their own, and ``check_labels`` refuses through both entry points what the two
    separate checks refused: a float array, a label of A, a label of -1; -100 passes."""
    from playaid_core_amd import head_trainer as ht
    from playaid_core_amd import lstm_trainer as lt
    from playaid_core_amd import trainer_base as tb

    shared = ("_raise", "_check", "_stream", "close", "__del__", "__enter__", "__exit__", "steps", "loss_of", "_split", "read", "epoch_stats",
              "_count", "_begin", "_created")
    for cls in (ht.HeadTrainer, lt.LSTMTrainer):
        assert issubclass(cls, tb.AdamTrainer) and cls.PREFIX == f"pa_{'head' if cls is ht.HeadTrainer else 'lstm'}_trainer"
        for name in shared:
            assert name in vars(tb.AdamTrainer) and name not in vars(cls), (cls.__name__, name)
        for name in ("__init__", "_run", "step", "grads"):
            assert name in vars(cls), (cls.__name__, name)
    assert "_inputs" in vars(ht.HeadTrainer) and "read_raw" in vars(ht.HeadTrainer)
    assert ht.IGNORE is tb.IGNORE is lt.IGNORE and tb.IGNORE == -100 and ht._WHICH is tb._WHICH
    assert ht.check_labels is tb.check_labels is lt.check_labels and lt.check_adam is tb.check_adam
    assert "head_trainer" not in open(lt.__file__).read()
    tb.check_adam(2e-4, (0.9, 0.999), 1e-8)
    ht.check_adam(2e-4, (0.9, 0.999), 1e-8, 1)
    for bad in ((0.0, (0.9, 0.999), 1e-8), (2e-4, (0.9, 1.0), 1e-8), (2e-4, (0.9, 0.999), float("inf"))):
        for check in (tb.check_adam, lambda *a: ht.check_adam(*a, 64)):
            with pytest.raises(ValueError):
                check(*bad)

    A, n = 5, 4
    good = np.array([0, 4, tb.IGNORE, 2], np.int32)
    g = np.arange(n * 3, dtype=np.int32).reshape(n, 3) % 10
    entries = (lambda l: tb.check_labels(l, n, A), lambda l: ht.check_batch(g, l, 10, 3, A, 8), lambda l: lt.check_step((n, 1, 32), n, 1, l, 21, A, n))
    for entry in entries:
        for ok in (good, good.tolist(), torch.from_numpy(good), good.astype(np.int64), np.full(n, tb.IGNORE, np.int32)):
            entry(ok)
        for bad in (good.astype(np.float32), torch.from_numpy(good).double(), good.astype(bool), np.where(good == 4, A, good),
                    np.where(good == 4, -1, good), np.where(good == 4, -99, good), good[:3]):
            with pytest.raises(ValueError):
                entry(bad)


def test_reference_gradient_against_central_differences():
    """The helper's float64 autograd gradient, 20 entries per tensor, against (L(w + h) - L(w - h)) / 2h."""
    case = (R.SMALL, (8, 4))
    dims = case[0]
    w, x, labels = R.make_case(case)
    assert (labels == R.IGNORE).any()
    _, grads, _ = R.loss_and_grads(dims, w, x, labels)
    rng = np.random.default_rng(0)
    h = 1e-6
    xs = torch.as_tensor(x[..., :dims[0]], dtype=torch.float64)
    net = R.Net(dims, w)
    with torch.no_grad():
        for i, key in enumerate(R.keys(dims[2])):
            g = grads[i].reshape(-1)
            p = net.ordered()[i].view(-1)
            picks = rng.choice(np.flatnonzero(g), size=min(20, int(np.count_nonzero(g))), replace=False)
            assert len(picks) >= min(20, g.size // 2), key
            for j in picks:
                vals = []
                for sign in (+1, -1):
                    old = float(p[j])
                    p[j] = old + sign * h
                    vals.append(float(net.loss(xs, labels)))
                    p[j] = old
                fd = (vals[0] - vals[1]) / (2 * h)
                assert abs(fd - g[j]) <= 1e-7 + 1e-5 * abs(g[j]), (key, j, fd, g[j])
    # no labelled row: the stated departure (loss 0, gradients 0)
    loss, grads, _ = R.loss_and_grads(dims, w, x, np.full(labels.shape, R.IGNORE, np.int32))
    assert loss == 0.0 and all(float(np.abs(g).max()) == 0.0 for g in grads)


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_the_gpu_bars_are_not_idle(case):
    """For the inputs of tests/test_lstm_train.py's gradient cases: torch's own fp32 gradient is within ROW_TOL / 4 of float64
    (relative to the tensor's largest entry) and its loss within LOGP_TOL / 4, and at least 0.2 of every reference gradient is
    non-zero -- but weight_hh at T = 1, which is identically zero."""
    dims, (T, N) = case
    w, x, labels = R.make_case(case)
    assert (labels == R.IGNORE).any() == (T * N > 4)
    l64, g64, _ = R.loss_and_grads(dims, w, x, labels)
    l32, g32, _ = R.loss_and_grads(dims, w, x, labels, torch.float32)
    assert abs(l32 - l64) <= R.LOGP_TOL / 4
    for key, a, b in zip(R.keys(dims[2]), g32, g64):
        if "weight_hh" in key and T == 1:
            assert not b.any() and not a.any(), key
            continue
        err = float(np.abs(a - b).max()) / float(np.abs(b).max())
        nz = float((b != 0).mean())
        print(f"{key}: torch fp32 - float64 {err:.2e} of the largest entry, non-zero share {nz:.2f}")
        assert err <= R.ROW_TOL / 4, key
        assert nz >= 0.2, key


def test_the_toy_halves_its_loss_in_float64():
    w, x, labels = R.toy_problem()
    losses, _ = R.train(R.SMALL, w, [(x, labels)] * 30, R.TOY_LR)
    print(f"float64 loss {losses[0]:.4f} -> {losses[-1]:.4f}")
    assert losses[-1] <= 0.5 * losses[0]
