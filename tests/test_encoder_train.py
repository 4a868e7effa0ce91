"""The encoder trainer's kernels (csrc/encoder_train.hip, ``pa_encoder_train_*``) on seeded random feature rows -- no backbone runs.

The reference is tests/helpers/encoder_train_ref.py: the head written out with torch ops under autograd and ``torch.optim.Adam``
in float64 on the CPU, fed the trainer's own dropout masks (``encoder_trainer.dropout_keep``); the same in float32 measures
what fp32 arithmetic costs against it (tests/test_encoder_train_host.py checks on the CPU that the bars below are reachable and
not idle on these very inputs, and that no case has a ReLU kink).

1. gradients (``apply = 0``, p = 0) against float64: each tensor within 2e-5 of its largest reference entry (the project's fp32
   row bar), the loss within 1e-4 (the log-probability bar), the counts exact, the q and k parts of in_proj bitwise zero at
   L = 1, nothing changed;
2. the same with dropout: the kernels' masks are the header's function, the same in both directions;
3. no labelled row: loss 0, gradients 0;
4. Adam apart from the gradients: one float64 step from the device's own state and gradient, three times -- an update
   enqueued before a launch that still reads the tensor shows here, and so does a mask that moved between grads() and step();
5. a 30-step trajectory on a separable toy problem against ``torch.optim.Adam`` in float64;
6. the loss the trainer reports equals the NLL of ``pa_encoder_forward`` on the same rows after applied steps (the padded
   projection is refreshed);
7. two trainers with one seed end with the same bits, another seed does not;
8. the trained weights round-trip through a fresh handle;
9. a trainer that has only computed gradients leaves ``pa_encoder_forward`` bit-identical;
10. refusals come from the host with a message.
"""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import test_encoder_head as EH  # noqa: E402
from helpers import encoder_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROW_TOL = 2e-5    # fp32 rows against float64, relative to the tensor's largest entry
LOGP_TOL = 1e-4   # log-probabilities, hence the loss
LR = 2e-4
CAP = 64          # pa_encoder_trainer_max_windows at max_rows >= 64 slots' worth


class Head:
    """A ``pa_encoder`` handle on the weights ``w`` (``test_encoder_head.make_weights``' dictionary)."""

    def __init__(self, dims, w, max_rows):
        from playaid_core_amd import _lib

        if not torch.cuda.is_available():
            pytest.skip("no GPU")
        self.lib = _lib.load()
        self.dims = dims
        in_dim, hidden, slots, enc, heads, layers, ff, A = dims
        blob = EH.pack_blob(w, in_dim, hidden, slots, enc, heads, layers, ff, A)
        self.h = C.c_void_p()
        rc = self.lib.pa_encoder_create(0, in_dim, hidden, slots, enc, heads, layers, ff, A, max_rows, blob.ctypes.data_as(C.c_void_p),
                                        blob.nbytes, C.byref(self.h))
        assert rc == 0, self.lib.pa_encoder_last_error(self.h).decode() if self.h else rc

    def forward(self, x):
        """x float32[L, N, ld] (host) -> log-probabilities float32[L * N, A] (host)."""
        from playaid_core_amd.engine import _ptr

        L, N, ld = x.shape
        xd = _dev(x)
        out = torch.full((L * N, self.dims[7]), float("nan"), device="cuda")
        rc = self.lib.pa_encoder_forward(self.h, _ptr(xd), ld, L, N, _ptr(out), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, self.lib.pa_encoder_last_error(self.h).decode()
        return out.cpu().numpy()

    def close(self):
        if self.h:
            self.lib.pa_encoder_destroy(self.h)
            self.h = C.c_void_p()


def _trainer(head, **kw):
    from playaid_core_amd.encoder_trainer import EncoderTrainer

    kw.setdefault("lr", LR)
    kw.setdefault("dropout", 0.0)
    return EncoderTrainer(head.h, dims=head.dims, **kw)


def _host(d, tr):
    return [d[k].cpu().numpy() for k in tr.keys]


def _loss(stats):
    return float(stats[:1].view(torch.float32).cpu()[0])


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rel(g, r):
    return float(np.abs(g.astype(np.float64) - r).max()) / float(np.abs(r).max())


def _check_gradients(tr, dims, L, p, w, x, labels, name):
    """``grads()`` against the cached float64 reference of the case; returns the host gradients."""
    layers, N = dims[5], dims[2]
    want_loss, want, logp, _ = R.reference(dims, L, p)
    got, stats = tr.grads(_dev(x), L, N, labels)
    got = _host(got, tr)
    st = stats.cpu()
    print(f"{name}: loss {_loss(stats):.7f} (float64 {want_loss:.7f})")
    D = dims[1] + dims[3]
    for key, g, r in zip(R.keys(layers), got, want):
        assert g.shape == r.shape, key
        if L == 1 and key.endswith((".in_w", ".in_b")):
            # one key: softmax is 1 whatever the score, dS = 0 exactly, and with it dQ and dK
            assert not r[:2 * D].any() and int((g[:2 * D].view(np.int32) << 1 != 0).sum()) == 0, f"{key}: q and k parts not zero at L = 1"
            g, r = g[2 * D:], r[2 * D:]
        err = _rel(g, r)
        print(f"  {key}: max|g - ref| / max|ref| = {err:.3e}")
        assert err <= ROW_TOL, key
    assert abs(_loss(stats) - want_loss) <= LOGP_TOL
    valid = labels != R.IGNORE
    assert int(st[1]) == int(valid.sum())
    assert int(st[2]) == int(((logp.argmax(1) == labels) & valid).sum())
    return got


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_gradients_against_float64(case):
    dims, L = case
    layers, N = dims[5], dims[2]
    w, x, labels, _, _ = R.make_case(dims, L)
    assert (labels == R.IGNORE).any() == (L * N > 4)
    head = Head(dims, w, CAP * N)
    tr = _trainer(head)
    try:
        assert tr.max_windows == CAP
        before = [tr.read(s) for s in ("weights", "m", "v")]
        _check_gradients(tr, dims, L, 0.0, w, x, labels, R.case_id(case))
        # apply = 0 changed nothing
        assert tr.steps == 0
        for s, b in zip(("weights", "m", "v"), before):
            after = tr.read(s)
            assert all(torch.equal(after[k].view(torch.int32), b[k].view(torch.int32)) for k in tr.keys), s
        for k, a in zip(tr.keys, R.blob_order(w, layers)):
            assert np.array_equal(before[0][k].cpu().numpy(), a), k   # (and the weights are the handle's)
    finally:
        tr.close()
        head.close()


@pytest.mark.parametrize("case", R.DROPOUT_CASES, ids=R.case_id)
def test_gradients_with_dropout_against_float64_under_the_same_masks(case):
    """The float64 reference is fed ``dropout_keep``'s masks for the trainer's seed (0) and step (0): this passes only if the
    kernels' masks are the header's function of the torch-layout index, and the same in the forward and the backward pass."""
    dims, L, p = case
    w, x, labels, masks, _ = R.make_case(dims, L, p)
    head = Head(dims, w, L * dims[2])
    tr = _trainer(head, dropout=p, seed=0)
    try:
        a = _check_gradients(tr, dims, L, p, w, x, labels, R.case_id(case))
        b = _host(tr.grads(_dev(x), L, dims[2], labels)[0], tr)
        assert all(np.array_equal(u.view(np.int32), v.view(np.int32)) for u, v in zip(a, b))   # the step did not move: nor did the masks
    finally:
        tr.close()
        head.close()


def test_no_labelled_row_gives_zero_loss_and_gradients():
    """The stated departure from torch (which gives NaN): n = 0 divides by 1."""
    dims, L = R.SMALL, 9
    w, x, _, _, _ = R.make_case(dims, L)
    head = Head(dims, w, L * dims[2])
    tr = _trainer(head, dropout=0.1)
    try:
        got, stats = tr.grads(_dev(x), L, dims[2], np.full(L * dims[2], R.IGNORE, np.int32))
        assert _loss(stats) == 0.0 and int(stats.cpu()[1]) == 0 and int(stats.cpu()[2]) == 0
        assert all(float(g.abs().max()) == 0.0 for g in got.values())
    finally:
        tr.close()
        head.close()


def _ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("dims", [R.SMALL, R.SERVED], ids=["small", "served"])
def test_adam_step_against_float64_from_the_devices_own_state(dims):
    """Three steps on three batches with dropout 0.1. Before each: w, m, v and the device's gradient of that batch (``grads()``,
    under the masks of the step to come); one float64 Adam step on the host from exactly those (with the hyper-parameters as
    pa_adam_config carries them, fp32); after ``step()`` on the same batch: |w - ref| <= 1e-5 lr + ulp32(w), m and v within 4 ulp
    of the fp32-rounded reference, every tensor moved. The gradient ``step()`` used is ``grads()``'s only if no tensor was updated
    before a launch that still read it and the masks did not advance in between."""
    in_dim, N, A, L = dims[0], dims[2], dims[7], 8
    w = EH.make_weights(in_dim, dims[1], N, dims[3], dims[5], dims[6], A, 6)
    head = Head(dims, w, L * N)
    tr = _trainer(head, dropout=0.1, seed=9)
    try:
        lr, b1, b2, eps = (float(np.float32(v)) for v in (LR, 0.9, 0.999, 1e-8))
        for k in (1, 2, 3):
            xd = _dev(EH.make_features(L, N, in_dim, 20 + k))
            labels = R.make_labels(L, N, A, 40 + k)
            w0, m0, v0 = (_host(tr.read(s), tr) for s in ("weights", "m", "v"))
            g = _host(tr.grads(xd, L, N, labels)[0], tr)
            tr.step(xd, L, N, labels)
            assert tr.steps == k
            w1, m1, v1 = (_host(tr.read(s), tr) for s in ("weights", "m", "v"))
            for i, key in enumerate(R.keys(dims[5])):
                wr, mr, vr = R.adam_step_f64(w0[i], m0[i], v0[i], g[i], k, lr, b1, b2, eps)
                dw = np.abs(w1[i] - wr) - _ulp32(wr)
                dm = np.abs(m1[i] - mr.astype(np.float32)) / _ulp32(mr)
                dv = np.abs(v1[i] - vr.astype(np.float32)) / _ulp32(vr)
                print(f"step {k} {key}: w off by {float(np.abs(w1[i] - wr).max()) / lr:.2e} lr, m {float(dm.max()):.1f} ulp, v {float(dv.max()):.1f} ulp")
                assert float(dw.max()) <= 1e-5 * lr, key
                assert float(dm.max()) <= 4 and float(dv.max()) <= 4, key
                assert float(np.abs(w1[i] - w0[i]).max()) > 0.5 * lr, f"{key} did not move"
    finally:
        tr.close()
        head.close()


@pytest.fixture(scope="module")
def toy():
    """The toy problem trained for 30 steps on the device (p = 0), with the CPU float64 and float32 runs beside it."""
    dims = R.SMALL
    w, x, labels = R.toy_problem()
    L, N = x.shape[:2]
    head = Head(dims, w, L * N)
    tr = _trainer(head, lr=R.TOY_LR)
    xd = _dev(x)
    stats, w3 = [], None
    for k in range(30):
        stats.append(tr.step(xd, L, N, labels))
        if k == 2:
            w3 = tr.read("weights")
    losses = [_loss(s) for s in stats]
    batches = [(x, labels)] * 30
    l64, t64 = R.train(dims, w, batches, R.TOY_LR)
    l32, t32 = R.train(dims, w, batches, R.TOY_LR, torch.float32)
    yield dict(dims=dims, w=w, x=x, xd=xd, labels=labels, L=L, N=N, head=head, tr=tr, losses=losses, w3=_host(w3, tr), l64=l64, l32=l32,
               t64=t64, t32=t32)
    tr.close()
    head.close()


def test_trajectory_follows_torch_adam(toy):
    losses, l64, l32 = toy["losses"], toy["l64"], toy["l32"]
    lr = R.TOY_LR
    dims = toy["dims"]
    D = dims[1] + dims[3]
    d32 = max(abs(a - b) for a, b in zip(l32, l64))
    worst = max(abs(a - b) for a, b in zip(losses, l64))
    print(f"loss: step 0 {losses[0]:.4f}, step 10 {losses[10]:.5f}, step 29 {losses[29]:.2e} (float64 {l64[29]:.2e}); "
          f"device - float64 {worst:.2e}, torch fp32 - float64 {d32:.2e}")
    assert toy["tr"].steps == 30
    assert l64[-1] <= 0.5 * l64[0]           # (the toy was picked so: tests/test_encoder_train_host.py)
    assert losses[-1] < losses[0]
    assert worst <= max(10 * d32, 1e-6)
    for i, key in enumerate(R.keys(dims[5])):
        a64, a32, dev = toy["t64"][2][i], toy["t32"][2][i], toy["w3"][i]
        if key.endswith(".in_b"):
            # the k third is left out: softmax is invariant under a shift of all scores of a query, so the true gradient of the key
            # bias is zero and Adam's m / sqrt(v) turns the rounding noise of any precision into steps of +-lr
            keep = np.r_[0:D, 2 * D:3 * D]
            a64, a32, dev = a64[keep], a32[keep], dev[keep]
        w32 = float(np.abs(a32 - a64).max())
        d = float(np.abs(dev - a64).max())
        print(f"  after 3 steps {key}: device - float64 {d / lr:.2e} lr, torch fp32 - float64 {w32 / lr:.2e} lr")
        assert d <= max(10 * w32, 1e-3 * lr), key


def test_trainer_and_inference_agree_after_applied_steps():
    """SERVED, five applied steps (p = 0), then a fifth of the rows unlabelled: the trainer's loss is the NLL of
    pa_encoder_forward's log-probabilities on the same rows. At this shape inference reads the zero-padded copy of the front
    projection: a copy left stale by the steps shows here."""
    dims, L = R.SERVED, 8
    N, A = dims[2], dims[7]
    w, x, labels, _, _ = R.make_case(dims, L)
    head = Head(dims, w, L * N)
    tr = _trainer(head, lr=1e-3)
    try:
        xd = _dev(x)
        first = head.forward(x)
        for _ in range(5):
            tr.step(xd, L, N, labels)
        lp = head.forward(x).astype(np.float64)
        assert float(np.abs(lp - first).max()) > 10 * LOGP_TOL   # the steps moved the model by far more than the bar
        labels = R.make_labels(L, N, A, 77)
        assert (labels == R.IGNORE).sum() >= L * N // 5
        _, stats = tr.grads(xd, L, N, labels)
        valid = labels != R.IGNORE
        nll = -float(np.mean(lp[np.flatnonzero(valid), labels[valid]]))
        print(f"inference NLL {nll:.6f}, trainer loss {_loss(stats):.6f}")
        assert abs(nll - _loss(stats)) <= LOGP_TOL
        assert int(stats.cpu()[1]) == int(valid.sum())
        assert int(stats.cpu()[2]) == int(((lp.argmax(1) == labels) & valid).sum())
    finally:
        tr.close()
        head.close()


def test_two_trainers_with_one_seed_end_with_the_same_bits():
    dims, L = R.SMALL, 9
    in_dim, N, A = dims[0], dims[2], dims[7]
    w = EH.make_weights(in_dim, dims[1], N, dims[3], dims[5], dims[6], A, 8)
    ends = []
    for seed in (4, 4, 5):
        head = Head(dims, w, L * N)
        tr = _trainer(head, dropout=0.1, seed=seed)
        try:
            for k in range(5):
                tr.step(_dev(EH.make_features(L, N, in_dim, 60 + k)), L, N, R.make_labels(L, N, A, 70 + k))
            ends.append([{k: v.clone() for k, v in tr.read(s).items()} for s in ("weights", "m", "v")])
            keys = tr.keys
        finally:
            tr.close()
            head.close()
    for a, b in zip(ends[0], ends[1]):
        assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in keys)
    assert not all(torch.equal(ends[0][0][k], ends[2][0][k]) for k in keys)   # another seed: other masks
    assert float(ends[0][1][keys[2]].abs().max()) > 0


def test_trained_weights_round_trip(toy):
    """A fresh handle built from read("weights") is the trained handle, and the weights are not the initial ones."""
    dims, head, tr = toy["dims"], toy["head"], toy["tr"]
    layers = dims[5]
    got = _host(tr.read("weights"), tr)
    for key, a, b in zip(R.keys(layers), got, R.blob_order(toy["w"], layers)):
        assert not np.array_equal(a, b), key   # (trained, not the initial weights)
    head2 = Head(dims, R.from_blob_order(got, layers, toy["w"]["enc"]), toy["L"] * toy["N"])
    try:
        a, b = head.forward(toy["x"]), head2.forward(toy["x"])
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    finally:
        head2.close()


def test_gradient_calls_leave_inference_untouched():
    """An untrained handle with a trainer attached that has only been asked for gradients: pa_encoder_forward gives the bits of
    a handle without a trainer."""
    dims, L = R.SERVED, 8
    N = dims[2]
    w, x, labels, _, _ = R.make_case(dims, L)
    head, plain = Head(dims, w, L * N), Head(dims, w, L * N)
    tr = _trainer(head, dropout=0.1)
    try:
        tr.grads(_dev(x), L, N, labels)
        assert tr.steps == 0
        a, b = head.forward(x), plain.forward(x)
        assert np.isfinite(a).all() and np.array_equal(a.view(np.int32), b.view(np.int32))
    finally:
        tr.close()
        head.close()
        plain.close()


def test_refusals_come_from_the_host_with_a_message():
    from playaid_core_amd import _lib
    from playaid_core_amd.engine import EngineError

    dims = R.SMALL
    in_dim, N, A = dims[0], dims[2], dims[7]
    w = EH.make_weights(in_dim, dims[1], N, dims[3], dims[5], dims[6], A, 3)
    head = Head(dims, w, (CAP + 1) * N)
    tr = _trainer(head)
    try:
        assert tr.max_windows == CAP
        L = CAP + 1
        with pytest.raises(EngineError) as e:
            tr.step(_dev(EH.make_features(L, N, in_dim, 5)), L, N, np.zeros(L * N, np.int32))
        assert e.value.code == _lib.PA_ERR_CAPACITY and "max_windows" in str(e.value)
        assert tr.steps == 0
        flat = torch.empty(tr._floats, device="cuda")
        stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
        rc = tr._lib.pa_encoder_trainer_read(tr._h, _lib.PA_TRAIN_WEIGHTS | _lib.PA_TRAIN_RAW, C.c_void_p(flat.data_ptr()), tr._floats, stream)
        assert rc == _lib.PA_ERR_INVALID_ARG and b"pa_encoder_trainer_read" in tr._lib.pa_encoder_trainer_last_error(tr._h)
        cfg = _lib.pa_adam_config(LR, 0.9, 0.999, 1e-8)
        t = C.c_void_p(0)
        rc = tr._lib.pa_encoder_trainer_create(head.h, C.byref(cfg), C.c_float(1.0), C.c_uint64(0), C.byref(t))
        assert rc == _lib.PA_ERR_INVALID_ARG and not t and b"dropout" in tr._lib.pa_encoder_last_error(head.h)
    finally:
        tr.close()
        head.close()
    dims = R.SERVED[:7] + (100,)
    w = EH.make_weights(dims[0], dims[1], dims[2], dims[3], dims[5], dims[6], 100, 3)
    head = Head(dims, w, 8 * dims[2])
    try:
        with pytest.raises(EngineError) as e:
            _trainer(head)
        assert e.value.code == _lib.PA_ERR_INVALID_ARG and "num_actions <= 64" in str(e.value)
    finally:
        head.close()
