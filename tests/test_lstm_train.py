"""The LSTM trainer's kernels (csrc/lstm_train.hip, ``pa_lstm_train_*``) on seeded random feature rows -- no backbone runs.

The reference is tests/helpers/lstm_train_ref.py: torch's ``nn.LSTM``, the decoder, ``F.nll_loss(ignore_index=-100)``, autograd
and ``torch.optim.Adam`` in float64 on the CPU; the same in float32 measures what fp32 arithmetic costs against it
(tests/test_lstm_train_host.py checks on the CPU that the bars below are not idle on these very inputs).

1. gradients (``apply = 0``) against float64: each tensor within 2e-5 of its largest reference entry (the project's fp32 row
   bar), the loss within 1e-4 (the log-probability bar), the counts exact, dW_hh bitwise zero at T = 1, nothing changed;
2. no labelled row: loss 0, gradients 0;
3. Adam apart from the gradients: one float64 step from the device's own state and gradient, three times -- an update
   enqueued before a launch that still reads the tensor shows here;
4. a 30-step trajectory on a separable toy problem against ``torch.optim.Adam`` in float64;
5. the loss the trainer reports equals the NLL of ``pa_lstm_forward`` on the same rows;
6. two trainers on two handles end with the same bits;
7. the trained weights round-trip through a fresh handle;
8. a trainer that has only computed gradients leaves ``pa_lstm_forward`` bit-identical.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import lstm_head as LH  # noqa: E402
from helpers import lstm_train_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu

ROW_TOL = 2e-5    # fp32 rows against float64, relative to the tensor's largest entry
LOGP_TOL = 1e-4   # log-probabilities, hence the loss
LR = 2e-4
MAX_ROWS = 37 * 7
SEED = 31         # R.make_case's


def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _head(dims, w, max_rows=MAX_ROWS):
    _gpu()
    return LH.Head(*dims, max_rows, w)


def _trainer(head, dims, max_rows=MAX_ROWS, **kw):
    from playaid_core_amd.lstm_trainer import LSTMTrainer

    kw.setdefault("lr", LR)
    return LSTMTrainer(head.h, dims=dims, max_rows=max_rows, **kw)


def _host(d, layers):
    return [d[k].cpu().numpy() for k in R.keys(layers)]


def _loss(stats):
    return float(stats[:1].view(torch.float32).cpu()[0])


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


@pytest.fixture(scope="module")
def setups():
    """dims -> (weights, handle, trainer): never stepped, shared."""
    made = {}

    def get(dims):
        if dims not in made:
            w = LH.make_weights(*dims, SEED)
            head = _head(dims, w)
            made[dims] = (w, head, _trainer(head, dims))
        return made[dims]

    yield get
    for _, head, tr in made.values():
        tr.close()
        head.close()


@pytest.mark.parametrize("case", R.CASES, ids=R.case_id)
def test_gradients_against_float64(setups, case):
    dims, (T, N) = case
    layers = dims[2]
    w, head, tr = setups(dims)
    _, x, labels = R.make_case(case, SEED)
    assert (labels == R.IGNORE).any() == (T * N > 4)
    want_loss, want, logp = R.loss_and_grads(dims, w, x, labels)
    before = [tr.read(s) for s in ("weights", "m", "v")]
    steps = tr.steps
    got, stats = tr.grads(_dev(x), T, N, labels)
    got = _host(got, layers)
    st = stats.cpu()
    print(f"{R.case_id(case)}: loss {_loss(stats):.7f} (float64 {want_loss:.7f})")
    for key, g, r in zip(R.keys(layers), got, want):
        assert g.shape == r.shape, key
        if "weight_hh" in key and T == 1:
            assert not r.any() and int((g.view(np.int32) != 0).sum()) == 0, f"{key}: not bitwise zero at T = 1"
            continue
        err = float(np.abs(g - r).max()) / float(np.abs(r).max())
        print(f"  {key}: max|g - ref| / max|ref| = {err:.3e}")
        assert err <= ROW_TOL, key
    assert abs(_loss(stats) - want_loss) <= LOGP_TOL
    valid = labels != R.IGNORE
    assert int(st[1]) == int(valid.sum())
    assert int(st[2]) == int(((logp.argmax(1) == labels) & valid).sum())
    # apply = 0 changed nothing
    assert tr.steps == steps
    for s, b in zip(("weights", "m", "v"), before):
        after = tr.read(s)
        assert all(torch.equal(after[k].view(torch.int32), b[k].view(torch.int32)) for k in R.keys(layers)), s
    for k, a in zip(R.keys(layers), R.blob_order(w, layers)):
        assert np.array_equal(before[0][k].cpu().numpy(), a), k   # (and the weights are the handle's)


def test_no_labelled_row_gives_zero_loss_and_gradients(setups):
    """The stated departure from torch (which gives NaN): n = 0 divides by 1."""
    case = (R.SMALL, (8, 4))
    w, head, tr = setups(R.SMALL)
    _, x, _ = R.make_case(case, SEED)
    got, stats = tr.grads(_dev(x), 8, 4, np.full(32, R.IGNORE, np.int32))
    assert _loss(stats) == 0.0 and int(stats.cpu()[1]) == 0 and int(stats.cpu()[2]) == 0
    assert all(float(g.abs().max()) == 0.0 for g in got.values())


def _ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("dims", [R.SMALL, R.SERVED], ids=["small", "served"])
def test_adam_step_against_float64_from_the_devices_own_state(dims):
    """Three steps on three batches. Before each: w, m, v and the device's gradient of that batch (``grads()``); one float64
    Adam step on the host from exactly those (with the hyper-parameters as pa_adam_config carries them, fp32); after ``step()``
    on the same batch: |w - ref| <= 1e-5 lr + ulp32(w), m and v within 4 ulp of the fp32-rounded reference, every tensor moved.
    The gradient ``step()`` used is ``grads()``'s only if no tensor was updated before a launch that still read it."""
    layers, T, N = dims[2], 8, 4
    w = LH.make_weights(*dims, 6)
    head = _head(dims, w, T * N)
    tr = _trainer(head, dims, T * N)
    try:
        lr, b1, b2, eps = (float(np.float32(v)) for v in (LR, 0.9, 0.999, 1e-8))
        for k in (1, 2, 3):
            xd = _dev(LH.make_features(T, N, dims[0], 20 + k))
            labels = R.make_labels(T, N, dims[3], 40 + k)
            w0, m0, v0 = (_host(tr.read(s), layers) for s in ("weights", "m", "v"))
            g = _host(tr.grads(xd, T, N, labels)[0], layers)
            tr.step(xd, T, N, labels)
            assert tr.steps == k
            w1, m1, v1 = (_host(tr.read(s), layers) for s in ("weights", "m", "v"))
            for i, key in enumerate(R.keys(layers)):
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
    """The toy problem trained for 30 steps on the device, with the CPU float64 and float32 runs beside it."""
    dims = R.SMALL
    w, x, labels = R.toy_problem()
    T, N = x.shape[:2]
    head = _head(dims, w, T * N)
    tr = _trainer(head, dims, T * N, lr=R.TOY_LR)
    xd = _dev(x)
    stats, w3 = [], None
    for k in range(30):
        stats.append(tr.step(xd, T, N, labels))
        if k == 2:
            w3 = tr.read("weights")
    losses = [_loss(s) for s in stats]
    batches = [(x, labels)] * 30
    l64, t64 = R.train(dims, w, batches, R.TOY_LR)
    l32, t32 = R.train(dims, w, batches, R.TOY_LR, torch.float32)
    yield dict(dims=dims, w=w, x=x, xd=xd, labels=labels, T=T, N=N, head=head, tr=tr, losses=losses, w3=_host(w3, dims[2]), l64=l64,
               l32=l32, t64=t64, t32=t32)
    tr.close()
    head.close()


def test_trajectory_follows_torch_adam(toy):
    losses, l64, l32 = toy["losses"], toy["l64"], toy["l32"]
    lr = R.TOY_LR
    d32 = max(abs(a - b) for a, b in zip(l32, l64))
    worst = max(abs(a - b) for a, b in zip(losses, l64))
    print(f"loss: step 0 {losses[0]:.4f}, step 10 {losses[10]:.5f}, step 29 {losses[29]:.2e} (float64 {l64[29]:.2e}); "
          f"device - float64 {worst:.2e}, torch fp32 - float64 {d32:.2e}")
    assert toy["tr"].steps == 30
    assert l64[-1] <= 0.5 * l64[0]           # (the toy was picked so: tests/test_lstm_train_host.py)
    assert losses[-1] < losses[0]
    assert worst <= max(10 * d32, 1e-6)
    for i, key in enumerate(R.keys(toy["dims"][2])):
        w32 = float(np.abs(toy["t32"][2][i] - toy["t64"][2][i]).max())
        dev = float(np.abs(toy["w3"][i] - toy["t64"][2][i]).max())
        print(f"  after 3 steps {key}: device - float64 {dev / lr:.2e} lr, torch fp32 - float64 {w32 / lr:.2e} lr")
        assert dev <= max(10 * w32, 1e-3 * lr), key


def test_trainer_and_inference_agree(toy):
    """The trainer's loss is the NLL of pa_lstm_forward's log-probabilities on the same rows (a fifth of them unlabelled)."""
    head, tr, T, N = toy["head"], toy["tr"], toy["T"], toy["N"]
    labels = toy["labels"].copy()
    labels[::5] = R.IGNORE
    lp = head.forward(toy["x"]).astype(np.float64)
    _, stats = tr.grads(toy["xd"], T, N, labels)
    valid = labels != R.IGNORE
    nll = -float(np.mean(lp[np.flatnonzero(valid), labels[valid]]))
    print(f"inference NLL {nll:.3e}, trainer loss {_loss(stats):.3e}")
    assert abs(nll - _loss(stats)) <= LOGP_TOL
    assert int(stats.cpu()[1]) == int(valid.sum())
    assert int(stats.cpu()[2]) == int(((lp.argmax(1) == labels) & valid).sum())


def test_two_trainers_end_with_the_same_bits():
    dims, T, N = R.SMALL, 9, 7
    w = LH.make_weights(*dims, 8)
    ends = []
    for _ in range(2):
        head = _head(dims, w, T * N)
        tr = _trainer(head, dims, T * N)
        try:
            for k in range(5):
                tr.step(_dev(LH.make_features(T, N, dims[0], 60 + k)), T, N, R.make_labels(T, N, dims[3], 70 + k))
            ends.append([{k: v.clone() for k, v in tr.read(s).items()} for s in ("weights", "m", "v")])
        finally:
            tr.close()
            head.close()
    for a, b in zip(*ends):
        assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in R.keys(dims[2]))
    assert float(ends[0][1]["lstm.weight_hh_l0"].abs().max()) > 0


def test_trained_weights_round_trip(toy):
    """A fresh handle built from read("weights") is the trained handle, and the weights are not the initial ones."""
    dims, head, tr = toy["dims"], toy["head"], toy["tr"]
    layers = dims[2]
    got = _host(tr.read("weights"), layers)
    for key, a, b in zip(R.keys(layers), got, R.blob_order(toy["w"], layers)):
        assert float(np.abs(a - b).max()) > R.TOY_LR, key   # (trained, not the initial weights)
    head2 = _head(dims, R.from_blob_order(got, layers), toy["T"] * toy["N"])
    try:
        a, b = head.forward(toy["x"]), head2.forward(toy["x"])
        assert np.array_equal(a.view(np.int32), b.view(np.int32))
    finally:
        head2.close()


def test_gradient_calls_leave_inference_untouched(setups):
    """An untrained handle with a trainer attached that has only been asked for gradients: pa_lstm_forward gives the bits of a
    handle without a trainer."""
    dims = R.SERVED
    w, head, tr = setups(dims)
    case = (dims, (8, 4))
    _, x, labels = R.make_case(case, SEED)
    tr.grads(_dev(x), 8, 4, labels)
    assert tr.steps == 0
    plain = _head(dims, w)
    try:
        a, b = head.forward(x), plain.forward(x)
        assert np.isfinite(a).all() and np.array_equal(a.view(np.int32), b.view(np.int32))
    finally:
        plain.close()
