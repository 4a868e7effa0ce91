"""The head trainer's kernels (csrc/head_train.hip, ``pa_head_train_*``) on seeded random feature rows -- no backbone runs.

The reference is tests/helpers/head_train_ref.py: the reference model's head, ``F.nll_loss(ignore_index=-100)``, autograd and
``torch.optim.Adam`` in float64 on the CPU; the same in float32 measures what fp32 arithmetic costs against it, and the bars
that are not the project's standing ones are multiples of that measured distance, computed here.

1. gradients (``apply = 0``) against float64: each tensor within 2e-5 of its largest reference entry (the project's fp32 row
   bar; torch's own fp32 run is at 2-5e-7 on these inputs), the loss within 1e-4 (the log-probability bar);
2. Adam apart from the gradients: one float64 step from the device's own state and gradient, three times;
3. a 30-step trajectory on a separable toy problem against ``torch.optim.Adam`` in float64;
4. the loss the trainer reports equals the NLL of the engine's ordinary head on the same windows;
5. two trainers on two engines end with the same bits;
6. the trained weights round-trip: ``read("weights")`` equals the arena re-packed on the host, and a fresh engine built from
   them gives bit-identical log-probabilities.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from helpers import head_train_ref as R  # noqa: E402

from playaid_core_amd import synth  # noqa: E402

pytestmark = pytest.mark.gpu

N_ROWS = 300
SHAPES = [(3, 5, 1), (3, 5, 7), (7, 63, 64), (7, 63, 37), (7, 63, 256)]
ROW_TOL = 2e-5    # fp32 rows against float64, relative to the tensor's largest entry
LOGP_TOL = 1e-4   # log-probabilities, hence the loss
LR = 2e-4


def _engine(sd, **kw):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from playaid_core_amd.engine import Engine

    kw.setdefault("max_batch_frames", 8)
    kw.setdefault("max_clip_frames", 64)
    return Engine(sd, **kw)


def _trainer(eng, **kw):
    from playaid_core_amd.head_trainer import HeadTrainer

    kw.setdefault("lr", LR)
    kw.setdefault("max_batch", 256)
    return HeadTrainer(eng, **kw)


def _host(d):
    return [d[k].cpu().numpy() for k in R.KEYS]


def _loss(stats):
    return float(stats[:1].view(torch.float32).cpu()[0])


@pytest.fixture(scope="module")
def setups():
    """(S, A) -> (state dict, engine, trainer, feats on the device, feats on the host): never stepped, shared."""
    made = {}

    def get(S, A):
        if (S, A) not in made:
            sd = synth.make_state_dict(seed=5, num_actions=A, sequence_length=S)
            eng = _engine(sd)
            feats = R.make_feats(N_ROWS, 3)
            made[(S, A)] = (sd, eng, _trainer(eng), feats.cuda(), feats)
        return made[(S, A)]

    yield get
    for _, eng, tr, _, _ in made.values():
        tr.close()
        eng.close()


@pytest.mark.parametrize("S,A,B", SHAPES)
def test_gradients_against_float64(setups, S, A, B):
    sd, eng, tr, fd, fh = setups(S, A)
    gather, labels = R.make_batch(N_ROWS, B, S, A, 9)
    assert (labels == R.IGNORE).any() == (B > 4) and len(set(gather[0])) == 1
    want_loss, want = R.loss_and_grads(sd, fh, gather, labels)
    before = [tr.read(w) for w in ("weights", "m", "v")]
    steps = tr.steps
    got, stats = tr.grads(fd, gather, labels)
    got = _host(got)
    st = stats.cpu()
    print(f"S={S} A={A} B={B}: loss {_loss(stats):.7f} (float64 {want_loss:.7f})")
    for key, g, w in zip(R.KEYS, got, want):
        nz = float((w != 0).mean())
        err = float(np.abs(g - w).max()) / float(np.abs(w).max())
        print(f"  {key}: max|g - ref| / max|ref| = {err:.3e}, non-zero share of the reference {nz:.2f}")
        assert nz >= 0.2, f"{key}: an idle check"
        assert g.shape == w.shape and err <= ROW_TOL, key
    assert abs(_loss(stats) - want_loss) <= LOGP_TOL
    assert int(st[1]) == int((labels != R.IGNORE).sum())
    lp = R.forward(R.head_params(sd, requires_grad=False), fh, gather)
    assert int(st[2]) == int(((lp.argmax(1).numpy() == labels) & (labels != R.IGNORE)).sum())
    # apply = 0 changed nothing
    assert tr.steps == steps
    for w, b in zip(("weights", "m", "v"), before):
        after = tr.read(w)
        assert all(torch.equal(after[k], b[k]) for k in R.KEYS), w


def test_no_labelled_window_gives_zero_loss_and_gradients(setups):
    """The stated departure from torch (which gives NaN): n = 0 divides by 1."""
    sd, eng, tr, fd, fh = setups(3, 5)
    gather, _ = R.make_batch(N_ROWS, 6, 3, 5, 4)
    got, stats = tr.grads(fd, gather, np.full(6, R.IGNORE, np.int32))
    assert _loss(stats) == 0.0 and int(stats.cpu()[1]) == 0
    assert all(float(g.abs().max()) == 0.0 for g in got.values())


def _ulp32(a):
    return np.spacing(np.abs(a).astype(np.float32)).astype(np.float64)


@pytest.mark.parametrize("S,A,B", [(3, 5, 7), (7, 63, 37)])
def test_adam_step_against_float64_from_the_devices_own_state(S, A, B):
    """Three steps on three batches. Before each: w, m, v and the device's gradient of that batch; one float64 Adam step on
    the host from exactly those (with the hyper-parameters as pa_adam_config carries them, fp32); after: |w - ref| <= 1e-5 lr +
    ulp32(w), m and v within 4 ulp of the fp32-rounded reference. The padding of all three layouts stays bitwise zero."""
    sd = synth.make_state_dict(seed=6, num_actions=A, sequence_length=S)
    eng = _engine(sd)
    tr = _trainer(eng)
    try:
        fd = R.make_feats(N_ROWS, 8).cuda()
        lr, b1, b2, eps = (float(np.float32(x)) for x in (LR, 0.9, 0.999, 1e-8))
        for k in (1, 2, 3):
            gather, labels = R.make_batch(N_ROWS, B, S, A, 20 + k)
            w0, m0, v0 = (_host(tr.read(x)) for x in ("weights", "m", "v"))
            g = _host(tr.grads(fd, gather, labels)[0])
            tr.step(fd, gather, labels)
            assert tr.steps == k
            w1, m1, v1 = (_host(tr.read(x)) for x in ("weights", "m", "v"))
            for i, key in enumerate(R.KEYS):
                wr, mr, vr = R.adam_step_f64(w0[i], m0[i], v0[i], g[i], k, lr, b1, b2, eps)
                dw = np.abs(w1[i] - wr) - _ulp32(wr)
                dm = np.abs(m1[i] - mr.astype(np.float32)) / _ulp32(mr)
                dv = np.abs(v1[i] - vr.astype(np.float32)) / _ulp32(vr)
                print(f"step {k} {key}: w off by {float(np.abs(w1[i] - wr).max()) / lr:.2e} lr, m {float(dm.max()):.1f} ulp, v {float(dv.max()):.1f} ulp")
                assert float(dw.max()) <= 1e-5 * lr, key
                assert float(dm.max()) <= 4 and float(dv.max()) <= 4, key
                assert float(np.abs(w1[i] - w0[i]).max()) > 0.5 * lr, f"{key} did not move"
        for which in ("weights", "m", "v"):
            raw = tr.read_raw(which)
            assert raw[0].shape == (512, S, 1024) and raw[4].shape == (128, 64)
            assert int((raw[0][:, :, 1000:].view(torch.int32) != 0).sum()) == 0, which
            assert int((raw[4][:, A:].view(torch.int32) != 0).sum()) == 0, which
            assert float(raw[0][:, :, :1000].abs().max()) > 0
    finally:
        tr.close()
        eng.close()


@pytest.fixture(scope="module")
def toy():
    """The toy problem trained for 30 steps on the device, with the CPU float64 and float32 runs beside it."""
    sd, feats, gather, labels = R.toy_problem()
    eng = _engine(sd, num_fighters=1, frame_delta=1)
    tr = _trainer(eng, max_batch=32)
    fd = feats.cuda()
    stats, w3 = [], None
    for k in range(30):
        stats.append(tr.step(fd, gather, labels))
        if k == 2:
            w3 = tr.read("weights")
    losses = [_loss(s) for s in stats]
    batches = [(feats, gather, labels)] * 30
    l64, t64 = R.train(sd, batches, LR)
    l32, t32 = R.train(sd, batches, LR, torch.float32)
    yield dict(sd=sd, feats=feats, fd=fd, gather=gather, labels=labels, eng=eng, tr=tr, losses=losses, w3=_host(w3), l64=l64, l32=l32,
               t64=t64, t32=t32)
    tr.close()
    eng.close()


def test_trajectory_follows_torch_adam(toy):
    losses, l64, l32 = toy["losses"], toy["l64"], toy["l32"]
    d32 = max(abs(a - b) for a, b in zip(l32, l64))
    worst = max(abs(a - b) for a, b in zip(losses, l64))
    print(f"loss: step 0 {losses[0]:.4f}, step 5 {losses[5]:.5f}, step 10 {losses[10]:.6f}, step 29 {losses[29]:.2e}; "
          f"device - float64 {worst:.2e}, torch fp32 - float64 {d32:.2e}")
    assert toy["tr"].steps == 30
    assert losses[10] < 0.1 * losses[0]
    assert worst <= max(10 * d32, 1e-6)
    for i, key in enumerate(R.KEYS):
        w32 = float(np.abs(toy["t32"][2][i] - toy["t64"][2][i]).max())
        dev = float(np.abs(toy["w3"][i] - toy["t64"][2][i]).max())
        print(f"  after 3 steps {key}: device - float64 {dev / LR:.2e} lr, torch fp32 - float64 {w32 / LR:.2e} lr")
        assert dev <= max(10 * w32, 1e-3 * LR), key


def test_trainer_and_inference_agree(toy):
    """The windows are the engine's own (one fighter, frame_delta 1): features_import + head_frames is the ordinary head."""
    eng, tr, gather, labels = toy["eng"], toy["tr"], toy["gather"], toy["labels"]
    n = toy["feats"].shape[0]
    eng.clip_begin(n)
    eng.features_import(0, toy["fd"].view(n, 1, 1024))
    lp = eng.alloc_logp(n - 1)
    eng.head_frames(1, n, eng.alloc_records(n - 1), lp)
    _, stats = tr.grads(toy["fd"], gather, labels)
    lp = lp.cpu().numpy()[:, 0].astype(np.float64)
    nll = -float(np.mean(lp[np.arange(len(labels)), labels]))
    print(f"inference NLL {nll:.3e}, trainer loss {_loss(stats):.3e}")
    assert abs(nll - _loss(stats)) <= LOGP_TOL
    assert int(stats.cpu()[2]) == int((lp.argmax(1) == labels).sum())


def test_two_trainers_end_with_the_same_bits():
    S, A, B = 3, 5, 33
    sd = synth.make_state_dict(seed=8, num_actions=A, sequence_length=S)
    fd = R.make_feats(N_ROWS, 12).cuda()
    ends = []
    for _ in range(2):
        eng = _engine(sd)
        tr = _trainer(eng)
        try:
            for k in range(5):
                gather, labels = R.make_batch(N_ROWS, B, S, A, 40 + k)
                tr.step(fd, gather, labels)
            ends.append([{k: v.clone() for k, v in tr.read(w).items()} for w in ("weights", "m", "v")])
        finally:
            tr.close()
            eng.close()
    for a, b in zip(*ends):
        assert all(torch.equal(a[k].view(torch.int32), b[k].view(torch.int32)) for k in R.KEYS)


def test_trained_weights_round_trip(toy):
    """read("weights") is the arena re-packed on the host, and an engine built from the read-out is the trained engine."""
    eng, tr, sd = toy["eng"], toy["tr"], toy["sd"]
    S, A = eng.S, eng.A
    got = _host(tr.read("weights"))
    arena = eng.weights_arena().data.cpu().numpy()
    # the head tensors are the arena's last six, each 256-byte aligned; all but the last have sizes that are multiples of 256
    sizes = [512 * S * 1024, 512, 512 * 128, 128, 128 * 64]
    end = arena.size - 4 * A
    assert end % 256 == 0
    b3 = arena[end:].view(np.float32)
    parts = []
    for n in reversed(sizes):
        parts.append(arena[end - 4 * n:end].view(np.float32))
        end -= 4 * n
    w3, b2, w2, b1, w1 = parts
    assert np.array_equal(got[0], w1.reshape(512, S, 1024)[:, :, :1000].transpose(0, 2, 1))
    assert np.array_equal(got[1], b1) and np.array_equal(got[3], b2) and np.array_equal(got[5], b3)
    assert np.array_equal(got[2], w2.reshape(512, 128).T) and np.array_equal(got[4], w3.reshape(128, 64).T[:A])
    assert float(np.abs(got[0] - np.asarray(sd[R.KEYS[0]])).max()) > LR   # (trained, not the initial weights)
    new_sd = dict(sd)
    new_sd.update({k: v for k, v in zip(R.KEYS, got)})
    eng2 = _engine(new_sd, num_fighters=1, frame_delta=1)
    try:
        n = toy["feats"].shape[0]
        out = []
        for e in (eng, eng2):
            e.clip_begin(n)
            e.features_import(0, toy["fd"].view(n, 1, 1024))
            lp = e.alloc_logp(n - 1)
            e.head_frames(1, n, e.alloc_records(n - 1), lp)
            out.append(lp.cpu())
        assert torch.equal(out[0].view(torch.int32), out[1].view(torch.int32))
    finally:
        eng2.close()
