"""The ResNet-18 stem on integer pixels (csrc/stem_pool.hip, FORM 2), through the C ABI.

The exact engines multiply the pixel INTEGERS 0 .. 255 (each exactly one bf16) with the three bf16 slices of the folded fp32 weights on
the bf16 matrix cores -- every product exact, fp32 sums -- and divide by 255 once. Neither this nor the fp32 stem on ``k / 255`` is
"the" fp32 value; float64 is the arbiter.

CPU: the slices add up to the weight exactly; the entry point refuses bad arguments before anything is enqueued.

GPU, operator (``pa_stem_int``): crops ``n`` = 1, 5, 64, 72, 128, 130 are the sizes at which the launcher's paths differ (8 runs of 4
row pairs a crop; an odd count; runs of 4; the engine's unequal interleaved halves; runs of 8 on 512 workgroups; more runs than
workgroups). Every batch is drawn from one pool of eight crops (three random, all 0, all 255, a 255 impulse at two corners and at
the centre) whose float64 reference is computed once:
  * against float64: ``max|got - ref| <= 2e-5 * max|ref|``, the bar of tests/test_backbone_layers.py for this stage, on the
    engine's synthetic weights and on weights whose magnitudes span six decades;
  * against today's fp32 kernel (``pa_backbone_trace`` stage 1 on ``x = k / 255``): the integer form's error is at most twice the
    fp32 form's (its sums are three times as long: sqrt(3) in rounding, twice is the margin);
  * a crop's output at n = 1 is bit for bit its output at any position of any larger batch; twenty launches give the same bits;
    the packed input has a zero border and fourth channel and the u8 values inside.

GPU, engine: the default process against ``PA_STEM_INT=0`` (a child) for each producer of the model input; ``pa_infer_windows``
(caller floats: the fp32 stem) alternating with each producer on one engine; unequal interleaved halves (72 crops).
"""
import ctypes
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import stem_int_worker as worker  # noqa: E402

P = "model.cnn2d."
F32_BAR = 2e-5
SIZES = [1, 5, 64, 72, 128, 130]
POOL = 8


def bf16_to_f64(u16):
    return (np.asarray(u16, np.uint32) << np.uint32(16)).view(np.float32).astype(np.float64)


def fold_stem(sd):
    """fold_conv of the engine: float64 scale, weights and bias each rounded to fp32. -> (w [64,3,7,7] f32, b [64] f32)"""
    w = np.asarray(sd[P + "conv1.weight"], np.float64)
    g, b, m, v = (np.asarray(sd[P + "bn1" + k], np.float64) for k in (".weight", ".bias", ".running_mean", ".running_var"))
    scale = g / np.sqrt(v + 1e-5)
    return (w * scale[:, None, None, None]).astype(np.float32), (b - m * scale).astype(np.float32)


def six_decades(sd):
    """The synthetic checkpoint with stem weights whose magnitudes run from 1e-6 to 1 (log-uniform), either sign."""
    rng = np.random.default_rng(606)
    sd = dict(sd)
    shape = np.asarray(sd[P + "conv1.weight"]).shape
    mag = 10.0 ** rng.uniform(-6.0, 0.0, shape)
    sd[P + "conv1.weight"] = (mag * rng.choice([-1.0, 1.0], shape)).astype(np.float32)
    return sd


def state_dict_of(kind, base):
    return base if kind == "synthetic" else six_decades(base)


def pool_crops():
    rng = np.random.default_rng(2024)
    c = np.zeros((POOL, 128, 128, 3), np.uint8)
    c[0] = rng.integers(0, 256, (128, 128, 3))
    c[2] = 255
    c[3, 0, 0] = 255        # impulses: tap alignment against the zero border
    c[4, 63, 64] = 255
    c[5, 127, 127] = 255
    c[6] = rng.integers(0, 256, (128, 128, 3))
    c[7] = rng.integers(0, 64, (128, 128, 3))   # dark crop: small integers
    return c


def batch_index(n):
    """Which pool crop sits at position i of a batch of n: every pool crop at many positions, the order differs per n."""
    return (np.arange(n) * 5 + n) % POOL


def reference(crops, w, b):
    """float64: conv2d(k / 255, w) + b, ReLU, 3x3/2 max-pool -> [n, 32, 32, 64]"""
    import torch
    import torch.nn.functional as F

    x = torch.from_numpy(crops.astype(np.float64) / 255.0).permute(0, 3, 1, 2)
    y = F.conv2d(x, torch.from_numpy(w.astype(np.float64)), torch.from_numpy(b.astype(np.float64)), stride=2, padding=3)
    return F.max_pool2d(F.relu(y), 3, 2, 1).permute(0, 2, 3, 1).numpy()


# =====================================================================================================================
# CPU
# =====================================================================================================================
def test_slices_add_up_to_the_weight_exactly(state_dict):
    from playaid_core_amd import conv

    for kind in ("synthetic", "six_decades"):
        w, _ = fold_stem(state_dict_of(kind, state_dict))
        sl = conv.stem_int_pack_weights(w)
        assert sl.shape == (3, 64, 224) and sl.dtype == np.uint16
        v = bf16_to_f64(sl).reshape(3, 64, 7, 8, 4)
        assert not v[:, :, :, 7].any() and not v[..., 3].any()          # the eighth pixel of a tap row and the fourth channel
        got = v[:, :, :, :7, :3].sum(axis=0).transpose(0, 3, 1, 2)       # [64][ky][kx][c] -> OIHW
        assert np.array_equal(got, w.astype(np.float64)), kind
        # every product of a slice with a pixel integer has at most 16 significant bits: exact in fp32
        m, _ = np.frexp(v)
        assert np.array_equal(np.ldexp(m, 8), np.round(np.ldexp(m, 8)))
        # slice order: |s1| <= half an ulp of s0's 8 bits, |s2| likewise of s1
        assert (np.abs(v[1]) <= np.abs(v[0]) * 2.0 ** -8 + 1e-300).all() and (np.abs(v[2]) <= np.abs(v[1]) * 2.0 ** -8 + 1e-300).all()


def test_entry_point_refuses_bad_arguments():
    from playaid_core_amd import _lib

    lib = _lib.load()
    z, a16, a4 = ctypes.c_void_p(0), ctypes.c_void_p(4096), ctypes.c_void_p(4100)
    bad = _lib.PA_ERR_INVALID_ARG
    ok_args = [a16, a16, a16, a16, a16]
    for i in range(5):   # every pointer null in turn
        args = list(ok_args)
        args[i] = z
        assert lib.pa_stem_int(*args, 4, z) == bad, i
    assert lib.pa_stem_int(*ok_args, 0, z) == bad
    assert lib.pa_stem_int(*ok_args, -3, z) == bad
    assert lib.pa_stem_int(*ok_args, 8193, z) == bad
    for i in (1, 3, 4):  # slices, packed input and output move in 16-byte units
        args = list(ok_args)
        args[i] = a4
        assert lib.pa_stem_int(*args, 4, z) == bad, i
    assert lib.pa_stem_int(a16, a16, ctypes.c_void_p(4098), a16, a16, 4, z) == bad
    w = np.zeros((64, 7, 7, 3), np.float32)
    assert lib.pa_stem_int_pack_weights(z, w.ctypes.data_as(ctypes.c_void_p)) == bad
    assert lib.pa_stem_int_pack_weights(w.ctypes.data_as(ctypes.c_void_p), z) == bad


# =====================================================================================================================
# GPU: the operator
# =====================================================================================================================
_CACHE = {}


def _operator(kind, state_dict):
    """Per weight set, once per module: folded weights, device slices and bias, the pool's float64 reference and its outputs at n = 1."""
    if kind not in _CACHE:
        import torch
        from playaid_core_amd import conv

        w, b = fold_stem(state_dict_of(kind, state_dict))
        sl = torch.from_numpy(conv.stem_int_pack_weights(w).view(np.int16)).cuda()
        bd = torch.from_numpy(b).cuda()
        crops = pool_crops()
        ref = reference(crops, w, b)
        ref.setflags(write=False)
        base = []
        for i in range(POOL):
            out, _ = conv.stem_int(torch.from_numpy(crops[i:i + 1]).cuda(), sl, bd)
            base.append(out.cpu().numpy())
        base = np.concatenate(base)
        base.setflags(write=False)
        _CACHE[kind] = dict(w=w, b=b, sl=sl, bd=bd, crops=crops, ref=ref, base=base)
    return _CACHE[kind]


def _border_is_zero(a, pad):
    return not (a[:, :pad].any() or a[:, -pad:].any() or a[:, :, :pad].any() or a[:, :, -pad:].any())


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["synthetic", "six_decades"])
def test_operator_against_float64(state_dict, kind):
    op = _operator(kind, state_dict)
    ref, base = op["ref"], op["base"]
    assert (ref != 0).mean() > 0.2
    assert _border_is_zero(base, 1)
    bar = F32_BAR * np.abs(ref).max()
    err = np.abs(base[:, 1:-1, 1:-1].astype(np.float64) - ref)
    per_crop = err.reshape(POOL, -1).max(axis=1)
    print(f"{kind}: n = 1, max|got - ref| per pool crop / bar = {np.array2string(per_crop / bar, precision=3)}")
    assert err.max() <= bar, f"{kind}: max|err| = {err.max() / bar:.3g} x the 2e-5 bar"


@pytest.mark.gpu
@pytest.mark.parametrize("n", SIZES[1:])
@pytest.mark.parametrize("kind", ["synthetic", "six_decades"])
def test_operator_is_independent_of_batch_and_position(state_dict, kind, n):
    """A crop's bits at n = 1 are its bits at every position of a batch of n (and so the float64 bar holds there too); the packed
    input is the u8 crop inside a zero border."""
    import torch
    from playaid_core_amd import conv

    op = _operator(kind, state_dict)
    idx = batch_index(n)
    crops = op["crops"][idx]
    out, packed = conv.stem_int(torch.from_numpy(crops).cuda(), op["sl"], op["bd"])
    got = out.cpu().numpy()
    assert _border_is_zero(got, 1)
    same = (got == op["base"][idx]).reshape(n, -1).all(axis=1)
    assert same.all(), f"{kind} n={n}: crops at positions {np.flatnonzero(~same)[:8]} differ from their n = 1 bits"
    bar = F32_BAR * np.abs(op["ref"]).max()
    err = np.abs(got[:, 1:-1, 1:-1].astype(np.float64) - op["ref"][idx]).max()
    print(f"{kind}: n = {n}, max|got - ref| / bar = {err / bar:.3g}")
    assert err <= bar
    pk = packed.float().cpu().numpy()   # bf16 -> fp32 is exact
    assert _border_is_zero(pk, 3) and not pk[..., 3].any()
    assert np.array_equal(pk[:, 3:-3, 3:-3, :3], crops.astype(np.float32))


@pytest.mark.gpu
def test_twenty_launches_give_the_same_bits(state_dict):
    import torch
    from playaid_core_amd import conv

    op = _operator("synthetic", state_dict)
    crops = torch.from_numpy(op["crops"][batch_index(130)]).cuda()
    first, packed = conv.stem_int(crops, op["sl"], op["bd"])
    for _ in range(19):
        again, _ = conv.stem_int(crops, op["sl"], op["bd"], packed=packed)
        assert torch.equal(first, again)


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["synthetic", "six_decades"])
def test_integer_form_against_the_fp32_kernel(state_dict, kind):
    """Both forms on the pool, both against float64: the integer form's error within twice the fp32 kernel's."""
    import torch
    from playaid_core_amd.engine import Engine

    op = _operator(kind, state_dict)
    eng = Engine(state_dict_of(kind, state_dict), max_batch_frames=POOL // 2, max_clip_frames=16, max_frame_height=128, max_frame_width=128)
    try:
        x = (op["crops"].astype(np.float32) / np.float32(255)).transpose(0, 3, 1, 2)   # the producers' k / 255, NCHW
        f32 = eng.backbone_trace(torch.from_numpy(np.ascontiguousarray(x)).cuda(), 1).cpu().numpy()
    finally:
        eng.close()
    ref = op["ref"]
    e_f32 = np.abs(f32[:, 1:-1, 1:-1].astype(np.float64) - ref).max()
    e_int = np.abs(op["base"][:, 1:-1, 1:-1].astype(np.float64) - ref).max()
    bar = F32_BAR * np.abs(ref).max()
    print(f"{kind}: max|err| against float64: fp32 kernel {e_f32:.4g} ({e_f32 / bar:.3g} of the bar), integer form {e_int:.4g} "
          f"({e_int / bar:.3g} of the bar), ratio {e_int / e_f32:.3g}")
    assert e_f32 <= bar
    assert e_int <= 2.0 * e_f32, f"{kind}: integer form {e_int:.4g} > 2 x fp32 kernel {e_f32:.4g}"


# =====================================================================================================================
# GPU: the engine
# =====================================================================================================================
def _child(tmp_path, stem_int):
    env = dict(os.environ)
    env.pop("PA_STEM_INT", None)
    if stem_int is not None:
        env["PA_STEM_INT"] = stem_int
    path = str(tmp_path / f"stem_int_{stem_int}.npz")
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "stem_int_worker.py"), path], capture_output=True, text=True,
                       env=env, timeout=600)
    assert r.returncode == 0, (stem_int, r.returncode, r.stderr[-2000:])
    return np.load(path)


@pytest.mark.gpu
def test_engine_agrees_with_the_fp32_stem(tmp_path):
    """The default process against ``PA_STEM_INT=0`` (a child), per producer of the model input: crops bit-identical, the same
    actions, log-probabilities within 1e-5."""
    eng = worker.make_engine()
    try:
        ours = worker.run(eng)
    finally:
        eng.close()
    old = _child(tmp_path, "0")
    for name in worker.PRODUCERS:
        assert np.array_equal(ours[f"{name}_crops"], old[f"{name}_crops"]), name
        d = np.abs(ours[f"{name}_logp"] - old[f"{name}_logp"]).max()
        print(f"{name}: max|dlogp| against PA_STEM_INT=0 = {d:.3g}")
        assert d <= 1e-5, (name, d)
        assert np.array_equal(ours[f"{name}_action_id"], old[f"{name}_action_id"]), name


@pytest.mark.gpu
@pytest.mark.parametrize("producer", list(worker.PRODUCERS))
def test_windows_and_producers_alternate_on_one_engine(engine, producer):
    """``pa_infer_windows`` (caller floats: x0 and the fp32 stem) and a producer of integer pixels, in turn on one engine: each
    reproduces its own first result bit for bit -- neither finds the other's values in its border."""
    import torch

    rng = np.random.default_rng(5)
    x = torch.from_numpy(rng.random((2, engine.S, 3, 128, 128), dtype=np.float32)).cuda()
    fn = worker.PRODUCERS[producer]
    w1 = engine.infer_windows(x).cpu().numpy()
    p1 = fn(engine)
    w2 = engine.infer_windows(x).cpu().numpy()
    p2 = fn(engine)
    w3 = engine.infer_windows(x).cpu().numpy()
    assert np.array_equal(w1, w2) and np.array_equal(w1, w3)
    for k in p1:
        assert np.array_equal(p1[k], p2[k]), (producer, k)


@pytest.mark.gpu
def test_unequal_interleaved_halves():
    """72 crops under PA_INTERLEAVE=1 (read at engine creation) run as halves of 40 and 32 on two streams: the second half's offset
    into the 8-byte-per-pixel input. Other layers' split-K choices depend on the batch, so the bar is the engine's 1e-5."""
    plain = worker.make_engine(max_batch_frames=36)
    try:
        a = worker.run_clip(plain, 36)
    finally:
        plain.close()
    saved = os.environ.get("PA_INTERLEAVE")
    os.environ["PA_INTERLEAVE"] = "1"
    try:
        inter = worker.make_engine(max_batch_frames=36)
    finally:
        if saved is None:
            del os.environ["PA_INTERLEAVE"]
        else:
            os.environ["PA_INTERLEAVE"] = saved
    try:
        b = worker.run_clip(inter, 36)
    finally:
        inter.close()
    assert np.array_equal(a["crops"], b["crops"])
    d = np.abs(a["logp"] - b["logp"]).max()
    print(f"72 crops, interleaved halves of 40 and 32: max|dlogp| = {d:.3g}")
    assert d <= 1e-5 and np.array_equal(a["action_id"], b["action_id"])
