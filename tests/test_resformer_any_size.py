"""``ResnetTransformerDetector(crop_size=...)``: the reference's transformer model on crops of another size than 128 (its own
driver feeds it 256 x 256) against ``oracle.resformer.forward``, which is size-agnostic (adaptive pool). Bars: those of
tests/test_resformer_detector.py -- 1e-4 on the log-probabilities, 1e-4 * max(1, max|want|) on the pooled features."""
import numpy as np
import pytest
import torch

from oracle import resformer as oracle_rf
from playaid_core_amd import synth

pytestmark = pytest.mark.gpu

TOL = 1e-4
ACTIONS = [f"a{i}" for i in range(63)]

_want = {}


@pytest.fixture(scope="module")
def rf_sd():
    return synth.make_resformer_state_dict(seed=2468, num_actions=63, sequence_length=3)


def _inputs(b, s, c, seed=5):
    rng = np.random.default_rng([seed, c])
    return torch.from_numpy(rng.integers(0, 256, size=(b, s, 3, c, c)).astype(np.float32) / 255.0)


def _oracle(c, rf_sd):
    """The oracle's features and log-probabilities for the [2, 3, 3, c, c] input, once per size (shared by both dtypes)."""
    if c not in _want:
        x = _inputs(2, 3, c)
        _want[c] = (x, oracle_rf.resnet50_features(x.reshape(6, 3, c, c), rf_sd).numpy(), oracle_rf.forward(x, rf_sd).numpy())
    return _want[c]


@pytest.mark.parametrize("crop_size", [96, 256])
@pytest.mark.parametrize("dtype", ["f32", "emulated_f32"])
def test_sized_resformer_detector_matches_oracle(rf_sd, dtype, crop_size):
    from playaid_core_amd.resnet_transformer_detector import ResnetTransformerDetector

    c = crop_size
    x, want_f, want = _oracle(c, rf_sd)
    model = ResnetTransformerDetector(ACTIONS, sequence_length=3, state_dict=rf_sd, crop_size=c, compute_dtype=dtype).eval()
    try:
        assert model.crop_size == c
        got_f = model._net.forward(x.reshape(6, 3, c, c)).cpu().numpy()
        err_f = np.abs(got_f - want_f).max()
        print(f"crop_size {c} {dtype}: features max|err| {err_f:.3g} (max|want| {np.abs(want_f).max():.3g}); forms {sorted(set(model._net.layer_forms()))}")
        assert err_f <= 1e-4 * max(1.0, np.abs(want_f).max())
        got = model(x).numpy()
        assert got.shape == (2, 3, 63)
        err = np.abs(got - want).max()
        print(f"crop_size {c} {dtype}: log-probabilities max|err| {err:.3g}")
        assert err <= TOL, err
        assert (got.argmax(2) == want.argmax(2)).all()
        assert model._net.layer_forms()[0] == "stem_pool_any"
        with pytest.raises(ValueError):
            model(_inputs(2, 3, 128))       # this model takes c x c crops
        # test_step / metrics on top of it, unchanged: every (window, slot) row scored against its label
        labels = torch.from_numpy(want.argmax(2).astype(np.int64))
        labels[0, 0] = (labels[0, 0] + 1) % 63
        model.reset_metrics()
        model.test_step((x, torch.zeros(2, dtype=torch.int64), labels, None), 0)
        m = model.metrics("test")
        assert abs(m["test_action_acc"] - 5 / 6) <= 1e-6
        nll = -np.take_along_axis(want.reshape(6, 63), labels.reshape(6, 1).numpy(), 1).mean()
        assert abs(m["test_action_loss"] - nll) <= 1e-3
    finally:
        model.close()


def test_crop_size_128_is_the_detector_without_the_argument(rf_sd):
    from playaid_core_amd.resnet_transformer_detector import ResnetTransformerDetector

    x = _inputs(2, 3, 128)
    a = ResnetTransformerDetector(ACTIONS, sequence_length=3, state_dict=rf_sd, max_rows=6).eval()
    b = ResnetTransformerDetector(ACTIONS, sequence_length=3, state_dict=rf_sd, max_rows=6, crop_size=128).eval()
    try:
        ya, yb = a(x), b(x)
        assert torch.equal(ya, yb)
        assert a._net.layer_forms() == b._net.layer_forms() and a._net.layer_forms()[0] == "stem_pool"
        assert a.crop_size == b.crop_size == 128
    finally:
        a.close()
        b.close()


def test_refused_sizes_and_dtypes(rf_sd):
    from playaid_core_amd.resnet_transformer_detector import ResnetTransformerDetector

    with pytest.raises(ValueError, match="bf16"):
        ResnetTransformerDetector(ACTIONS, sequence_length=3, state_dict=rf_sd, crop_size=256, compute_dtype="bf16")
    for bad in (100, 32, 544):
        with pytest.raises(ValueError, match="multiple of 32"):
            ResnetTransformerDetector(ACTIONS, sequence_length=3, state_dict=rf_sd, crop_size=bad)
