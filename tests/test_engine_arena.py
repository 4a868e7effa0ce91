"""Fold and adopt lay out the same weight arena: ``pa_create`` folds the blob into it, ``pa_create_from_arena`` (``Engine.clone()``,
the RCCL broadcast) places the same entries from the layer table alone (csrc/engine_table.h) and copies the bytes in.

Per compute dtype, an engine of 4 and of 32 frames x 2 fighters -- 8 and 64 crops, the two sides of the F(4x4, 3x3) threshold and so
the smallest engines whose arenas differ in layout: the clone's arena has the original's bytes, and two crops through
``pa_backbone_windows`` come out bit-identical on both."""
import numpy as np
import pytest
import torch

S, A = 3, 5


@pytest.fixture(scope="module")
def state_dict():
    from playaid_core_amd import synth

    return synth.make_state_dict(seed=4321, num_actions=A, sequence_length=S)


def _features(eng, x):
    feats = torch.zeros((x.shape[0], 1024), dtype=torch.float32, device=eng.device)
    eng._check(eng._lib.pa_backbone_windows(eng._h, x.data_ptr(), x.shape[0], feats.data_ptr(), eng._stream()))
    torch.cuda.synchronize(eng.device)
    return feats.cpu().numpy()


@pytest.mark.gpu
@pytest.mark.parametrize("frames", (4, 32))
@pytest.mark.parametrize("dtype", ("f32", "emulated_f32", "bf16"))
def test_clone_has_the_arena_and_the_bits(state_dict, dtype, frames):
    from playaid_core_amd.engine import Engine

    eng = Engine(state_dict, max_batch_frames=frames, max_clip_frames=8, max_frame_height=128, max_frame_width=128, compute_dtype=dtype)
    twin = eng.clone()
    try:
        a, b = eng.weights_arena().data.cpu().numpy(), twin.weights_arena().data.cpu().numpy()
        assert a.size > 20_000_000 and a.any()   # ResNet-18's eleven million conv weights, as bf16 at the least
        assert a.size == b.size and np.array_equal(a, b)
        pixels = np.random.default_rng(99).integers(0, 256, (2, 3, 128, 128)).astype(np.float32) / np.float32(255)
        x = torch.from_numpy(pixels).to(eng.device)
        fa, fb = _features(eng, x), _features(twin, x)
        assert np.abs(fa[:, :1000]).max() > 0 and np.isfinite(fa).all()
        assert np.array_equal(fa.view(np.uint32), fb.view(np.uint32))
    finally:
        twin.close()
        eng.close()
