"""``pa_augment_crops`` (``csrc/augment.hip``) against its numpy twin ``augment.augment_reference``: bit-equal bytes in both
output formats -- every stage alone at its extremes, everything at once, and records that break every rule of the host check
(the kernel is defined for any bytes: it reads them as ``augment.clamp_params`` does)."""
import numpy as np
import pytest
import torch

from playaid_core_amd import augment

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from playaid_core_amd import synth
    from playaid_core_amd.engine import Engine

    eng = Engine(synth.make_state_dict(seed=7), max_batch_frames=4, max_clip_frames=16, max_frame_height=128, max_frame_width=128)
    yield eng
    eng.close()


@pytest.fixture(scope="module")
def source():
    """Five fixed-seed noise crops (one of them smooth, so that hue and saturation vary slowly), one all 0 and one all 255."""
    rng = np.random.default_rng(2024)
    src = rng.integers(0, 256, (7, 128, 128, 3), dtype=np.uint8)
    yy, xx = np.mgrid[0:128, 0:128]
    src[4] = np.stack([(xx * 2) % 256, (yy * 2) % 256, (xx + yy) % 256], -1).astype(np.uint8)
    src[5], src[6] = 0, 255
    return src


def _compare(engine, source, params, check=True):
    src_dev = torch.from_numpy(source).to(engine.device)
    for fmt in ("uint8", "model"):
        got = augment.augment_crops(engine, src_dev, params, fmt, check=check).cpu().numpy()
        want = augment.augment_reference(source, params, fmt)
        assert got.dtype == want.dtype and got.shape == want.shape
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{fmt}: {len(bad)} values differ, first at {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")
    return augment.augment_reference(source, params, "uint8")


def _each(source, **fields):
    """One record per source crop, identity but for ``fields``."""
    p = augment.identity_params(len(source))
    for k, v in fields.items():
        p[k] = v
    p["key"] = np.arange(len(source), dtype=np.uint64) * np.uint64(0x9E3779B97F4A7C15) + np.uint64(1 << 40)
    return p


STAGES = {
    "flip": dict(flip=1),
    "bc_low": dict(alpha=0.8, beta=-0.2),
    "bc_high": dict(alpha=1.2, beta=0.4),
    "blur2": dict(blur_k=2),
    "blur3": dict(blur_k=3),
    "blur2_flip": dict(blur_k=2, flip=1),
    "hue_-256_sat_67": dict(hue_shift=-256, sat_shift=67),
    "hue_0_sat_-67": dict(hue_shift=0, sat_shift=-67),
    "hue_179.5_sat_67": dict(hue_shift=179.5, sat_shift=67),
    "hue_256_sat_-67": dict(hue_shift=256, sat_shift=-67),
    "val_5": dict(val_shift=5),
    "val_-5": dict(val_shift=-5),
    "noise": dict(noise_sigma=np.float32(np.sqrt(200.0))),
    "pixel_dropout": dict(pixel_drop_thr=int(0.3 * 2 ** 32)),
    "channel_001": dict(channel_mask=0b001),
    "channel_110": dict(channel_mask=0b110),
}


@pytest.mark.parametrize("name", sorted(STAGES))
def test_each_stage_alone(engine, source, name):
    p = _each(source, **STAGES[name])
    assert augment.check_params(p, len(source))
    want = _compare(engine, source, p)
    for i in range(4):   # (the stage did something: the comparison above is not one of two untouched copies)
        assert not np.array_equal(want[i], source[i])
    if name.startswith("blur"):   # the border rows and columns (first and last of each) are blurred through the reflected border
        plain = augment.augment_reference(source[:1], _each(source[:1], flip=STAGES[name].get("flip", 0)))[0]
        for edge, was in ((want[0, 0], plain[0]), (want[0, -1], plain[-1]), (want[0, :, 0], plain[:, 0]), (want[0, :, -1], plain[:, -1])):
            assert not np.array_equal(edge, was)


def test_holes(engine, source):
    p = _each(source, n_holes=8)
    p["holes"][:] = [(0, 0), (124, 124), (0, 124), (124, 0), (60, 61), (62, 63), (3, 3), (100, 7)]
    p["n_holes"][1] = 1
    want = _compare(engine, source, p)
    assert (want[0, 124:, 124:] == 0).all() and (want[0, :4, :4] == 0).all() and (want[1, 124:, 124:] == source[1, 124:, 124:]).all()


@pytest.mark.parametrize("scale,side,start", [(0.7, None, 0), (0.9, None, 0), (None, 89, 0), (None, 89, 39), (None, 126, 1), (0.8, 100, 17)])
def test_geometry(engine, source, scale, side, start):
    p = _each(source)
    p["xmap"] = augment.compose_map(scale, side, start)
    p["ymap"] = augment.compose_map(scale, side, 0 if side is None else 128 - side - start)
    assert augment.check_params(p, len(source))
    _compare(engine, source, p)


@pytest.mark.parametrize("n", [1, 3, 40])
def test_everything_at_once(engine, source, n):
    rng = np.random.default_rng(100 + n)
    src = np.concatenate([rng.permutation(len(source)), rng.integers(0, len(source), 40)])[:n]   # a permutation, then repeats
    on = {"horizontal_flip": 1.0, "downscale": 1.0, "resize": 1.0, "course_dropout": 1.0, "channel_dropout": 1.0, "pixel_dropout": 1.0,
          "gauss_noise": 1.0}
    p = augment.sample_params(n, on, rng, src=src)
    p["alpha"], p["beta"] = 1 + rng.uniform(-0.2, 0.2, n), rng.uniform(-0.2, 0.4, n)
    p["blur_k"] = rng.choice([2, 3], n)
    assert augment.check_params(p, len(source))
    _compare(engine, source, p)


def test_sampled_levels(engine, source):
    for level in (1, 2):
        rng = np.random.default_rng(level)
        _compare(engine, source, augment.sample_params(24, level, rng, src=rng.integers(0, len(source), 24)))


def test_identity_in_model_layout_is_the_datasets_division(engine, source):
    src_dev = torch.from_numpy(source).to(engine.device)
    got = augment.augment_crops(engine, src_dev, augment.identity_params(len(source)), "model").cpu()
    assert torch.equal(got, torch.from_numpy(source).permute(0, 3, 1, 2).float() / 255)
    got8 = augment.augment_crops(engine, src_dev, augment.identity_params(len(source)), "uint8").cpu()
    assert torch.equal(got8, torch.from_numpy(source))


def test_unchecked_records_are_read_clamped(engine, source):
    """Records that break every rule of ``pa_augment_params_check``, launched WITHOUT the check: the launch completes and gives
    the twin's bytes for the clamped records. (Nothing here is meant to fault: the kernel is defined for these bytes.)"""
    n_src = len(source)
    rng = np.random.default_rng(77)
    p = augment.sample_params(16, 2, rng, src=rng.integers(0, n_src, 16))
    p["src"][:4] = [n_src, -1, 2 ** 31 - 1, -2 ** 31]
    p["xmap"][1] = rng.integers(0, 256, 128)
    p["ymap"][2] = rng.integers(128, 256, 128)
    p["n_holes"][3], p["n_holes"][4], p["n_holes"][5] = 9, -3, 8
    p["holes"][3], p["holes"][5] = 125, rng.integers(0, 256, (8, 2))
    p["blur_k"][6], p["blur_k"][7] = 4, -2
    p["alpha"][8], p["beta"][8] = np.nan, np.inf
    p["alpha"][9], p["beta"][9] = 1e30, -1e30
    p["hue_shift"][10], p["sat_shift"][10], p["val_shift"][10] = np.inf, np.nan, -np.inf
    p["hue_shift"][11], p["sat_shift"][11], p["val_shift"][11] = 1e9, -300.0, 300.0
    p["noise_sigma"][12], p["noise_sigma"][13], p["noise_sigma"][14] = np.nan, -4.0, 1e6
    p["channel_mask"][14], p["flip"][14] = 0xFFFF, 7
    p["channel_mask"][15] = 8
    for i in range(16):
        assert not augment.check_params(p[i:i + 1], n_src), i
    with pytest.raises(ValueError):
        augment.augment_crops(engine, torch.from_numpy(source).to(engine.device), p)
    # a fully random block of bytes as well
    junk = np.frombuffer(rng.bytes(8 * augment.PARAMS_DTYPE.itemsize), dtype=augment.PARAMS_DTYPE)
    _compare(engine, source, np.concatenate([p, junk]), check=False)
