"""``pa_synth_composite`` (``csrc/synth_composite.hip``) against its numpy twin ``synth_dataset.composite_reference``: bit-equal
bytes in both output formats over every INTER_AREA branch, alpha plane, paste offset and stage origin, several sprites and stages
in one launch, records that break every rule of the host check (the kernel is defined for any bytes: it reads them as
``synth_dataset.clamp_params`` does), and the ``out=`` argument. tests/test_synth_composite_host.py pins the twin itself."""
import numpy as np
import pytest
import torch

from playaid_core_amd import _lib
from playaid_core_amd import synth_dataset as sd

pytestmark = pytest.mark.gpu

# h x w, as tests/test_synth_composite_host.py names them: copy, 2 x 2 fast, integer fast, general (h > w; oh = 127), enlarging,
# wide copies, enlarging with one axis at scale exactly 1, and 1024 x 1000 (integer fast by 8)
SIZES = [(1, 1), (128, 128), (256, 256), (384, 384), (200, 150), (300, 301), (90, 60), (37, 128), (127, 3), (4, 128), (1024, 1000)]
ALPHAS = ["zero", "full", "random", "one", "254"]
OFFSETS = [(0, 0), (-40, 40), (40, -40), (200, 0), (-200, 0)]
STAGE_SHAPES = [(144, 160), (720, 1280)]   # (H, W)


@pytest.fixture(scope="module")
def engine():
    from playaid_core_amd import synth
    from playaid_core_amd.engine import Engine

    eng = Engine(synth.make_state_dict(seed=7), max_batch_frames=4, max_clip_frames=16, max_frame_height=128, max_frame_width=128)
    yield eng
    eng.close()


def make_sprite(h, w, alpha, seed=0):
    rng = np.random.default_rng([h, w, ALPHAS.index(alpha), seed])
    s = rng.integers(0, 256, (h, w, 4), dtype=np.uint8)
    if alpha != "random":
        s[..., 3] = {"zero": 0, "full": 255, "one": 1, "254": 254}[alpha]
    return s


def as_tree(arrays):
    return {"c": {"A": {"c00": {"r": {"90": list(arrays)}}}}}


class Banks:
    def __init__(self, engine, sprite_arrays, stage_arrays):
        self.sprite_arrays, self.stage_arrays = list(sprite_arrays), list(stage_arrays)
        self.sprites = sd.SpriteBank.from_arrays(engine, as_tree(self.sprite_arrays))
        self.stages = sd.StageBank.from_arrays(engine, self.stage_arrays)

    def close(self):
        self.sprites.close()
        self.stages.close()


@pytest.fixture(scope="module")
def stage_images():
    rng = np.random.default_rng(31)
    return [rng.integers(0, 256, (h, w, 3), dtype=np.uint8) for h, w in STAGE_SHAPES]


@pytest.fixture(scope="module")
def banks(engine, stage_images):
    """Every size with every alpha plane (sprite number = size * 5 + alpha), both stages."""
    b = Banks(engine, [make_sprite(h, w, a) for h, w in SIZES for a in ALPHAS], stage_images)
    yield b
    b.close()


def grid_records(stage_arrays, dim, sprites):
    recs = []
    for s in sprites:
        for k, st in enumerate(stage_arrays):
            H, W = st.shape[:2]
            for x, y in ((0, 0), (W - dim, H - dim)):
                recs += [(s, k, x, y, dx, dy, (0, 0)) for dx, dy in OFFSETS]
    return np.array(recs, dtype=sd.PARAMS_DTYPE)


def compare(engine, b, recs, dim=128, formats=("uint8", "model"), check=True):
    want8 = None
    for fmt in formats:
        got = sd.composite(engine, b.sprites, b.stages, recs, dim, fmt, check=check).cpu().numpy()
        want = sd.composite_reference(b.sprite_arrays, b.stage_arrays, recs, dim, fmt)
        assert got.dtype == want.dtype and got.shape == want.shape
        if not np.array_equal(got, want):
            bad = np.argwhere(got != want)
            raise AssertionError(f"{fmt}: {len(bad)} values differ, first at {bad[0]}: {got[tuple(bad[0])]} != {want[tuple(bad[0])]}")
        want8 = want if fmt == "uint8" else want8
    return want8


@pytest.mark.parametrize("size", range(len(SIZES)), ids=[f"{h}x{w}" for h, w in SIZES])
def test_every_branch_alpha_offset_and_origin(engine, banks, size):
    recs = grid_records(banks.stage_arrays, 128, range(size * 5, size * 5 + 5))
    assert len(recs) == 100 and sd.check_params(recs, banks.sprites, banks.stages, 128)
    want = compare(engine, banks, recs)
    crop0 = banks.stage_arrays[0][:128, :128]
    assert np.array_equal(want[0], crop0) and np.array_equal(want[3], crop0)   # alpha 0; off the canvas
    assert not np.array_equal(want[20], crop0)                                  # alpha 255 (the comparison is not of two untouched crops)


@pytest.mark.parametrize("dim", [32, 96, 97, 256])
def test_other_sizes_of_the_square(engine, stage_images, dim):
    """uint8 only (the model layout is 128 x 128). 97 is no multiple of 4: frames that do not start on a dword, a last quad
    that is cut. 127 x 3 resizes to an empty image at dim 32 and makes its whole bank refuse that dim."""
    sizes = [hw for hw in [(1, 1), (128, 128), (256, 256), (200, 150), (300, 301), (90, 60), (127, 3), (1024, 1000)] if sd.sprite_size(*hw, dim)[0] >= 1]
    assert len(sizes) == (7 if dim == 32 else 8)
    b = Banks(engine, [make_sprite(h, w, a, seed=dim) for h, w in sizes for a in ("random", "254")],
              [s for s in stage_images if min(s.shape[:2]) >= dim])
    try:
        recs = grid_records(b.stage_arrays, dim, range(len(b.sprite_arrays)))
        compare(engine, b, recs, dim, formats=("uint8",))
        with pytest.raises(Exception) as exc:
            sd.composite(engine, b.sprites, b.stages, recs, dim, "model")
        assert getattr(exc.value, "code", None) == _lib.PA_ERR_INVALID_ARG
    finally:
        b.close()


@pytest.mark.parametrize("n", [1, 23])
def test_mixed_sprites_and_stages_in_one_launch(engine, banks, n):
    rng = np.random.default_rng(500 + n)
    recs = np.zeros(n, dtype=sd.PARAMS_DTYPE)
    recs["sprite"] = rng.permutation(len(banks.sprite_arrays))[:n] if n > 1 else 27   # 300 x 301, random alpha
    recs["stage"] = rng.integers(0, 2, n)
    for i in range(n):
        H, W = STAGE_SHAPES[int(recs["stage"][i])]
        recs["stage_x"][i], recs["stage_y"][i] = rng.integers(0, W - 128, endpoint=True), rng.integers(0, H - 128, endpoint=True)
    recs["paste_dx"], recs["paste_dy"] = rng.integers(-60, 60, n, endpoint=True), rng.integers(-60, 60, n, endpoint=True)
    assert sd.check_params(recs, banks.sprites, banks.stages, 128)
    compare(engine, banks, recs)


def test_unchecked_records_are_read_clamped(engine, banks):
    """Records that break every rule of ``pa_synth_params_check``, launched WITHOUT the check: the launch completes and gives
    the twin's bytes for the clamped records. (Nothing here is meant to fault: the kernel is defined for these bytes.)"""
    n_sp = len(banks.sprite_arrays)
    recs = np.zeros(14, dtype=sd.PARAMS_DTYPE)
    recs["sprite"] = [27, n_sp, -1, 2 ** 31 - 1, -2 ** 31, 22, 22, 22, 22, 22, 22, 22, 22, 22]   # 22: 200 x 150, random alpha
    recs["stage"][5:9] = [2, -1, 2 ** 31 - 1, -2 ** 31]
    recs["stage"][9:] = 1
    recs["stage_x"][9:11], recs["stage_y"][9:11] = [1280 - 128 + 1, -1], [2 ** 31 - 1, -2 ** 31]
    recs["stage_x"][6], recs["stage_y"][6] = 33, 17                      # (beyond stage 0 once the stage is clamped to it)
    recs["paste_dx"][11:13], recs["paste_dy"][11:13] = [4097, -2 ** 31], [2 ** 31 - 1, -4097]
    recs["reserved"][13] = (-1, 7)
    for i in range(1, 14):
        assert not sd.check_params(recs[i:i + 1], banks.sprites, banks.stages, 128), i
    assert sd.check_params(recs[:1], banks.sprites, banks.stages, 128)
    with pytest.raises(ValueError):
        sd.composite(engine, banks.sprites, banks.stages, recs)
    rng = np.random.default_rng(78)
    junk = np.frombuffer(rng.bytes(9 * sd.PARAMS_DTYPE.itemsize), dtype=sd.PARAMS_DTYPE)   # fully random bytes as well
    both = np.concatenate([recs, junk])
    clamped = sd.clamp_params(both, banks.sprites.shapes, banks.stages.shapes, 128)
    assert sd.check_params(clamped, banks.sprites, banks.stages, 128) and not np.array_equal(clamped, both)
    got = sd.composite(engine, banks.sprites, banks.stages, both, 128, "uint8", check=False).cpu().numpy()
    assert np.array_equal(got, sd.composite_reference(banks.sprite_arrays, banks.stage_arrays, clamped, 128, "uint8"))
    compare(engine, banks, both, check=False)


def test_out_argument(engine, banks):
    recs = grid_records(banks.stage_arrays, 128, [12, 27])[:6]
    want8 = sd.composite_reference(banks.sprite_arrays, banks.stage_arrays, recs, 128, "uint8")
    wantf = sd.composite_reference(banks.sprite_arrays, banks.stage_arrays, recs, 128, "model")
    big = torch.full((10, 3, 128, 128), -1.0, dtype=torch.float32, device=engine.device)
    ret = sd.composite(engine, banks.sprites, banks.stages, recs, 128, "model", out=big[2:8])
    assert ret.data_ptr() == big[2:8].data_ptr()
    host = big.cpu().numpy()
    assert np.array_equal(host[2:8], wantf) and (host[:2] == -1).all() and (host[8:] == -1).all()   # the slice and nothing else
    big8 = torch.full((10, 128, 128, 3), 7, dtype=torch.uint8, device=engine.device)
    sd.composite(engine, banks.sprites, banks.stages, recs, 128, "uint8", out=big8[4:10])
    host8 = big8.cpu().numpy()
    assert np.array_equal(host8[4:], want8) and (host8[:4] == 7).all()
    # wrong shape, dtype or layout: refused here; a misaligned address: refused by the library
    for bad in (big[2:7], big8[2:8], big[2:8].permute(0, 1, 3, 2)):
        with pytest.raises(ValueError):
            sd.composite(engine, banks.sprites, banks.stages, recs, 128, "model", out=bad)
    flat = torch.zeros(6 * 128 * 128 * 3 + 16, dtype=torch.uint8, device=engine.device)
    for shift in (1, 4, 8):
        with pytest.raises(Exception) as exc:
            sd.composite(engine, banks.sprites, banks.stages, recs, 128, "uint8", out=flat[shift:shift + 6 * 128 * 128 * 3].view(6, 128, 128, 3))
        assert getattr(exc.value, "code", None) == _lib.PA_ERR_INVALID_ARG
    assert (flat == 0).all()


def test_library_refusals(engine, banks, stage_images):
    recs = grid_records(banks.stage_arrays, 128, [12])[:2]
    for dim in (31, 257):
        with pytest.raises(Exception):
            sd.composite(engine, banks.sprites, banks.stages, recs, dim, "uint8", check=False)
    with pytest.raises(Exception) as exc:   # 160 x 144 is smaller than 150 x 150
        sd.composite(engine, banks.sprites, banks.stages, recs, 150, "uint8", check=False)
    assert exc.value.code == _lib.PA_ERR_INVALID_ARG
    host_only = sd.StageBank.from_arrays(None, stage_images)
    with pytest.raises(Exception) as exc:
        sd.composite(engine, banks.sprites, host_only, recs, 128, "uint8")
    assert exc.value.code == _lib.PA_ERR_INVALID_ARG
    host_only.close()
