"""Square crops of any output size on the device (``pa_square_crops_sized``, csrc/crop_sized.hip) against the oracle's
``yolo_crop.square_crop(image, box, output_size, padding)``, bit for bit, and the Python surfaces on top of it
(``Engine.square_crops(output_size=)``, ``YoloCrop.square_crop(output_size=)``, ``ClipWindowDataset(crop_size=)``).

Per size S the square sides d are chosen to take every branch of ``cv2.resize(INTER_AREA)`` to (S, int(d * (S / float(d)))):
d < S (fixed-point bilinear emulation; S - 1 next to the copy), d == S (copy), S < d with a fractional scale (general shrink:
S + 37, 2 S + 91, 640), d = 2 S (2 x 2), d = 3 S (integer scale), and two sides whose height comes out as S - 1 (black last
row) -- each at a centre that is inside, clipped at a corner, clipped at one edge, or on the frame's edge, with the reference's
padding (30: the engine's cached Pillow tables) and with none (tables computed per crop). No case may report a capacity status.
"""
import ctypes as C

import numpy as np
import pytest
import torch

from playaid_core_amd import synth

pytestmark = pytest.mark.gpu

SIZES = (64, 96, 200, 256)
CENTRES = ((0.5, 0.5), (0.02, 0.04), (0.985, 0.97), (0.5, 0.99), (0.0, 0.5))
OFF_SCREEN = (1.6, 0.5, 0.15, 0.3)
SHORT = {64: (49, 103), 96: (47, 147), 200: (97, 167), 256: (49, 103)}   # first and third d in 30..700 with int(d * (S / float(d))) == S - 1

_cache = {}


def sides(size):
    short = [d for d in range(30, 701) if int(d * (size / float(d))) == size - 1]
    assert (short[0], short[2]) == SHORT[size]
    return [max(24, size // 2 - 3), size - 1, size, size + 37, 2 * size, 2 * size + 91, 3 * size if 3 * size <= 700 else 640, 640,
            short[0], short[2]]


def frames_720():
    if "f720" not in _cache:
        _cache["f720"] = synth.make_frames(6, 720, 1280, seed=11)
    return _cache["f720"]


def cases(size, pad):
    """-> boxes float64[6, 2, 4]: the ten sides at the cycling centres, then the off-screen box, then one more inside box."""
    h, w = 720, 1280
    boxes = np.zeros((6, 2, 4))
    for k, d in enumerate(sides(size)):
        cx, cy = CENTRES[k % len(CENTRES)]
        boxes[k // 2, k % 2] = (cx, cy, (d + 0.5) / w, (0.8 * d + 0.5) / h)
    boxes[5, 0] = OFF_SCREEN
    boxes[5, 1] = (0.4, 0.6, (size + 0.5) / w, (size + 0.5) / h)
    return boxes


def oracle_crops(key, frames, boxes, size, pad):
    """The oracle's answer for every (frame, slot), computed once per case set and shared by both engine dtypes."""
    from oracle import yolo_crop

    if key not in _cache:
        _cache[key] = [[yolo_crop.square_crop(frames[i], boxes[i, p], size, padding=pad) for p in range(boxes.shape[1])]
                       for i in range(boxes.shape[0])]
    return _cache[key]


def sized_raw(engine, frames, boxes, pad, size, swap_rb=False):
    """``pa_square_crops_sized`` itself (``Engine.square_crops`` calls the 128 kernels at 128)."""
    from playaid_core_amd.engine import _ptr

    fd = torch.from_numpy(np.ascontiguousarray(frames)).to(engine.device)
    bd = torch.from_numpy(np.ascontiguousarray(boxes, dtype=np.float64)).to(engine.device)
    n, h, w, _ = fd.shape
    crops = torch.full((n, engine.F, size, size, 3), 0xA5, dtype=torch.uint8, device=engine.device)
    status = torch.full((n, engine.F), -1, dtype=torch.int32, device=engine.device)
    rc = engine._lib.pa_square_crops_sized(engine._h, _ptr(fd), n, h, w, _ptr(bd), pad, int(swap_rb), size, _ptr(crops), _ptr(status),
                                           C.c_void_p(torch.cuda.current_stream(engine.device).cuda_stream))
    assert rc == 0, engine._lib.pa_last_error(engine._h)
    torch.cuda.synchronize()
    return crops.cpu().numpy(), status.cpu().numpy()


@pytest.mark.parametrize("pad", [30, 0])
@pytest.mark.parametrize("size", SIZES)
def test_sized_crops_bit_exact_720p(engine, size, pad):
    frames = frames_720()
    boxes = cases(size, pad)
    crops, status = engine.square_crops(frames, boxes, padding=pad, output_size=size)
    assert crops.shape == (6, 2, size, size, 3) and crops.dtype == np.uint8
    want = oracle_crops(("720", size, pad), frames, boxes, size, pad)
    ds = sides(size)
    for k in range(10):
        i, p = k // 2, k % 2
        ok, ref = want[i][p]
        assert ok, (size, pad, ds[k])
        assert status[i, p] == 0, f"S={size} pad={pad} d={ds[k]} centre={CENTRES[k % 5]}: status {status[i, p]}"
        assert np.array_equal(crops[i, p], ref), (f"S={size} pad={pad} d={ds[k]} centre={CENTRES[k % 5]}: "
                                                  f"{int((crops[i, p] != ref).sum())} bytes differ, max {np.abs(crops[i, p].astype(int) - ref).max()}")
    # off screen: with the padding the slice is (d + 60) x 0, the reference returns (False, None), and the failed crop is all zero;
    # without padding it is d x 0, which ImageOps.pad turns into a black d x d canvas without resizing: ok, and all zero too
    ok_off, ref_off = want[5][0]
    assert ok_off == (pad == 0) and (ref_off is None or not ref_off.any())
    assert (status[5, 0] == 0) == ok_off and not crops[5, 0].any()
    assert want[5][1][0] and status[5, 1] == 0 and np.array_equal(crops[5, 1], want[5][1][1])
    # a second identical call returns identical bytes
    crops2, status2 = engine.square_crops(frames, boxes, padding=pad, output_size=size)
    assert np.array_equal(crops, crops2) and np.array_equal(status, status2)
    # the channel swap reverses the channels and nothing else
    sw, st = engine.square_crops(frames[:2], boxes[:2], padding=pad, swap_rb=True, output_size=size)
    assert np.array_equal(sw, crops[:2, :, :, :, ::-1]) and np.array_equal(st, status[:2])


@pytest.mark.parametrize("size", SIZES)
def test_sized_crops_bit_exact_1080p(engine, size):
    from oracle import yolo_crop

    h, w = 1080, 1920
    if "f1080" not in _cache:
        _cache["f1080"] = synth.make_frames(1, h, w, seed=13)
    frame = _cache["f1080"]
    ds = (size, 2 * size, 700)
    frames = np.repeat(frame, 2, axis=0)
    boxes = np.zeros((2, 2, 4))
    for k, d in enumerate(ds + (size,)):
        boxes[k // 2, k % 2] = (0.5, 0.5, (d + 0.5) / w, (0.8 * d + 0.5) / h)
    crops, status = engine.square_crops(frames, boxes, padding=30, output_size=size)
    for k, d in enumerate(ds):
        key = ("1080", size, d)
        if key not in _cache:
            _cache[key] = yolo_crop.square_crop(frame[0], boxes[k // 2, k % 2], size, padding=30)
        ok, ref = _cache[key]
        assert ok and status[k // 2, k % 2] == 0, (size, d, status)
        assert np.array_equal(crops[k // 2, k % 2], ref), (size, d)


@pytest.mark.parametrize("hw", [(1080, 1920), (720, 1280)])
def test_sized_entry_at_128_equals_the_128_kernels(engine, hw):
    """``pa_square_crops_sized(output_size=128)`` against ``pa_square_crops``, byte for byte, on the boxes of
    tests/test_gpu_parity.py::test_square_crops_bit_exact (clipped, off-screen, integer scales, d == 128, huge)."""
    h, w = hw
    n = 6
    frames = synth.make_frames(n, h, w, seed=11)
    boxes = synth.make_boxes(n, h, w)
    boxes[0, 0] = (0.03, 0.05, 0.16, 0.30)
    boxes[0, 1] = (0.97, 0.96, 0.15, 0.28)
    boxes[1, 0] = (1.6, 0.5, 0.15, 0.3)
    boxes[1, 1] = (0.5, 0.5, 0.30, 0.20)
    boxes[2, 0] = (0.5, 0.5, 256.5 / w, 200.5 / h)
    boxes[2, 1] = (0.4, 0.6, 128.5 / w, 100.5 / h)
    boxes[3, 0] = (0.5, 0.5, 384.5 / w, 300.5 / h)
    boxes[3, 1] = (0.5, -0.4, 0.15, 0.3)
    boxes[4, 0] = (0.5, 0.5, 0.5, 0.9)
    boxes[4, 1] = (0.3, 0.6, 0.6, 0.5)
    want, want_status = engine.square_crops(frames, boxes, padding=30)        # the 128 x 128 kernels
    got, status = sized_raw(engine, frames, boxes, 30, 128)
    assert np.array_equal(status, want_status) and (status == 0).sum() >= 9
    assert np.array_equal(got, want)
    again, _ = engine.square_crops(frames, boxes, padding=30)                 # and the 128 path is as it was after a sized call
    assert np.array_equal(again, want)


def test_sized_entry_refuses_sizes_outside_its_range(engine):
    from playaid_core_amd import _lib
    from playaid_core_amd.engine import _ptr

    fd = torch.zeros((1, 64, 64, 3), dtype=torch.uint8, device=engine.device)
    bd = torch.zeros((1, engine.F, 4), dtype=torch.float64, device=engine.device)
    out = torch.zeros((engine.F * 600 * 600 * 3,), dtype=torch.uint8, device=engine.device)
    st = torch.zeros((engine.F,), dtype=torch.int32, device=engine.device)
    for bad in (15, 513, 0, -128):
        assert engine._lib.pa_square_crops_sized(engine._h, _ptr(fd), 1, 64, 64, _ptr(bd), 0, 0, bad, _ptr(out), _ptr(st), None) == _lib.PA_ERR_INVALID_ARG
    for edge in (16, 512):
        assert engine._lib.pa_square_crops_sized(engine._h, _ptr(fd), 1, 64, 64, _ptr(bd), 0, 0, edge, _ptr(out), _ptr(st), None) == _lib.PA_OK
    torch.cuda.synchronize()
    with pytest.raises(ValueError):
        engine.square_crops(np.zeros((1, 64, 64, 3), np.uint8), np.zeros((1, 2, 4)), output_size=8)
    with pytest.raises(ValueError):
        engine.square_crops(np.zeros((1, 64, 64, 3), np.uint8), np.zeros((1, 2, 4)), output_size=600)


def test_smallest_and_largest_sizes_match_the_oracle(engine):
    """The ends of the range, and an odd size: 16, 333 and 512 on one clipped and one inside box each."""
    from oracle import yolo_crop

    frames = frames_720()[:1]
    h, w = 720, 1280
    boxes = np.array([[(0.5, 0.5, 300.5 / w, 200.5 / h), (0.02, 0.97, 90.5 / w, 100.5 / h)]])
    for size in (16, 333, 512):
        crops, status = engine.square_crops(frames, boxes, padding=30, output_size=size)
        for p in range(2):
            key = ("ends", size, p)
            if key not in _cache:
                _cache[key] = yolo_crop.square_crop(frames[0], boxes[0, p], size, padding=30)
            ok, ref = _cache[key]
            assert ok and status[0, p] == 0 and np.array_equal(crops[0, p], ref), (size, p)


def test_yolo_crop_square_crop_takes_an_output_size(engine):
    from oracle import yolo_crop
    from playaid_core_amd.fighter import YoloCrop

    frame = frames_720()[2]
    box = (0.47, 0.55, 0.21, 0.52)
    yc = YoloCrop(*box)
    ok, got = yc.square_crop(frame, output_size=256, padding=30, engine=engine)
    want_ok, want = yolo_crop.square_crop(frame, box, 256, padding=30)
    assert ok and want_ok and got.shape == (256, 256, 3) and np.array_equal(got, want)
    ok, got = yc.square_crop(frame, padding=30, engine=engine)            # the default is the 128 path, as ever
    assert ok and np.array_equal(got, yolo_crop.square_crop(frame, box, 128, padding=30)[1])
    assert YoloCrop(*OFF_SCREEN).square_crop(frame, output_size=256, padding=30, engine=engine) == (False, None)
    for bad in (8, 600):
        with pytest.raises(ValueError):
            yc.square_crop(frame, output_size=bad, padding=30, engine=engine)


def test_square_crops_device_takes_an_output_size(engine):
    frames = frames_720()[:3]
    boxes = cases(96, 30)[:3]
    want, want_status = engine.square_crops(frames, boxes, padding=30, output_size=96)
    fd = torch.from_numpy(frames).to(engine.device)
    bd = torch.from_numpy(np.ascontiguousarray(boxes[:, 0])).to(engine.device)
    out = torch.zeros((3, 96, 96, 3), dtype=torch.uint8, device=engine.device)
    st = engine.square_crops_device(fd, bd, out, padding=30, output_size=96)
    torch.cuda.synchronize()
    assert np.array_equal(out.cpu().numpy(), want[:, 0]) and np.array_equal(st.cpu().numpy(), want_status[:, 0])
    with pytest.raises(ValueError):
        engine.square_crops_device(fd, bd, out, padding=30, output_size=128)   # out is 96 x 96


def test_clip_window_dataset_cuts_crops_of_another_size(engine, state_dict, tmp_path):
    from oracle import yolo_crop
    from playaid_core_amd.ai_runner import AIRunner, ClipSource
    from playaid_core_amd.anim_ontology import MOVE_TO_CLASS_ID
    from playaid_core_amd.cnn_action_detector import CNNActionDetector
    from playaid_core_amd.dataset_utils import action_sample_from_frame_middle_out
    from playaid_core_amd.ult_action_dataset import ClipWindowDataset

    actions = list(MOVE_TO_CLASS_ID.keys())
    model = CNNActionDetector(actions, state_dict=state_dict, max_batch_frames=32, max_clip_frames=64, max_frame_height=270,
                              max_frame_width=480, compute_dtype=engine.compute_dtype).eval()
    try:
        runner = AIRunner(ClipSource.synthetic(24, 270, 480), model=model, output_dir=str(tmp_path / "a"), crop_mode="square")
        n_per = runner.max_frames - 1
        gt = [[actions[(f * 7 + 3 * p) % len(actions)] for f in range(1, runner.max_frames)] for p in range(2)]
        ds96 = ClipWindowDataset(runner, actions=gt, crop_size=96)
        ds128 = ClipWindowDataset(runner, actions=gt)
        assert ds96.crop_size == 96 and ds128.crop_size == 128 and len(ds96) == len(ds128) == n_per * 2
        boxes, src, _ = runner._boxes()
        s = runner.num_frames_per_sample
        for idx in (0, 5, n_per - 1, n_per + 7):
            p, frame_num = idx // n_per, 1 + idx % n_per
            x, char_id, action_ids, meta = ds96[idx]
            assert x.shape == (s, 3, 96, 96) and x.dtype == torch.float32
            nums = action_sample_from_frame_middle_out(frame_num, num_frames_per_sample=s, frame_delta=runner.frame_delta,
                                                       max_frames=runner.max_frames, min_frame=1)
            got = (x * 255).round().byte().permute(0, 2, 3, 1).numpy()
            for j, f in enumerate(nums):
                ok, ref = yolo_crop.square_crop(runner.clip.frames[src[f - 1, p]], boxes[f - 1, p], 96, padding=model.engine.cfg.crop_padding)
                assert ok and np.array_equal(got[j], ref[:, :, ::-1]), (idx, f)     # RGB, like the 128 dataset's crops
                assert np.array_equal(meta["frames"][j], ref[:, :, ::-1])
            x128, char128, ids128, meta128 = ds128[idx]
            assert x128.shape == (s, 3, 128, 128)
            assert int(char_id) == int(char128) and torch.equal(action_ids, ids128)
            assert meta["actions"] == meta128["actions"] and meta["frame_paths"] == meta128["frame_paths"] and meta["char"] == meta128["char"]
        xb, cb, ab, metas = next(ds96.batches(4))
        assert xb.shape == (4, s, 3, 96, 96) and ab.shape == (4, s)
        # a clip that holds crop files only has nothing to cut another size from
        files_only = ClipSource(np.zeros((24, 0, 0, 3), np.uint8), runner.clip.labels, "files",
                                crop_images=[[np.zeros((40, 30, 3), np.uint8)] * 2 for _ in range(24)])
        r2 = AIRunner(files_only, model=model, output_dir=str(tmp_path / "b"))
        with pytest.raises(ValueError, match="frames are needed"):
            ClipWindowDataset(r2, crop_size=96)
        assert ClipWindowDataset(r2).crop_size == 128
        with pytest.raises(ValueError):
            ClipWindowDataset(runner, crop_size=8)
    finally:
        model.engine.close()
