"""The device's baseline JPEG encoder (csrc/jpegenc.hip, playaid_core_amd/jpeg_encode.py) against the live libjpeg-turbo
behind Pillow, BYTE FOR BYTE: every file ``JpegEncoder`` writes equals ``Image.fromarray(rgb).save(format="JPEG",
quality=q, subsampling=s)`` of the same pixels. Then the layers above it: Motion-JPEG clips written from the device and
read back by the device's decoder, and the detector's crop cache (playaid_core_amd/ai_cache.py) as files."""
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (8, 8), (7, 9), (16, 16), (17, 23), (33, 40), (128, 128), (64, 49), (100, 75), (9, 130)]   # h x w
CONTENTS = ("noise", "gradient", "constant", "blocky")
QUALITIES = (95, 100, 75, 20)
SAMPLINGS = (0, 2)


def make_image(h, w, content, seed):
    rng = np.random.default_rng(seed)
    if content == "noise":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if content == "gradient":
        y, x = np.mgrid[0:h, 0:w]
        return np.stack([x * 255 // max(w - 1, 1), y * 255 // max(h - 1, 1), (x + y) * 255 // max(h + w - 2, 1)], -1).astype(np.uint8)
    if content == "constant":
        return np.broadcast_to(np.array([200, 30, 90], np.uint8), (h, w, 3)).copy()
    cells = rng.integers(0, 256, (-(-h // 8), -(-w // 8), 3), dtype=np.uint8)   # blocky: one colour per 8 x 8 cell
    return np.repeat(np.repeat(cells, 8, 0), 8, 1)[:h, :w].copy()


def pil_jpeg(rgb, quality, subsampling):
    from PIL import Image

    b = io.BytesIO()
    Image.fromarray(rgb).save(b, format="JPEG", quality=quality, subsampling=subsampling)
    return b.getvalue()


def count_ff00(blob):
    d = np.frombuffer(blob, np.uint8)[623:-2]
    return int(np.count_nonzero((d[:-1] == 0xFF) & (d[1:] == 0)))


@pytest.fixture(scope="module")
def image_set():
    """The 40 images (10 sizes x 4 contents, R G B) and Pillow's file of each for every quality and sampling."""
    imgs = [make_image(h, w, c, 100 + 7 * i + j) for i, (h, w) in enumerate(SIZES) for j, c in enumerate(CONTENTS)]
    ref = {(q, s): [pil_jpeg(im, q, s) for im in imgs] for q in QUALITIES for s in SAMPLINGS}
    return imgs, ref


def pack(imgs, device, bgr):
    """Images back to back at offsets that are NOT aligned (one byte of slack more per image)."""
    import torch

    offs, pos = [], 3
    for i, im in enumerate(imgs):
        offs.append(pos)
        pos += im.size + 1 + (i % 5)
    buf = np.full(pos + 16, 0x5A, np.uint8)
    for off, im in zip(offs, imgs):
        buf[off: off + im.size] = (im[..., ::-1] if bgr else im).reshape(-1)
    desc = np.array([[off, (im.shape[1] << 32) | im.shape[0]] for off, im in zip(offs, imgs)], np.int64)
    return torch.from_numpy(buf).to(device), torch.from_numpy(desc).to(device)


@pytest.fixture(scope="module")
def encoder():
    from playaid_core_amd.jpeg_encode import JpegEncoder, coded_blocks

    blocks = sum(max(coded_blocks(h, w, 0), coded_blocks(h, w, 2)) for h, w in SIZES) * len(CONTENTS)
    enc = JpegEncoder(64, blocks, scratch_bytes=1 << 20)
    yield enc
    enc.close()


def encode_set(enc, imgs, q, s, bgr, **kw):
    images, desc = pack(imgs, enc.device, bgr)
    return enc.encode_images(images, desc, 128, 130, quality=q, subsampling=s, bgr=bgr, **kw)


def test_reference_set_exercises_stuffing_and_zero_runs(image_set):
    """A pass of the byte comparison below cannot hide an untested path: Pillow's own files of the set hold >= 1000
    stuffed FF 00 pairs, and at least one block with a run of >= 16 zeros in front of a non-zero coefficient (ZRL)."""
    from oracle import jpeg as oj

    imgs, ref = image_set
    assert sum(count_ff00(f) for files in ref.values() for f in files) >= 1000
    zz = oj.ZIGZAG
    found = False
    for s in SAMPLINGS:
        for blob in ref[(20, s)]:
            _, planes = oj.decode_coefficients(blob)
            for pl in planes:
                c = pl.reshape(-1, 64)[:, zz]
                nz = c != 0
                for row in nz[nz[:, 17:].any(1)]:
                    idx = np.flatnonzero(row)
                    idx = idx[idx > 0]
                    if len(idx) and np.max(np.diff(np.concatenate([[0], idx]))) > 16:
                        found = True
                        break
    assert found, "no block of the quality-20 files needs a ZRL code"


@pytest.mark.parametrize("bgr", [True, False])
@pytest.mark.parametrize("subsampling", SAMPLINGS)
@pytest.mark.parametrize("quality", QUALITIES)
def test_bytes_equal_pillow(image_set, encoder, quality, subsampling, bgr):
    """All 40 images of mixed sizes in ONE call: every file byte-identical to Pillow's, every length exact, the files in
    input order at 16-byte aligned offsets."""
    from playaid_core_amd.jpeg_encode import JpegEncoder

    imgs, ref = image_set
    files, rec = encode_set(encoder, imgs, quality, subsampling, bgr)
    got = JpegEncoder.unpack_files(files, rec)
    r = rec.cpu().numpy()
    want = ref[(quality, subsampling)]
    assert [int(v) for v in r[:, 1].astype(np.int32)] == [len(f) for f in want]
    assert (r[:, 0] % 16 == 0).all() and (np.diff(r[:, 0]) == [(len(f) + 15) // 16 * 16 for f in want[:-1]]).all()
    for i, (g, f) in enumerate(zip(got, want)):
        assert g == f, f"image {i} ({imgs[i].shape}): first difference at byte {next(k for k in range(min(len(g), len(f))) if g[k] != f[k]) if g[:len(f)] != f[:len(g)] else 'length'}"
    assert encoder.overflows() == 0


def test_empty_entries_and_bad_descriptors(image_set, encoder):
    """height = width = 0 gives nbytes 0; an image larger than the call's max size or outside the buffer gives -1 and is
    counted; the others of the call are untouched by either."""
    import torch

    from playaid_core_amd.jpeg_encode import JpegEncoder

    imgs, ref = image_set
    images, desc = pack(imgs[:6], encoder.device, True)
    d = desc.cpu().numpy().copy()
    d[1, 1] = 0                              # empty
    d[3, 1] = (131 << 32) | 20               # wider than max_width
    d[4, 0] = images.numel() - 10            # runs past the buffer
    files, rec = encoder.encode_images(images, torch.from_numpy(d).to(encoder.device), 128, 130, quality=95, subsampling=0)
    got = JpegEncoder.unpack_files(files, rec)
    assert got[1] == b"" and got[3] is None and got[4] is None
    for i in (0, 2, 5):
        assert got[i] == ref[(95, 0)][i]
    assert encoder.overflows() == 2 and encoder.overflows() == 0


@pytest.mark.parametrize("hw", [(1080, 1920), (720, 1280)])
def test_large_frames_equal_pillow(hw):
    """Whole synthetic frames, 4:2:0 at quality 95 through ``encode_frames``: tens of thousands of blocks, many scan tiles;
    1080 rows leave the last MCU row half empty (240 dummy luma blocks)."""
    from playaid_core_amd import synth
    from playaid_core_amd.jpeg_encode import JpegEncoder

    h, w = hw
    frame = synth.make_frames(1, h, w)   # BGR
    enc = JpegEncoder.for_frames(1, h, w, 2)
    try:
        got = enc.encode_frames(frame, quality=95, subsampling=2, bgr=True)
    finally:
        enc.close()
    want = pil_jpeg(np.ascontiguousarray(frame[0][..., ::-1]), 95, 2)
    assert len(got) == 1 and len(got[0]) == len(want) and got[0] == want


def test_round_trip_through_the_device_decoder(tmp_path):
    """136 x 200 frames (no multiple of 16): encode_frames -> MjpegDecoder.decode equals the oracle's round trip of the same
    pixels; write_frames_mjpeg -> VideoCapture.read_frames gives the same arrays."""
    import torch

    from oracle import jpeg as oj
    from playaid_core_amd import synth, video
    from playaid_core_amd.jpeg_encode import JpegEncoder

    frames = synth.make_frames(3, 136, 200)   # BGR
    want = np.stack([oj.roundtrip_any(np.ascontiguousarray(f[..., ::-1]), 95, 2)[..., ::-1] for f in frames])
    enc = JpegEncoder.for_frames(3, 136, 200, 2)
    try:
        files = enc.encode_frames(torch.from_numpy(frames).cuda(), quality=95, subsampling=2, bgr=True)
    finally:
        enc.close()
    data = np.frombuffer(b"".join(files), np.uint8)
    spans = np.concatenate([[0], np.cumsum([len(f) for f in files])]).astype(np.int64)
    dec = video.MjpegDecoder(3, 136, 200, max(data.size, 1024) + 4096)
    try:
        dec.set_sync_rounds(0)   # exact mode: verify passes until nothing changes
        got = dec.decode(data, spans, 136, 200)
        torch.cuda.synchronize()
        assert np.array_equal(got.cpu().numpy(), want)
    finally:
        dec.close()
    path = str(tmp_path / "clip.avi")
    assert video.write_frames_mjpeg(path, torch.from_numpy(frames).cuda(), 30.0) == files
    cap = video.VideoCapture(path)
    assert cap.isOpened() and cap.frame_count() == 3
    back = cap.read_frames(0, 3, exact=True)
    torch.cuda.synchronize()
    assert np.array_equal(back.cpu().numpy(), want)
    cap.release()


def _aligned(n):
    return (n + 15) // 16 * 16


def test_capacity_of_the_file_buffer(image_set, encoder):
    """files_capacity cut to the first 25 files: those records and bytes are unchanged, the other 15 get nbytes -1 and are
    counted, and the bytes behind the capacity stay untouched."""
    import torch

    from playaid_core_amd.jpeg_encode import JpegEncoder

    imgs, ref = image_set
    want = ref[(95, 0)]
    cap = sum(_aligned(len(f)) for f in want[:25])
    whole = torch.full((cap + 65536,), 0xA5, dtype=torch.uint8, device=encoder.device)
    files, rec = encode_set(encoder, imgs, 95, 0, True, files=whole[:cap])
    got = JpegEncoder.unpack_files(files, rec)
    assert got[:25] == want[:25] and all(g is None for g in got[25:])
    assert (rec.cpu().numpy()[25:, 1].astype(np.int32) == -1).all()
    assert encoder.overflows() == 15
    assert bool((whole[cap:] == 0xA5).all())


def test_capacity_of_the_stream_scratch(image_set):
    """The same with a handle whose scratch holds the un-stuffed streams of the first 25 images only."""
    import torch

    from playaid_core_amd.jpeg_encode import JpegEncoder, coded_blocks

    imgs, ref = image_set
    want = ref[(95, 0)]
    streams = [len(f) - 625 - count_ff00(f) for f in want]
    scratch = sum((s + 63) // 64 * 64 for s in streams[:25])
    assert scratch >= 1024
    enc = JpegEncoder(64, sum(coded_blocks(h, w, 0) for h, w in SIZES) * len(CONTENTS), scratch_bytes=scratch)
    try:
        whole = torch.full((sum(_aligned(len(f)) for f in want) + 4096,), 0xA5, dtype=torch.uint8, device=enc.device)
        files, rec = encode_set(enc, imgs, 95, 0, True, files=whole[:-4096])
        got = JpegEncoder.unpack_files(files, rec)
        assert got[:25] == want[:25] and all(g is None for g in got[25:])
        assert enc.overflows() == 15
        used = sum(_aligned(len(f)) for f in want[:25])
        assert bool((whole[used:] == 0xA5).all())
    finally:
        enc.close()


def test_same_bytes_on_another_stream(image_set, encoder):
    """The OR atomics that merge neighbouring blocks' words do not depend on their order: two runs on two streams give
    identical buffers, mixed sizes and uniform frames alike."""
    import torch

    from playaid_core_amd import synth
    from playaid_core_amd.jpeg_encode import JpegEncoder

    imgs, ref = image_set
    outs = []
    for _ in range(2):
        st = torch.cuda.Stream()
        with torch.cuda.stream(st):
            files, rec = encode_set(encoder, imgs, 75, 2, True)
            uni = encoder.encode_frames(synth.make_frames(2, 72, 104), quality=95, subsampling=2)
        st.synchronize()
        outs.append((JpegEncoder.unpack_files(files, rec), rec.cpu().numpy().copy(), uni))
    assert outs[0][0] == outs[1][0] == ref[(75, 2)] and np.array_equal(outs[0][1], outs[1][1]) and outs[0][2] == outs[1][2]


# ---- the detector's crop cache as files ---------------------------------------------------------------------------------

CACHE_N, CACHE_H, CACHE_W = 24, 360, 640


@pytest.fixture(scope="module")
def cache_clip():
    """A synthetic 24-frame 360 x 640 clip and the label rows a detector would have written for its two fighters (rounded
    pixel boxes -> xyxy2xywh / gn in float32, classes 2 / 3, as tests/test_savebox.py builds them): both fighters on every
    frame, except that the second one is missing on the last three (a tail, no interior gap)."""
    from playaid_core_amd import synth

    n, h, w = CACHE_N, CACHE_H, CACHE_W
    F32 = np.float32
    frames = synth.make_frames(n, h, w)
    boxes = synth.make_boxes(n, h, w)
    dets = np.zeros((n, 2, 6), F32)
    counts = np.full(n, 2, np.int32)
    for i in range(n):
        for p in range(2):
            cx, cy, bw, bh = boxes[i, p] * np.array([w, h, w, h])
            x1, y1, x2, y2 = np.rint([cx - bw / 2, cy - bh / 2, cx + bw / 2, cy + bh / 2]).clip(0, [w, h, w, h]).astype(F32)
            xywh = np.array([(x1 + x2) / F32(2), (y1 + y2) / F32(2), x2 - x1, y2 - y1], F32)
            dets[i, p] = np.concatenate([[2 + p], (xywh / np.array([w, h, w, h], F32)).astype(F32), [0.9 - 0.01 * p]]).astype(F32)
    counts[n - 3:] = 1
    dets[n - 3:, 1] = 0
    return frames, dets, counts


def _cache_encoder(engine):
    from playaid_core_amd.jpeg_encode import JpegEncoder, coded_blocks

    k = 2 * CACHE_N
    return JpegEncoder(k, k * coded_blocks(CACHE_H, CACHE_W, 0))


def test_cache_files_equal_the_in_memory_round_trip(engine, cache_clip, tmp_path):
    """write_detector_cache: every crop file decodes (Pillow = the library behind cv2.imread) to exactly the image
    pa_save_one_box_crops(jpeg_quality=95) holds for that (frame, fighter); its bytes are Pillow's save of the oracle's raw
    rectangle; the label files parse back to the table's rows; a class's second detection in a frame gets the
    increment_path name."""
    import torch
    from PIL import Image

    from oracle import detect as odet
    from playaid_core_amd import ai_cache, constants
    from playaid_core_amd.ai_runner import read_fighter_yolo_crop_text

    frames, dets, counts = cache_clip
    n, h, w = CACHE_N, CACHE_H, CACHE_W
    fd, dd, cd = torch.from_numpy(frames).cuda(), torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
    out = str(tmp_path / "cache")
    enc = _cache_encoder(engine)
    try:
        done = ai_cache.write_detector_cache(engine, enc, fd, dd, cd, out, "clip")
        assert done == {"labels": n, "crops": 2 * n - 3}
        images, desc = engine.save_one_box_crops(fd, dd, cd, jpeg_quality=95)
        engine.check_device_errors()
        held = engine.unpack_crop_images(images, desc)
        for i in range(n):
            text = open(os.path.join(out, "labels", f"clip_{i + 1}.txt")).read()
            for p in range(2):
                fighter = constants.CHAR_LIST[2 + p]
                path = os.path.join(out, "crops", fighter, f"clip_{i + 1}.jpg")
                crop = read_fighter_yolo_crop_text(text, fighter)
                if p >= counts[i]:
                    assert not os.path.exists(path) and held[i * 2 + p] is None and crop is None
                    continue
                row = dets[i, p]
                want_row = [float("%g" % float(v)) for v in row]
                assert [crop.class_id, crop.center_x, crop.center_y, crop.crop_width, crop.crop_height, crop.confidence] == want_row
                blob = open(path, "rb").read()
                x1, y1, x2, y2 = odet.save_one_box_rect(row, (h, w))
                assert blob == pil_jpeg(np.ascontiguousarray(frames[i][y1:y2, x1:x2][..., ::-1]), 95, 0), (i, p)
                got = np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))[..., ::-1]
                assert np.array_equal(got, held[i * 2 + p]), (i, p)
        # three detections in a frame, two of one class: one crop slot per DETECTION, the second file takes the counter
        d3 = np.zeros((2, 3, 6), np.float32)
        d3[:, :2] = dets[:2]
        d3[1, 2] = dets[5, 0]
        c3 = np.array([2, 3], np.int32)
        out3 = str(tmp_path / "cache3")
        done = ai_cache.write_detector_cache(engine, enc, fd[:2], torch.from_numpy(d3).cuda(), torch.from_numpy(c3).cuda(), out3, "clip")
        assert done == {"labels": 2, "crops": 5}
        a = constants.CHAR_LIST[2]
        assert sorted(os.listdir(os.path.join(out3, "crops", a))) == ["clip_1.jpg", "clip_2.jpg", "clip_22.jpg"]
        x1, y1, x2, y2 = odet.save_one_box_rect(d3[1, 2], (h, w))
        assert open(os.path.join(out3, "crops", a, "clip_22.jpg"), "rb").read() == \
            pil_jpeg(np.ascontiguousarray(frames[1][y1:y2, x1:x2][..., ::-1]), 95, 0)
        assert len(open(os.path.join(out3, "labels", "clip_2.txt")).read().splitlines()) == 3
    finally:
        enc.close()


def test_resume_from_the_cache_gives_the_chains_records(engine, cache_clip, tmp_path):
    """Detector stage here, the rest from the files: AIRunner(ClipSource.from_cache(...)) yields the records (action ids, and
    confidences bit for bit) of detector_path.run_detections_to_labels on the same frames and table."""
    import torch

    from playaid_core_amd import ai_cache, synth
    from playaid_core_amd.ai_runner import AIRunner, ClipSource
    from playaid_core_amd.anim_ontology import MOVE_TO_CLASS_ID
    from playaid_core_amd.cnn_action_detector import CNNActionDetector
    from playaid_core_amd.detector_path import run_detections_to_labels

    frames, dets, counts = cache_clip
    n, h, w = CACHE_N, CACHE_H, CACHE_W
    fd, dd, cd = torch.from_numpy(frames).cuda(), torch.from_numpy(dets).cuda(), torch.from_numpy(counts).cuda()
    out = str(tmp_path / "cache")
    enc = _cache_encoder(engine)
    try:
        ai_cache.write_detector_cache(engine, enc, fd, dd, cd, out, "clip")
    finally:
        enc.close()
    want = run_detections_to_labels(engine, fd, dd, cd, jpeg_quality=95)
    assert want["max_frames"] == n
    ckpt = str(tmp_path / "seeded.ckpt")
    synth.save_checkpoint(ckpt, seed=1234)
    model = CNNActionDetector.load_from_checkpoint(ckpt, actions=list(MOVE_TO_CLASS_ID.keys()), max_batch_frames=64, max_clip_frames=512,
                                                   max_frame_height=h, max_frame_width=w, compute_dtype=engine.compute_dtype)
    runner = AIRunner(ClipSource.from_cache(str(tmp_path / "clip.avi"), out), model=model, output_dir=str(tmp_path / "out"))
    assert runner.max_frames == n and runner.clip.frames.shape == (n, 0, 0, 3)
    runner.run_action_recognition()
    res = runner._results
    assert np.array_equal(res["action_id"][: n - 1], want["action_id"][: n - 1])
    assert np.array_equal(res["prob"][: n - 1], want["prob"][: n - 1])
    for p, fighter in enumerate(runner.fighters):
        for f in range(1, n):
            rec = runner.ai_output_data[fighter][f - 1]
            assert rec.action == model.actions[int(want["action_id"][f - 1, p])]
            assert rec.predicted_action_confidence == float(want["prob"][f - 1, p]) * 100.0
