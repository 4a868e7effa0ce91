"""The device's decoder for JPEG files of mixed sizes and samplings (csrc/jpegdec.hip, playaid_core_amd/jpeg_decode.py)
against the live libjpeg-turbo behind Pillow, PIXEL FOR PIXEL: every image equals ``Image.open(file).convert("RGB")``. Then
the layers above it: chunked lists, and resuming a clip from the detector's cache directory without a decoded pixel on the
host."""
import ctypes
import io
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

SIZES = [(1, 1), (1, 9), (8, 8), (7, 9), (9, 7), (15, 16), (16, 16), (17, 33), (33, 17), (20, 3), (20, 4), (20, 5), (3, 20), (130, 2),
         (2, 130), (64, 48), (128, 128), (37, 301), (203, 151)]   # h x w
N_MIXED = 80   # 19 sizes x 4 samplings = 76 combinations, each at least once (19 and 4 are coprime)
CANARY = 256


def make_content(h, w, i):
    """Uniform noise or a smooth random walk. The cycles are decoupled (content by i // 4, sampling by i % 4, quality by i // 3,
    tables by i % 3), and every image at most 5 pixels wide or high is noise: with smooth content the replicated and the
    filtered chroma of a plane 2 samples wide round to the same pixels, and the rule would not be pinned."""
    rng = np.random.default_rng(1000 + i)
    if min(h, w) <= 5 or (i // 4) % 2:
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)   # uniform noise
    walk = np.cumsum(np.cumsum(rng.integers(-3, 4, (h, w, 3)), axis=0), axis=1) // 4 + rng.integers(40, 200, 3)   # smooth random walk
    return np.clip(walk, 0, 255).astype(np.uint8)


def make_file(i):
    """File i of the mixed batch: size, sampling (4:4:4 / 4:2:2 / 4:2:0 / grey), quality, tables and restart markers cycle."""
    from PIL import Image

    h, w = SIZES[i % len(SIZES)]
    sampling = i % 4
    rgb = make_content(h, w, i)
    kw = dict(quality=(95, 75, 30)[(i // 3) % 3], optimize=i % 3 == 0)
    if i % 10 == 1:
        kw["restart_marker_blocks"] = 3
    if i % 10 == 6:
        kw["restart_marker_rows"] = 1
    b = io.BytesIO()
    if sampling == 3:
        Image.fromarray(rgb[..., 1]).save(b, "JPEG", **kw)
    else:
        Image.fromarray(rgb).save(b, "JPEG", subsampling=sampling, **kw)
    return b.getvalue()


def pil_rgb(blob):
    from PIL import Image

    return np.asarray(Image.open(io.BytesIO(blob)).convert("RGB"))


@pytest.fixture(scope="module")
def mixed():
    """The mixed batch's files and what Pillow (live libjpeg-turbo) decodes from each, R G B."""
    blobs = [make_file(i) for i in range(N_MIXED)]
    return blobs, [pil_rgb(b) for b in blobs]


@pytest.fixture(scope="module")
def dec():
    from playaid_core_amd.jpeg_decode import JpegDecoder

    d = JpegDecoder.for_crops(96, 208, 304)
    yield d
    d.close()


def raw_decode(d, blobs, bgr=True, capacity=None, fill=None):
    """One pa_jpegdec_decode over ``blobs`` -> (rc, images uint8 host array incl. the canary, desc int64[n, 2], status)."""
    import torch

    from playaid_core_amd import _lib, jpeg_decode

    lib = _lib.load()
    n = len(blobs)
    _, total, _ = jpeg_decode.plan(blobs)
    data, spans = jpeg_decode._concat(blobs)
    cap = total if capacity is None else capacity
    images = torch.full((total + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    desc = torch.zeros((n, 2), dtype=torch.int64, device="cuda")
    status = torch.full((n,), -1, dtype=torch.int32, device="cuda")
    stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = lib.pa_jpegdec_decode(d._h, data.ctypes.data_as(ctypes.c_void_p), spans.ctypes.data_as(ctypes.c_void_p), n, int(bgr),
                               ctypes.c_void_p(images.data_ptr()), cap, ctypes.c_void_p(desc.data_ptr()),
                               ctypes.c_void_p(status.data_ptr()), stream)
    torch.cuda.synchronize()
    return rc, images.cpu().numpy(), desc.cpu().numpy(), status.cpu().numpy()


def image_of(images, desc, i):
    off, h, w = int(desc[i, 0]), int(desc[i, 1] & 0xFFFFFFFF), int(desc[i, 1] >> 32)
    return images[off: off + h * w * 3].reshape(h, w, 3)


def test_mixed_batch_is_bit_exact(dec, mixed):
    """One call over 80 files of 19 sizes, four samplings, three qualities, optimised tables and restart markers on some:
    every image equals Pillow's, in both channel orders; statuses 0; descriptors = the plan; nothing behind images_bytes."""
    from playaid_core_amd import _lib, jpeg_decode

    blobs, want = mixed
    hdesc, total, _ = jpeg_decode.plan(blobs)
    for bgr in (True, False):
        rc, images, desc, status = raw_decode(dec, blobs, bgr=bgr)
        assert rc == _lib.PA_OK
        assert np.array_equal(desc, hdesc)
        assert not status.any(), np.nonzero(status)[0]
        bad = [i for i in range(len(blobs)) if not np.array_equal(image_of(images, desc, i), want[i][..., ::-1] if bgr else want[i])]
        assert not bad, [(i, SIZES[i % len(SIZES)], i % 4) for i in bad]
        assert (images[total:] == 0xA5).all()


def test_spans_in_any_order_repeated_and_empty(dec, mixed):
    from playaid_core_amd import _lib

    blobs, want = mixed
    order = list(range(len(blobs)))[::-1]
    order[3:3] = [order[10]]
    order[40:40] = [order[0]]
    blobs2 = [blobs[i] for i in order]
    want2 = [want[i] for i in order]
    for at in (0, 17, len(blobs2)):
        blobs2.insert(at, None)
        want2.insert(at, np.zeros((0, 0, 3), np.uint8))
    # the files stay where they are in memory, only the spans move: spans in any order, two repeated, three empty
    import torch

    from playaid_core_amd import jpeg_decode

    lib = _lib.load()
    data, spans = jpeg_decode._concat(blobs)
    sp2 = np.zeros((len(blobs2), 2), np.int64)
    k = 0
    for j, b in enumerate(blobs2):
        if b is None:
            sp2[j] = (5, 5)
        else:
            sp2[j] = spans[order[k]]
            k += 1
    _, total, _ = jpeg_decode.plan(blobs2)
    images = torch.full((total + CANARY,), 0xA5, dtype=torch.uint8, device="cuda")
    desc = torch.zeros((len(blobs2), 2), dtype=torch.int64, device="cuda")
    status = torch.full((len(blobs2),), -1, dtype=torch.int32, device="cuda")
    rc = lib.pa_jpegdec_decode(dec._h, data.ctypes.data_as(ctypes.c_void_p), sp2.ctypes.data_as(ctypes.c_void_p), len(blobs2), 1,
                               ctypes.c_void_p(images.data_ptr()), total, ctypes.c_void_p(desc.data_ptr()),
                               ctypes.c_void_p(status.data_ptr()), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream))
    torch.cuda.synchronize()
    assert rc == _lib.PA_OK, lib.pa_jpegdec_last_error(dec._h)
    images, desc, status = images.cpu().numpy(), desc.cpu().numpy(), status.cpu().numpy()
    assert not status.any()
    for j, w in enumerate(want2):
        got = image_of(images, desc, j)
        assert got.shape == w.shape and np.array_equal(got, w[..., ::-1]), j
    assert (images[total:] == 0xA5).all()


def test_agrees_with_the_frame_decoder(dec):
    """Eight 48 x 64 4:2:0 files through pa_jpegdec_decode and through pa_mjpeg_decode: identical bytes."""
    import torch

    from playaid_core_amd import _lib, synth, video

    frames = synth.make_frames(8, 48, 64, seed=3)
    blobs = synth.encode_jpeg_frames(frames, quality=95)
    md = video.MjpegDecoder(max_frames=8, max_height=48, max_width=64, max_bytes=1 << 20)
    try:
        data = np.frombuffer(b"".join(blobs), np.uint8)
        ends = np.cumsum([len(b) for b in blobs])
        spans = np.stack([ends - [len(b) for b in blobs], ends], axis=1)
        st = torch.zeros(8, dtype=torch.int32, device="cuda")
        ref = md.decode(data, spans, 48, 64, status=st)
        torch.cuda.synchronize()
        ref = ref.cpu().numpy()
        assert not st.cpu().numpy().any()
    finally:
        md.close()
    rc, images, desc, status = raw_decode(dec, blobs)
    assert rc == _lib.PA_OK and not status.any()
    assert np.array_equal(images[: 8 * 48 * 64 * 3].reshape(8, 48, 64, 3), ref)


def test_limits_and_a_corrupt_stream(mixed):
    from playaid_core_amd import _lib, jpeg_decode
    from playaid_core_amd.jpeg_decode import JpegDecoder

    lib = _lib.load()
    blobs, want = mixed
    few = blobs[:8]
    _, total, blocks = jpeg_decode.plan(few)
    d = JpegDecoder(8, blocks, 1 << 20)
    short = JpegDecoder(8, blocks - 1, 1 << 20)
    try:
        rc, images, _, status = raw_decode(d, few)
        assert rc == _lib.PA_OK and not status.any()   # the handle is exactly large enough
        for handle, bl, cap in ((d, blobs[:9], None), (d, few, total - 16), (short, few, None)):
            rc, images, _, status = raw_decode(handle, bl, capacity=cap)
            assert rc == _lib.PA_ERR_CAPACITY, rc
            assert b"pa_jpegdec_decode" in lib.pa_jpegdec_last_error(handle._h)
            assert (images == 0xA5).all() and (status == -1).all()   # nothing was enqueued
    finally:
        d.close()
        short.close()
    # one image's entropy-coded second half replaced by another file's scan bytes: header intact, stream valid-looking but
    # wrong. The call succeeds, the other eleven are bit-exact, nothing is written outside the images.
    rng = np.random.default_rng(77)
    from PIL import Image

    files = []
    for i in range(12):
        b = io.BytesIO()
        Image.fromarray(rng.integers(0, 256, (64, 48, 3), dtype=np.uint8)).save(b, "JPEG", quality=95, subsampling=(0, 2)[i % 2])
        files.append(b.getvalue())
    info = (ctypes.c_int32 * 8)()
    why = ctypes.create_string_buffer(128)

    def scan_off(blob):
        buf = np.frombuffer(blob, np.uint8)
        assert lib.pa_mjpeg_probe(buf.ctypes.data_as(ctypes.c_void_p), len(blob), info, why, 128) == _lib.PA_OK
        return info[6]

    victim, donor = files[5], files[2]
    so, do = scan_off(victim), scan_off(donor)
    half = so + (len(victim) - 2 - so) // 2
    nrep = len(victim) - 2 - half
    assert len(donor) - 2 - do >= nrep
    bad = victim[:half] + donor[do: do + nrep] + victim[-2:]
    assert len(bad) == len(victim) and bad != victim
    batch = files[:5] + [bad] + files[6:]
    d = JpegDecoder.for_crops(12, 64, 48)
    try:
        rc, images, desc, status = raw_decode(d, batch)
        assert rc == _lib.PA_OK
        _, total, _ = jpeg_decode.plan(batch)
        for i in range(12):
            if i != 5:
                assert status[i] == 0 and np.array_equal(image_of(images, desc, i), pil_rgb(files[i])[..., ::-1]), i
        assert (images[total:] == 0xA5).all()
    finally:
        d.close()


def test_chunked_lists_equal_one_call(mixed):
    """40 files through a handle of 16 images (three consecutive calls on one output buffer) and through one of 64."""
    from playaid_core_amd.jpeg_decode import JpegDecoder

    blobs, want = mixed
    blobs = [b if i % 9 != 4 else None for i, b in enumerate(blobs[20:60])]
    outs = []
    for cap in (16, 64):
        d = JpegDecoder.for_crops(cap, 208, 304)
        try:
            images, desc, status = d.decode_files(blobs)
            outs.append((images.cpu().numpy(), desc.cpu().numpy(), status.cpu().numpy()))
        finally:
            d.close()
    assert np.array_equal(outs[0][1], outs[1][1]) and not outs[0][2].any() and not outs[1][2].any()
    for i, b in enumerate(blobs):   # (image by image: the bytes that pad an image to 16 are nobody's)
        got, one = image_of(outs[0][0], outs[0][1], i), image_of(outs[1][0], outs[1][1], i)
        assert np.array_equal(got, one), i
        if b is None:
            assert got.shape == (0, 0, 3)
        else:
            assert np.array_equal(got, want[20 + i][..., ::-1]), i
    with pytest.raises(ValueError, match="image 1"):
        d2 = JpegDecoder.for_crops(4, 64, 64)
        try:
            d2.decode_files([blobs[0], blobs[0][:100]])
        finally:
            d2.close()


RES_N, RES_H, RES_W = 40, 360, 640


def test_resume_from_a_cache_decoded_on_the_device(tmp_path):
    """A cache directory written by ai_cache.write_detector_cache (40 frames, the second fighter missing on the last three),
    three crop files replaced by the 128 x 128 4:2:0 files the reference's repair leaves: the runner over
    ClipSource.from_cache(decoder=...) gives bit for bit the results of the host (Pillow) path on the same model."""
    import torch
    from PIL import Image

    from playaid_core_amd import ai_cache, constants, synth
    from playaid_core_amd.ai_runner import AIRunner, ClipSource
    from playaid_core_amd.anim_ontology import MOVE_TO_CLASS_ID
    from playaid_core_amd.cnn_action_detector import CNNActionDetector
    from playaid_core_amd.jpeg_decode import JpegDecoder
    from playaid_core_amd.jpeg_encode import JpegEncoder, coded_blocks

    n, h, w = RES_N, RES_H, RES_W
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
    ckpt = str(tmp_path / "seeded.ckpt")
    synth.save_checkpoint(ckpt, seed=1234)
    model = CNNActionDetector.load_from_checkpoint(ckpt, actions=list(MOVE_TO_CLASS_ID.keys()), max_batch_frames=64, max_clip_frames=512,
                                                   max_frame_height=h, max_frame_width=w)
    out = str(tmp_path / "cache")
    enc = JpegEncoder(2 * n, 2 * n * coded_blocks(h, w, 0))
    try:
        done = ai_cache.write_detector_cache(model.engine, enc, torch.from_numpy(frames).cuda(), torch.from_numpy(dets).cuda(),
                                             torch.from_numpy(counts).cuda(), out, "clip")
    finally:
        enc.close()
    assert done == {"labels": n, "crops": 2 * n - 3}
    rng = np.random.default_rng(9)
    for i, p in ((4, 0), (5, 0), (17, 1)):   # what cv2.imwrite leaves for a repaired gap: 128 x 128, quality 95, 4:2:0
        path = os.path.join(out, "crops", constants.CHAR_LIST[2 + p], f"clip_{i + 1}.jpg")
        assert os.path.exists(path)
        Image.fromarray(rng.integers(0, 256, (128, 128, 3), dtype=np.uint8)).save(path, quality=95, subsampling=2)
    video_path = str(tmp_path / "clip.avi")
    host = AIRunner(ClipSource.from_cache(video_path, out), model=model, output_dir=str(tmp_path / "out_host"))
    host.run_action_recognition()
    dec = JpegDecoder.for_crops(2 * n, h, w)
    try:
        clip = ClipSource.from_cache(video_path, out, decoder=dec)
        assert clip.crop_images is None and clip.packed_crops[0].is_cuda and clip.frames.shape == (n, 0, 0, 3)
        hd = clip.packed_crops[2]
        assert hd.shape == (n, 2, 2) and (hd[n - 3:, 1, 1] == 0).all() and (hd[:, 0, 1] != 0).all()
        assert int(hd[4, 0, 1]) == (128 << 32) | 128
        dev = AIRunner(clip, model=model, output_dir=str(tmp_path / "out_dev"))
        dev.run_action_recognition()
        # a file the decoder does not take is named by its path
        bad = os.path.join(out, "crops", constants.CHAR_LIST[2], "clip_7.jpg")
        Image.fromarray(frames[0][:32, :32]).save(bad, progressive=True)
        with pytest.raises(ValueError, match="clip_7.jpg"):
            ClipSource.from_cache(video_path, out, decoder=dec)
    finally:
        dec.close()
    a, b = host._results, dev._results
    assert np.array_equal(a["action_id"], b["action_id"])
    assert np.array_equal(a["prob"], b["prob"])
    assert np.array_equal(a["crops_rgb"], b["crops_rgb"])
    assert host.ai_output_data.to_dict() == dev.ai_output_data.to_dict()
    assert len(dev.ai_output_data[dev.fighters[0]]) == n - 1
