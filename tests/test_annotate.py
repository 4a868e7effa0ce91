"""The annotator's drawing on the device (pa_annotate_frames, csrc/annotate.hip) against live Pillow, bit for bit: every frame
is seeded noise, so a wrong copy shows as much as a wrong pixel of a label. The arbiter is tests/annotate_reference.py."""
import ctypes as C
import io

import numpy as np
import pytest
from annotate_reference import noise_frames, reference_annotate

pytestmark = pytest.mark.gpu

BLUE, ORANGE, GREY = (25, 58, 115), (201, 99, 48), (55, 55, 55)
SHAPES = {"scalar": (2, 72, 100), "vector": (3, 64, 128)}  # a pitch of 300 bytes is no multiple of 16; 384 is


def draw_lists(n, h, w):
    """Per frame the box_label calls (box, label, color, draw_box, line_width). Frame 0 carries the cap of 16; with three
    frames the middle one has none."""
    full = [
        ((20, 30, 60, 50), "Dash | #3", BLUE, False, 4),                      # fits above its box
        ((5, 4, 40, 30), "Walk | #12 | active", ORANGE, False, 4),            # box[1] < 11: goes inside
        ((w - 20, 40, w - 2, 60), "ForwardSmash | #7", GREY, False, 4),       # cut by the right edge
        ((0, 50, 30, 60), "x0", BLUE, False, 4),                              # starts at column 0
        ((3, h - 20, 50, h - 5), "A" * (w // 6 + 5), ORANGE, False, 4),       # longer than the frame is wide
        ((10, h - 1, 40, h - 1), "last", GREY, True, 1),                      # a box on the last row
        ((30, 10, 70, 40), "", (250, 10, 20), True, 1),                       # roomy box, width 1 (and an empty label)
        ((60, 20, 95, 60), "", (10, 250, 20), True, 4),                       # roomy box, width 4
        ((80, 5, 82, 7), "", (10, 20, 250), True, 1),                         # 3 x 3 box, width 1
        ((90, 30, 92, 32), "", (240, 240, 10), True, 4),                      # 3 x 3 box, width 4: strokes leave the box
        ((40, 35, 50, 45), "ghost", None, False, 4),                          # color=None: white text, no background
        ((50, 45, 75, 62), "", None, True, 2),                                # color=None with a box: a WHITE outline
        ((980, 80, 1200, 60), "Frame #5", BLUE, False, 4),                    # the timer's box, wholly outside
        ((25, 66, 60, 70), "over", (1, 2, 3), False, 4),                      # two overlapping labels: the later one wins
        ((31, 69, 70, 71), "lap~", (200, 100, 0), False, 4),
        ((-7, -3, 12, 9), "neg", (90, 0, 90), True, 2),                       # negative corner
    ]
    few = [((w // 2, h // 2, w // 2 + 20, h // 2 + 9), "Jab | #1 | startup", ORANGE, True, 3), ((2, 12, 9, 20), "|", BLUE, False, 4)]
    return [full] + [[]] * (n - 2) + [few]


def annotate_on_device(frames, lists, pads, stream=None):
    import torch

    from playaid_core_amd.annotator import Annotator

    n, h, w, _ = frames.shape
    ann = Annotator(30, w, h, max_frames=n, pads=pads)
    fd = frames if isinstance(frames, torch.Tensor) else torch.from_numpy(frames).cuda()
    ann.set_frames(fd)
    for f, calls in enumerate(lists):
        for box, label, color, draw_box, lw in calls:
            ann.lw = lw
            ann.box_label(f, box, label=label, color=color, draw_box=draw_box)
    out = ann.result()
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    ann.close()
    return got


def expected(frames, lists, pads):
    out = []
    for f, calls in enumerate(lists):
        im = frames[f]
        for box, label, color, draw_box, lw in calls:  # one call at a time: each has its own line width
            im = reference_annotate(im, [(box, label, color, draw_box)], lw)
        out.append(reference_annotate(im, [], 1, pads))
    return np.stack(out)


def assert_same(got, want):
    assert got.shape == want.shape, (got.shape, want.shape)
    if not np.array_equal(got, want):
        f, y, x = np.argwhere((got != want).any(axis=3))[0]
        raise AssertionError(f"{int((got != want).any(axis=3).sum())} pixels differ; first at frame {f} row {y} column {x}: "
                             f"device {got[f, y, x].tolist()} Pillow {want[f, y, x].tolist()}")


@pytest.fixture(scope="module")
def references():
    """frames, draw lists and the Pillow result per (shape, pads): computed once."""
    cache = {}

    def get(shape, pads):
        if (shape, pads) not in cache:
            n, h, w = SHAPES[shape]
            frames = noise_frames(n, h, w, seed=h * w)
            lists = draw_lists(n, h, w)
            cache[shape, pads] = (frames, lists, expected(frames, lists, pads))
        return cache[shape, pads]

    return get


@pytest.mark.parametrize("shape,pads", [("scalar", (0, 0, 0)), ("scalar", (16, 24, 8)), ("vector", (0, 0, 0)), ("vector", (16, 24, 8)),
                                        ("vector", (400, 400, 400))])
def test_draw_lists_bit_exact_against_pillow(references, shape, pads):
    frames, lists, want = references(shape, pads)
    assert [len(c) for c in lists][0] == 16 and (len(lists) < 3 or lists[1] == [])
    assert (want[:, : frames.shape[1], pads[0]: pads[0] + frames.shape[2]] != frames).any(axis=3).sum() > 1000  # the lists do paint
    assert_same(annotate_on_device(frames, lists, pads), want)


def test_random_outlines_in_painters_order():
    """16 random outlined boxes per frame -- thin, edge-touching, partly outside -- over 24 frames, scalar and vector pitch."""
    rng = np.random.default_rng(5)
    for h, w in ((20, 25), (20, 32)):
        n = 24
        frames = noise_frames(n, h, w, seed=w)
        lists = []
        for _ in range(n):
            calls = []
            for _ in range(16):
                xs, ys = np.sort(rng.integers(-4, w + 4, 2)), np.sort(rng.integers(-4, h + 4, 2))
                calls.append(((int(xs[0]), int(ys[0]), int(xs[1]), int(ys[1])), "", tuple(int(v) for v in rng.integers(0, 256, 3)), True,
                              int(rng.integers(1, 7))))
            lists.append(calls)
        assert_same(annotate_on_device(frames, lists, (0, 0, 0)), expected(frames, lists, (0, 0, 0)))


def test_one_1080p_frame_with_manuscript_labels():
    frames = noise_frames(1, 1080, 1920, seed=1080)
    lists = [[((1171, 293, 1435, 581), "ForwardSmash | #12 | active", BLUE, False, 4), ((310, 640, 520, 930), " | #3", GREY, False, 4)]]
    got = annotate_on_device(frames, lists, (0, 0, 0))
    assert_same(got, expected(frames, lists, (0, 0, 0)))
    assert 0 < (got != frames).any(axis=3).sum() <= (27 * 6 + 2) * 13 + (5 * 6 + 2) * 13


def test_two_streams_give_what_one_after_the_other_gives():
    import torch

    from playaid_core_amd.annotator import Annotator

    n, h, w = SHAPES["vector"]
    frames = torch.from_numpy(noise_frames(n, h, w, seed=3)).cuda()
    lists_a = draw_lists(n, h, w)
    lists_b = [[((8 * f + 3, 20, 70, 50), f"stream b #{f}", ORANGE, True, 2)] for f in range(n)]
    ann = Annotator(30, w, h, max_frames=n)

    def run(lists):
        ann.set_frames(frames)
        for f, calls in enumerate(lists):
            for box, label, color, draw_box, lw in calls:
                ann.lw = lw
                ann.box_label(f, box, label=label, color=color, draw_box=draw_box)
        return ann.result()

    torch.cuda.synchronize()
    serial = [run(lists_a).cpu().numpy(), run(lists_b).cpu().numpy()]
    streams = [torch.cuda.Stream(), torch.cuda.Stream()]
    outs = []
    for s, lists in zip(streams, (lists_a, lists_b)):
        with torch.cuda.stream(s):
            outs.append(run(lists))
    torch.cuda.synchronize()
    assert np.array_equal(outs[0].cpu().numpy(), serial[0]) and np.array_equal(outs[1].cpu().numpy(), serial[1])
    assert not np.array_equal(serial[0], serial[1])
    ann.close()


def test_c_abi_rejects_bad_lists_before_any_launch():
    import torch

    from playaid_core_amd import _lib, annotator

    lib = _lib.load()
    atlas = np.ascontiguousarray(annotator.glyph_atlas())
    h = C.c_void_p(0)
    create = lambda *geometry: lib.pa_annot_create(0, atlas.ctypes.data_as(C.c_void_p), *geometry, C.byref(h))  # noqa: E731
    assert create(6, 11, 32, 95, 2, 17, 64) == _lib.PA_ERR_INVALID_ARG and not h  # max_items above the cap
    assert create(6, 11, 32, 95, 2, 16, 64) == _lib.PA_OK and h
    n, hh, ww = 2, 16, 32
    src = torch.zeros((n, hh, ww, 3), dtype=torch.uint8, device="cuda")
    dst = torch.full((n, hh, ww, 3), 7, dtype=torch.uint8, device="cuda")
    items = np.zeros((n, 16), annotator.ITEM_DTYPE)
    items[0, 0]["text_len"] = 2
    counts = np.array([1, 0], np.int32)
    text = np.frombuffer(b"ok", np.uint8).copy()

    def call(n=n, items=items, counts=counts, text=text, text_bytes=2, pads=(0, 0, 0), out=dst):
        return lib.pa_annotate_frames(h, C.c_void_p(src.data_ptr()), n, hh, ww, items.ctypes.data_as(C.c_void_p), counts.ctypes.data_as(C.c_void_p),
                                      text.ctypes.data_as(C.c_void_p), text_bytes, *pads, C.c_void_p(out.data_ptr()), None)

    assert call(counts=np.array([17, 0], np.int32)) == _lib.PA_ERR_INVALID_ARG
    assert call(counts=np.array([-1, 0], np.int32)) == _lib.PA_ERR_INVALID_ARG
    far = items.copy()
    far[0, 0]["text_off"] = 1  # 1 + 2 > 2
    assert call(items=far) == _lib.PA_ERR_INVALID_ARG
    assert call(text=np.frombuffer(b"o\n", np.uint8).copy()) == _lib.PA_ERR_INVALID_ARG  # a code outside the atlas
    assert call(text=np.frombuffer(b"o\x7f", np.uint8).copy()) == _lib.PA_ERR_INVALID_ARG
    assert call(text_bytes=65) == _lib.PA_ERR_INVALID_ARG
    assert call(pads=(-1, 0, 0)) == _lib.PA_ERR_INVALID_ARG
    assert call(out=src) == _lib.PA_ERR_INVALID_ARG
    assert call(n=3) == _lib.PA_ERR_CAPACITY
    torch.cuda.synchronize()
    assert int((dst != 7).sum()) == 0  # nothing was launched
    assert call(n=0) == _lib.PA_OK and call() == _lib.PA_OK
    torch.cuda.synchronize()
    assert int(dst[1].sum()) == 0 and int((dst[0] == 255).sum()) > 0  # the copy, and "ok" in white on it
    lib.pa_annot_destroy(h)


@pytest.mark.parametrize("skip_graphs", [True, False], ids=["unpadded", "padded"])
def test_render_writes_the_annotated_clip_byte_for_byte(tmp_path, skip_graphs):
    """Manuscript.render(output_video_path=...): Motion-JPEG in, annotated Motion-JPEG out. The encoder is pinned byte for
    byte elsewhere, so each written JPEG equals Pillow's encoding of the Pillow-annotated frame -- or the drawing is off."""
    import yaml
    from PIL import Image

    from oracle import jpeg
    from playaid_core_amd import manuscript, synth, video

    n, h, w = 8, 96, 128
    blobs = synth.encode_jpeg_frames(synth.make_frames(n, h, w, seed=7), quality=95)
    clip = str(tmp_path / "clip.avi")
    video.write_avi_mjpeg(clip, blobs, 30.0, w, h)
    boxes = synth.make_boxes(n, h, w)  # [n, 2, 4] normalised centre / size
    actions = ["Walk", "Walk", "Undefined", "Dash", "Dash", "Dash", "Walk", "ForwardSmash"]
    ai = {name: {i: {"action": actions[(i + 3 * p) % n], "crop": f"{2 + p} " + " ".join(repr(float(v)) for v in boxes[i, p]) + " 1.0",
                     "predicted_action_confidence": 1.0} for i in range(n)} for p, name in enumerate(("Pikachu", "Joker"))}
    ai_path = str(tmp_path / "ai_output.yaml")
    with open(ai_path, "w") as fh:
        yaml.safe_dump(ai, fh)
    out = str(tmp_path / "annotated.avi")
    m = manuscript.Manuscript(input_video_path=clip, ai_output_path=ai_path)
    summary = m.render(output_video_path=out, skip_graphs=skip_graphs, show_timer=True, chunk_frames=3)  # chunks of 3, 3, 2
    assert summary == manuscript.Manuscript(input_video_path=clip, ai_output_path=ai_path).render() and summary["frames"] == n
    data, spans, meta = video.read_avi_mjpeg(out)
    pads = (0, 0, 0) if skip_graphs else (400, 400, 400)
    assert len(spans) == n and (meta["width"], meta["height"]) == (w + pads[0] + pads[1], h + pads[2]) and meta["fps"] == 30.0
    fighters, seen = [], []
    for i in range(n):
        fighters = manuscript.update_fighters_from_timeline(i, m.timeline[i], fighters)
        calls = manuscript.frame_labels(i, fighters, w, h, 0, True)
        seen.append([c[1] for c in calls])
        want = reference_annotate(jpeg.decode_bgr(blobs[i]), [(box, label, color, False) for box, label, color in calls], 4, pads)
        buf = io.BytesIO()
        Image.fromarray(np.ascontiguousarray(want[..., ::-1])).save(buf, "JPEG", quality=95, subsampling=2)
        assert bytes(data[spans[i, 0]: spans[i, 1]]) == buf.getvalue(), f"frame {i}"
    assert seen[0] == ["Walk | #1", "Dash | #1", "Frame #0"] and seen[2] == [" | #1", "Dash | #3", "Frame #2"] and seen[6][0] == "Walk | #1"
