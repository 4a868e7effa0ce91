"""Host side of the annotator (playaid_core_amd/annotator.py, manuscript.py's label building): the glyph atlas and the outline
rule against LIVE Pillow, the pure label function on a hand-written timeline, the argument checks, the ABI. No GPU."""
import json
import os
import re

import numpy as np
import pytest
from click.testing import CliRunner
from PIL import Image, ImageDraw, ImageFont

from playaid_core_amd import _lib, annotator, fighter as fighter_mod, manuscript, synth

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PRINTABLE = [chr(c) for c in range(32, 127)]


@pytest.fixture(scope="module")
def atlas():
    return annotator.glyph_atlas()


@pytest.fixture(scope="module")
def font():
    return ImageFont.load_default_imagefont()


def live_mask(font, s):
    m = font.getmask(s)
    return np.frombuffer(bytes(m), np.uint8).reshape(m.size[1], m.size[0])


def test_atlas_geometry_is_the_bitmap_fonts(atlas, font):
    assert atlas.shape == (95, 96, 11, 6) and atlas.dtype == np.uint8
    assert set(np.unique(atlas)) == {0, 255}  # no blending arithmetic: a text pixel is the ink or untouched
    assert font.getbbox("ForwardSmash | #12 | hitstun")[2:] == (6 * 28, 11)  # what the removed getsize returned


def test_atlas_reproduces_getmask_on_every_pair_and_single(atlas, font):
    for a in PRINTABLE:
        assert np.array_equal(annotator.text_mask(atlas, a), live_mask(font, a)), a
        for b in PRINTABLE:
            assert np.array_equal(annotator.text_mask(atlas, a + b), live_mask(font, a + b)), a + b
    # the quirk the table exists for: a cell's last column depends on what follows
    assert any(not np.array_equal(atlas[c, n], atlas[c, 95]) for c in range(95) for n in range(95))
    assert np.array_equal(atlas[:, :95, :, :5], np.repeat(atlas[:, 95:, :, :5], 95, axis=1))  # columns 0-4 never do


def test_atlas_reproduces_getmask_on_random_strings(atlas, font):
    rng = np.random.default_rng(20261018)
    for _ in range(500):
        s = "".join(chr(c) for c in rng.integers(32, 127, rng.integers(1, 41)))
        assert np.array_equal(annotator.text_mask(atlas, s), live_mask(font, s)), s


def _pillow_outlines(boxes, width, size):
    """bool[len(boxes), size, size]: what ImageDraw.rectangle(outline=, width=) paints for each box, on the RGBA image the
    reference draws on."""
    im = Image.new("RGBA", (size, size))
    draw = ImageDraw.Draw(im)
    out = bytearray()
    for b in boxes:
        draw.rectangle((0, 0, size, size), fill=(0, 0, 0, 0))
        draw.rectangle(b, outline=(255, 255, 255), width=width)
        out += im.getchannel(0).tobytes()
    return np.frombuffer(bytes(out), np.uint8).reshape(len(boxes), size, size) != 0


# corners on a 20 x 20 grid: the whole 20 x 20 image (boxes touching its edges), and the same grid shifted by -5 over a 10 x 10
# image (boxes partly and wholly outside). Pillow refuses x1 < x0 / y1 < y0, so every ORDERED box: 44100 per grid and width.
@pytest.mark.parametrize("size,lo", [(20, 0), (10, -5)], ids=["inside", "outside"])
def test_outline_rule_equals_live_pillow_on_every_box(size, lo):
    grid = range(lo, lo + 20)
    rows = [(a, b) for a in grid for b in grid if a <= b]
    checked = 0
    for width in (1, 2, 3, 4, 6):
        for x0 in grid:
            boxes = [(x0, y0, x1, y1) for x1 in range(x0, lo + 20) for y0, y1 in rows]
            want = _pillow_outlines(boxes, width, size)
            arr = np.array(boxes, np.int32)
            got = annotator.outline_mask(arr.T, np.full(len(arr), width, np.int32), size, size)
            bad = np.flatnonzero((got != want).any(axis=(1, 2)))
            assert bad.size == 0, f"width {width}, box {boxes[bad[0]]}: rule\n{got[bad[0]].astype(int)}\nPillow\n{want[bad[0]].astype(int)}"
            checked += len(boxes)
    assert checked == 5 * 210 * 210


def test_outline_counts_of_the_two_known_boxes():
    # a roomy box: nested one-pixel frames; a thin one: the vertical strokes leave the box (20 pixels at width 4, not 16)
    assert [int(annotator.outline_mask((5, 6, 30, 20), w, 40, 40).sum()) for w in (1, 2, 4, 6)] == [78, 148, 264, 348]
    m = annotator.outline_mask((5, 6, 8, 9), 4, 40, 40)
    assert int(m.sum()) == 20 and m[10:, :].any()
    assert np.array_equal(m, _pillow_outlines([(5, 6, 8, 9)], 4, 40)[0])


# ---- labels ------------------------------------------------------------------------------------------------------------

class _Crop:
    def __init__(self, box):
        self.box = box

    def xyxy_pixels(self, w, h):
        return self.box


class _Fighter:
    def __init__(self, fighter_id, action, frame, anim_state="", hitstun_left=0, box=(10, 20, 30, 40)):
        self.fighter_id, self.action, self.animation_frame_num, self.anim_state = fighter_id, action, frame, anim_state
        self.hitstun_left, self.crop = hitstun_left, _Crop(box)


def test_frame_labels_on_a_hand_written_timeline():
    a = _Fighter(0, "ForwardSmash", 12, anim_state="active", box=(100, 200, 180, 300))
    b = _Fighter(1, "Undefined", 3, hitstun_left=7, box=(0, 5, 40, 90))
    c = _Fighter(4, "", 1)
    assert manuscript.fighter_label(a) == "ForwardSmash | #12 | active"
    assert manuscript.fighter_label(b) == " | #3"
    assert manuscript.fighter_label(c) == " | #1"
    assert manuscript.fighter_label(_Fighter(1, "Dash", 2)) == "Dash | #2"
    calls = manuscript.frame_labels(7, [a, b, c], 1920, 1080)
    assert calls == [((100, 200, 180, 300), "ForwardSmash | #12 | active", (25, 58, 115)),
                     ((0, 5, 40, 90), " | #3", (55, 55, 55)),  # hitstun: grey
                     ((10, 20, 30, 40), " | #1", (201, 99, 48))]
    # show_timer: one more label at the reference's fixed box, coloured like the LAST fighter (its table colour even in hitstun)
    timed = manuscript.frame_labels(7, [a, b], 1920, 1080, log_offset=5, show_timer=True)
    assert timed[:2] == calls[:2] and timed[2] == ((980, 80, 1200, 60), "Frame #12", (201, 99, 48))
    # a negative log_offset skips the fighters' labels of the first frames; the timer stays, clamped at 0, in the FIRST fighter's colour
    assert manuscript.frame_labels(2, [a, b], 1920, 1080, log_offset=-3, show_timer=True) == [((980, 80, 1200, 60), "Frame #0", (25, 58, 115))]
    assert manuscript.frame_labels(2, [a, b], 1920, 1080, log_offset=-3) == []
    assert manuscript.frame_labels(3, [a, b], 1920, 1080, log_offset=-3) == calls[:2]
    assert manuscript.frame_labels(3, [], 1920, 1080, show_timer=True) == []


def test_anim_state_follows_the_frame_data_table(monkeypatch):
    f = _Fighter(0, "ForwardSmash", 1)
    real = fighter_mod.Fighter.anim_state.fget
    f.fighter_name = "Pikachu"
    assert real(f) == ""  # the table ships empty
    monkeypatch.setitem(fighter_mod.FIGHTER_FRAME_DATA, "Pikachu", {"ForwardSmash": {"startup": 15, "active_start": 15, "active_end": 17},
                                                                   "Taunt": {"startup": None, "active_start": None, "active_end": None}})
    states = []
    for frame in (14, 15, 17, 18):
        f.animation_frame_num = frame
        states.append(real(f))
    assert states == ["startup", "active", "active", "end lag"]
    f.action = "Taunt"
    assert real(f) == ""
    f.action = "Dash"
    assert real(f) == ""


# ---- argument checks, before any launch --------------------------------------------------------------------------------

def test_box_label_value_errors_need_no_gpu():
    a = annotator.Annotator(30, 128, 64, max_frames=2, max_text=40)
    assert (a.left_padding, a.right_padding, a.bottom_padding, a.output_width, a.output_height) == (0, 0, 0, 128, 64)
    assert a.lw == 2
    a.begin(2)
    for bad in ("café", "two\nlines", "tab\t", "\x7f"):
        with pytest.raises(ValueError, match="printable ASCII"):
            a.box_label(0, (1, 2, 3, 4), label=bad)
    for k in range(16):
        a.box_label(0, (1, 2, 3, 4), label="ab" if k < 2 else "")
    with pytest.raises(ValueError, match="more than 16 items"):
        a.box_label(0, (1, 2, 3, 4))
    a.box_label(1, (1, 2, 3, 4), label="x" * 36)  # 4 + 36 = the buffer, exactly
    with pytest.raises(ValueError, match="text buffer"):
        a.box_label(1, (1, 2, 3, 4), label="y")
    with pytest.raises(ValueError, match="reversed"):
        a.box_label(1, (5, 9, 8, 6))  # live Pillow refuses to outline it
    a.box_label(1, (980, 80, 1200, 60), draw_box=False)  # the timer's box is fine: nothing outlines it
    with pytest.raises(ValueError, match="reversed"):
        a.box_label(1, (5, 9, 8, 6), color=None)  # color=None still outlines (in white)
    a.box_label(1, (5, 9, 8, 6), color=None, draw_box=False)
    with pytest.raises(ValueError, match="integers"):
        a.box_label(1, (1.5, 2, 3, 4))
    with pytest.raises(IndexError):
        a.box_label(2, (1, 2, 3, 4))
    assert a._counts.tolist() == [16, 3] and bytes(a._text) == b"abab" + b"x" * 36
    it = a._items[1, 1]
    assert it["box"].tolist() == [980, 80, 1200, 60] and it["draw_box"] == 0 and it["has_color"] == 1 and it["rgb"].tolist() == [128] * 3


def test_annotator_geometry_mirrors_the_reference():
    a = annotator.Annotator(60, 1920, 1080, show_stats=True)
    assert (a.left_padding, a.right_padding, a.bottom_padding) == (400, 400, 400)
    assert (a.output_width, a.output_height) == (2720, 1480)
    assert a.lw == max(round((1080 + 1920 + 4) / 2 * 0.003), 2) == 5
    a.begin(1, line_width=4)
    assert a.lw == 4


# ---- ABI ---------------------------------------------------------------------------------------------------------------

def test_header_prototypes_bindings_and_abi_version():
    header = open(os.path.join(ROOT, "include", "playaid_hip.h")).read()
    bound = {name: (res, args) for name, res, args in _lib.SYMBOLS}
    for name in ("pa_annot_create", "pa_annotate_frames", "pa_annot_destroy"):
        proto = re.search(r"^(?:int|void) " + name + r"\(([^;]*)\);", header, re.M | re.S)
        assert proto, name
        assert name in bound and len(bound[name][1]) == proto.group(1).count(",") + 1, name
    assert re.search(r"^#define PA_ABI_VERSION 15$", header, re.M) and _lib.PA_ABI_VERSION == 15
    assert re.search(r"^#define PA_ANNOT_MAX_ITEMS 16$", header, re.M) and _lib.PA_ANNOT_MAX_ITEMS == annotator.MAX_ITEMS == 16
    import ctypes

    assert ctypes.sizeof(_lib.pa_annot_item) == annotator.ITEM_DTYPE.itemsize == 40
    for name, (off, _) in {n: (annotator.ITEM_DTYPE.fields[n][1], 0) for n in annotator.ITEM_DTYPE.names}.items():
        assert getattr(_lib.pa_annot_item, name).offset == off, name


# ---- nothing changes without an output path ----------------------------------------------------------------------------

def test_render_and_cli_without_an_output_path_are_unchanged(tmp_path):
    log = str(tmp_path / "stub.log")
    synth.make_stub_log(log, 16)
    m = manuscript.Manuscript(input_video_path="absent.npz", ground_truth_path=log, log_offset=5)
    summary = m.render()
    assert summary == m.render(output_video_path=None, skip_graphs=True, show_timer=True)
    assert sorted(summary) == ["fighters", "frames"] and summary["frames"] == 11
    assert [sorted(f) for f in summary["fighters"]] == [["actions", "fighter_id", "fighter_name", "last_crop", "moves"]] * 2
    assert [f["actions"] for f in summary["fighters"]] == [{"Undefined": 11}] * 2
    r = CliRunner().invoke(manuscript.run_manuscript, ["--video-path", "absent.npz", "--log-path", log])
    assert r.exit_code == 0, r.output
    assert r.output == json.dumps(summary, indent=1, sort_keys=True) + "\nCOMPLETED\n"
