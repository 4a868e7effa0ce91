"""The annotator's drawing step on the MI355X: boxes and labels on frames in HBM (``pa_annotate_frames``, ``csrc/annotate.hip``).

Mirrors the reference's ``Annotator`` (``playaid/annotator.py:31-145, 300-363``) for the part ``Manuscript.render`` uses per
frame: ``set_frame`` -> ``box_label`` ... -> ``result`` (which pads the frame, ``maybe_pad_image``). Here the calls take a
CHUNK of device frames: ``set_frames(frames_dev)``, ``box_label(frame_index, box, ...)``, ``result()`` -- one launch copies
the chunk into the padded output and paints every frame's draw list on the way.

What is drawn is the reference's Pillow branch, the only one ``Manuscript.render`` reaches: ``set_frame`` computes
``self.pil = pil or non_ascii`` with a default ``example="abc✅"`` that is not ASCII, so ``pil=False`` is overridden and the
cv2 ``putText`` branch is dead on this path. The branch is ``ImageDraw.rectangle(outline=, width=)``,
``ImageDraw.rectangle(fill=)`` and ``ImageDraw.text(font=ImageFont.load_default(), fill="white")`` on an RGBA image; the
reference's ``text_font.getsize`` dates it to Pillow < 10, where ``load_default()`` is the built-in bitmap font --
``ImageFont.load_default_imagefont()`` today, 6 x 11 cells whose masks hold 0 / 255 only. ``glyph_atlas()`` reads that font
from the LIVE Pillow (no bitmap is committed) into the (character, next character) table the kernel places text from.
Two quirks are kept: text is always white (the Pillow branch ignores ``txt_color``), and ``color=None`` draws no
background and, with ``draw_box``, a WHITE outline (``rectangle(outline=None)`` falls back to ImageDraw's default ink).

Not here: the matplotlib / bokeh charts (``update_onscreen_charts`` etc.: the padding stays black), the emoji font, the cv2
branch. There is no CPU fallback: ``result()`` needs the HIP library and a GPU (``HipLibraryError`` otherwise).
``glyph_atlas``, ``outline_mask`` and the argument checks are host arithmetic and need neither.
"""
from __future__ import annotations

import ctypes as C
import operator
from typing import Optional, Sequence, Tuple

import numpy as np

MAX_ITEMS = 16  # PA_ANNOT_MAX_ITEMS: box_label calls per frame
FIRST_CHAR, N_CHARS = 32, 95  # printable ASCII

ITEM_DTYPE = np.dtype([("box", "<i4", (4,)), ("draw_box", "<i4"), ("line_width", "<i4"), ("has_color", "<i4"), ("text_off", "<i4"),
                       ("text_len", "<i4"), ("rgb", "u1", (3,)), ("reserved", "u1")])  # pa_annot_item
assert ITEM_DTYPE.itemsize == 40


def _mask_array(font, s: str) -> np.ndarray:
    m = font.getmask(s)
    w, h = m.size
    return np.frombuffer(bytes(m), dtype=np.uint8).reshape(h, w)


def glyph_atlas() -> np.ndarray:
    """``uint8[95][96][cell_h][cell_w]`` from Pillow's built-in bitmap font: ``[c][n]`` is the cell of character ``32 + c``
    when ``32 + n`` follows it, ``[c][95]`` when nothing does. The mask of a string is NOT the concatenation of its
    characters' masks -- the last column of a cell depends on the next character (how Pillow pastes glyphs) -- but cell k of
    ``font.getmask(s)`` equals ``font.getmask(s[k] + s[k + 1])[:, :cell_w]``, which is what the table holds."""
    from PIL import ImageFont

    font = ImageFont.load_default_imagefont()
    cw, ch = font.getbbox(" ")[2:]
    atlas = np.zeros((N_CHARS, N_CHARS + 1, ch, cw), np.uint8)
    for c in range(N_CHARS):
        a = chr(FIRST_CHAR + c)
        if font.getbbox(a)[2:] != (cw, ch):
            raise ValueError(f"Pillow's default bitmap font is not monospaced at {a!r}")
        atlas[c, N_CHARS] = _mask_array(font, a)
        for n in range(N_CHARS):
            atlas[c, n] = _mask_array(font, a + chr(FIRST_CHAR + n))[:, :cw]
    return atlas


def text_mask(atlas: np.ndarray, label: str) -> np.ndarray:
    """The mask ``font.getmask(label)`` as the kernel assembles it from the atlas (host restatement, for tests)."""
    codes = np.frombuffer(label.encode("ascii"), np.uint8).astype(np.int64) - FIRST_CHAR
    nxt = np.append(codes[1:], N_CHARS)
    return np.concatenate(list(atlas[codes, nxt]), axis=1)


def outline_mask(box, width, height: int, image_width: int) -> np.ndarray:
    """The pixels ``ImageDraw.rectangle(box, outline=..., width=width)`` paints in a ``height`` x ``image_width`` image:
    the rule ``csrc/annotate.hip`` evaluates per pixel, stated with numpy. ``box`` = (x0, y0, x1, y1) and ``width`` may be
    scalars (-> bool[height, image_width]) or arrays of one shape S (-> bool[S + (height, image_width)]).

    Pillow's routine orders the rows (y0 <= y1) and draws, for i = 0 .. width - 1, the horizontal lines y0 + i and y1 - i
    over the columns between x0 and x1, and vertical lines at x1 - i and x0 + i from row a = y0 + width to row
    b = y1 - width + 1. A vertical ``line`` paints |b - a| pixels starting at a and walking towards b, without its end
    point: rows a .. b - 1 for a roomy box, rows b + 1 .. a for a box thinner than twice the width -- and those can lie
    below y1, outside the box."""
    x0, y0, x1, y1 = (np.asarray(v, np.int32)[..., None, None] for v in box)
    lw = np.asarray(width, np.int32)[..., None, None]
    y0, y1 = np.minimum(y0, y1), np.maximum(y0, y1)
    yy, xx = np.mgrid[0:height, 0:image_width].astype(np.int32)
    band = ((yy >= y0) & (yy < y0 + lw)) | ((yy <= y1) & (yy > y1 - lw))
    side = ((xx <= x1) & (xx > x1 - lw)) | ((xx >= x0) & (xx < x0 + lw))
    a, b = y0 + lw, y1 - lw + 1
    rows = np.where(b >= a, (yy >= a) & (yy < b), (yy <= a) & (yy > b))
    return (band & (xx >= np.minimum(x0, x1)) & (xx <= np.maximum(x0, x1))) | (side & rows)


def default_line_width(height: int, width: int) -> int:
    """``max(round(sum(im.shape) / 2 * 0.003), 2)`` (``annotator.py:101``); ``im`` there is the RGBA frame, shape (H, W, 4)."""
    return max(round((height + width + 4) / 2 * 0.003), 2)


class Annotator:
    """``Annotator(fps, input_width, input_height, show_stats=False)``: ``show_stats`` pads 400 columns left and right and
    400 rows below, as the reference does for its charts (which are not drawn here: the padding is black).

    ``max_frames``: frames per ``set_frames`` chunk; ``max_text``: label characters per chunk; ``pads`` = (left, right,
    bottom) overrides the reference's two paddings."""

    def __init__(self, fps, input_width: int, input_height: int, show_stats: bool = False, max_frames: int = 64,
                 max_text: int = 16384, device: str = "cuda:0", pads: Optional[Tuple[int, int, int]] = None):
        self.fps = fps
        self.input_width, self.input_height = int(input_width), int(input_height)
        self.show_stats = bool(show_stats)
        self.left_padding = self.right_padding = self.bottom_padding = 400 if self.show_stats else 0
        if pads is not None:
            self.left_padding, self.right_padding, self.bottom_padding = (int(v) for v in pads)
            if min(self.left_padding, self.right_padding, self.bottom_padding) < 0:
                raise ValueError(f"pads {pads!r} are negative")
        self.output_width = self.input_width + self.left_padding + self.right_padding
        self.output_height = self.input_height + self.bottom_padding
        self.max_frames, self.max_text = int(max_frames), int(max_text)
        self.device_name = device
        self.lw = default_line_width(self.input_height, self.input_width)
        self._h = C.c_void_p(0)
        self._lib = None
        self._frames = None
        self._items = np.zeros((self.max_frames, MAX_ITEMS), ITEM_DTYPE)
        self._counts = np.zeros(self.max_frames, np.int32)
        self._text = bytearray()

    # -- the handle (made at the first result(): everything above works without a GPU) ------------------------------
    def _handle(self):
        if self._h:
            return self._h
        import torch

        from . import _lib
        from .engine import EngineError

        self._lib = _lib.load()
        if not torch.cuda.is_available():
            raise _lib.HipLibraryError("no HIP device visible to PyTorch-ROCm; annotation has no CPU fallback")
        self.device = torch.device(self.device_name)
        torch.cuda.set_device(self.device)
        atlas = np.ascontiguousarray(glyph_atlas())
        rc = self._lib.pa_annot_create(self.device.index or 0, atlas.ctypes.data_as(C.c_void_p), atlas.shape[3], atlas.shape[2], FIRST_CHAR,
                                       N_CHARS, self.max_frames, MAX_ITEMS, self.max_text, C.byref(self._h))
        if rc != _lib.PA_OK:
            self.close()
            raise EngineError(rc, "pa_annot_create: " + self._lib.pa_status_string(rc).decode())
        return self._h

    def close(self):
        if getattr(self, "_h", None) and self._lib is not None:
            self._lib.pa_annot_destroy(self._h)
        self._h = C.c_void_p(0)

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    # -- the reference's calls, per chunk -----------------------------------------------------------------------------
    def set_frames(self, frames_dev, line_width: Optional[int] = None):
        """``set_frame`` for a chunk: uint8[n, H, W, 3] BGR on the device (what the decoder writes). Starts empty draw lists."""
        import torch

        if not isinstance(frames_dev, torch.Tensor) or frames_dev.dtype != torch.uint8 or not frames_dev.is_cuda or \
                not frames_dev.is_contiguous() or frames_dev.ndim != 4 or frames_dev.shape[3] != 3:
            raise ValueError("set_frames: frames are a contiguous uint8[n, H, W, 3] device tensor")
        n, h, w, _ = frames_dev.shape
        if (h, w) != (self.input_height, self.input_width):
            raise ValueError(f"set_frames: frames are {h} x {w}, the annotator was made for {self.input_height} x {self.input_width}")
        if not 1 <= n <= self.max_frames:
            raise ValueError(f"set_frames: {n} frames, the annotator takes 1..{self.max_frames} per chunk")
        self._frames = frames_dev
        self.begin(n, line_width)

    def begin(self, n: int, line_width: Optional[int] = None):
        """Empty draw lists for ``n`` frames (``set_frames`` calls it; on its own it lets the lists be built without a GPU)."""
        if not 1 <= n <= self.max_frames:
            raise ValueError(f"{n} frames, the annotator takes 1..{self.max_frames} per chunk")
        self._n = n
        self.lw = line_width or default_line_width(self.input_height, self.input_width)
        self._counts[:] = 0
        self._text = bytearray()

    def box_label(self, frame_index: int, box: Sequence[int], label: str = "", color: Optional[Tuple[int, int, int]] = (128, 128, 128),
                  txt_color=(255, 255, 255), draw_box: bool = True):
        """One ``box_label`` call on frame ``frame_index`` of the chunk (``annotator.py:103-145``). ``box`` = (x0, y0, x1,
        y1) integers, anywhere (negative, outside the frame). ``txt_color`` is accepted and ignored, as in the reference's
        Pillow branch: the text is white. ``color=None``: no background, and the outline (if ``draw_box``) in white."""
        if not 0 <= frame_index < getattr(self, "_n", 0):
            raise IndexError(f"box_label: frame {frame_index} outside the chunk")
        try:
            b = [operator.index(v) for v in box]
        except TypeError:
            raise ValueError(f"box_label: box {box!r} is not four integers") from None
        if len(b) != 4 or any(not -2 ** 31 <= v < 2 ** 31 for v in b):
            raise ValueError(f"box_label: box {box!r} is not four 32-bit integers")
        bad = [ch for ch in label if not FIRST_CHAR <= ord(ch) < FIRST_CHAR + N_CHARS]
        if bad:
            raise ValueError(f"box_label: label {label!r} has characters outside printable ASCII (32..126): {bad!r}")
        if draw_box and self.lw and (b[2] < b[0] or b[3] < b[1]):
            # (Pillow >= 9.5 refuses it: "x1 must be greater than or equal to x0")
            raise ValueError(f"box_label: box {box!r} is reversed; ImageDraw.rectangle does not outline it")
        k = int(self._counts[frame_index])
        if k >= MAX_ITEMS:
            raise ValueError(f"box_label: more than {MAX_ITEMS} items in frame {frame_index}")
        if len(self._text) + len(label) > self.max_text:
            raise ValueError(f"box_label: the chunk's labels exceed the text buffer ({self.max_text} characters)")
        it = self._items[frame_index, k]
        it["box"] = b
        it["draw_box"] = int(bool(draw_box))
        it["line_width"] = int(self.lw)
        it["has_color"] = int(color is not None)
        it["rgb"] = [int(c) & 255 for c in color] if color is not None else [0, 0, 0]
        it["text_off"] = len(self._text)
        it["text_len"] = len(label)
        self._text += label.encode("ascii")
        self._counts[frame_index] = k + 1

    def result(self, out=None):
        """Enqueues the launch on the current stream and returns uint8[n, output_height, output_width, 3] BGR on the device."""
        import torch

        from . import _lib
        from .engine import EngineError

        if self._frames is None:
            raise ValueError("result: no frames set")
        h = self._handle()
        n = self._n
        shape = (n, self.output_height, self.output_width, 3)
        if out is None:
            out = torch.empty(shape, dtype=torch.uint8, device=self._frames.device)
        elif out.dtype != torch.uint8 or not out.is_cuda or not out.is_contiguous() or tuple(out.shape) != shape:
            raise ValueError(f"result: out is a contiguous uint8{list(shape)} device tensor")
        text = np.frombuffer(bytes(self._text), np.uint8) if self._text else np.zeros(1, np.uint8)
        stream = C.c_void_p(torch.cuda.current_stream(self._frames.device).cuda_stream)
        rc = self._lib.pa_annotate_frames(h, C.c_void_p(self._frames.data_ptr()), n, self.input_height, self.input_width,
                                          self._items.ctypes.data_as(C.c_void_p), self._counts.ctypes.data_as(C.c_void_p),
                                          text.ctypes.data_as(C.c_void_p), len(self._text), self.left_padding, self.right_padding,
                                          self.bottom_padding, C.c_void_p(out.data_ptr()), stream)
        if rc != _lib.PA_OK:
            raise EngineError(rc, "pa_annotate_frames: " + self._lib.pa_status_string(rc).decode())
        return out
