"""The arbiter of the annotation tests: the reference's literal drawing sequence with live Pillow
(``playaid/manuscript.py:156-158``, ``playaid/annotator.py:119-145, 300-311, 362``), shared by tests/test_annotate_host.py
and tests/test_annotate.py. Not a test module."""
import numpy as np
from PIL import Image, ImageDraw, ImageFont


def reference_annotate(frame_bgr, calls, line_width, pads=(0, 0, 0)):
    """``calls``: (box, label, color, draw_box) per ``box_label`` call; ``pads`` = (left, right, bottom).
    BGR frame in -> the BGR frame the reference hands its video writer."""
    im = Image.fromarray(np.ascontiguousarray(frame_bgr[..., ::-1])).convert("RGBA")  # cv2.COLOR_BGR2RGBA
    draw = ImageDraw.Draw(im)
    font = ImageFont.load_default_imagefont()  # Pillow < 10's ImageFont.load_default()
    for box, label, color, draw_box in calls:
        if draw_box:
            draw.rectangle(box, width=line_width, outline=color)
        if label:
            w, h = font.getbbox(label)[2:]  # the removed font.getsize(label)
            outside = box[1] - h >= 0
            if color:
                draw.rectangle((box[0], box[1] - h if outside else box[1], box[0] + w + 1, box[1] + 1 if outside else box[1] + h + 1),
                               fill=color)
            draw.text((box[0], box[1] - h if outside else box[1]), label, font=font, fill="white")
    a = np.array(im)
    left, right, bottom = pads
    if left or right or bottom:
        a = np.pad(a, ((0, bottom), (left, right), (0, 0)))
    return np.ascontiguousarray(a[..., 2::-1])  # cv2.COLOR_RGBA2BGR


def noise_frames(n, h, w, seed):
    return np.random.default_rng(seed).integers(0, 256, (n, h, w, 3), dtype=np.uint8)
