"""``detect_composite.generate_stage_char_compositions`` end to end on the device -- resize, ``pa_sprite_augment``, scenes, JPEG
encode -- against the numpy twins and Pillow's own encoder: every ``comp-i.jpg`` byte for byte, every label file, the numbering
of a second call and ``overwrite``."""
import io
import os
import sys

import numpy as np
import pytest
from PIL import Image

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "tests"))
from helpers import detect_composite_cases as cases  # noqa: E402

from playaid_core_amd import detect_composite as dc  # noqa: E402
from playaid_core_amd import sprite_augment as sa  # noqa: E402
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd import synth_dataset as sd  # noqa: E402

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def engine():
    from playaid_core_amd.engine import Engine

    eng = Engine(synth.make_state_dict(seed=7), max_batch_frames=4, max_clip_frames=16, max_frame_height=128, max_frame_width=128)
    yield eng
    eng.close()


def _jpeg(rgb):
    b = io.BytesIO()
    Image.fromarray(rgb).save(b, format="JPEG", quality=95, subsampling=2)   # the pin tests/test_jpeg_encode.py uses
    return b.getvalue()


def _twin(sprites, render_arrays, stages, stage_arrays, seed, first, n, batch):
    """(jpeg bytes, label text) per image, as the entry point numbers and draws them."""
    out = []
    for i0 in range(first, first + n, batch):
        b = min(batch, first + n - i0)
        resize, aug, scenes, labels = dc.sample_scenes(np.random.default_rng([seed, i0]), sprites, stages, b)
        slots = np.zeros((0, 128, 128, 4), dtype=np.uint8)
        if len(resize):
            slots = sa.augment_sprites_reference(dc.resize_sprites_reference(render_arrays, resize, 150, 525), aug)
        for scene, rows in zip(dc.compose_scenes_reference(slots, stage_arrays, scenes), labels):
            out.append((_jpeg(scene), dc.label_text(rows)))
    return out


def test_files_equal_the_twins_and_the_numbering_continues(engine, tmp_path):
    tree = cases.sampler_tree()
    sprites = sd.SpriteBank.from_arrays(engine, tree)
    render_arrays = [f for acts in tree.values() for bodies in acts.values() for raws in bodies.values() for cams in raws.values()
                     for frames in cams.values() for f in frames]
    assert [a.shape[:2] for a in render_arrays] == sprites.shapes
    stage_arrays = cases.make_stages([(150, 200), (77, 131)])
    stages = sd.StageBank.from_arrays(engine, stage_arrays)
    root = str(tmp_path)

    def check(first, n, seed, batch):
        want = _twin(sprites, render_arrays, stages, stage_arrays, seed, first, n, batch)
        for k, (blob, text) in enumerate(want):
            i = first + k
            with open(os.path.join(root, "train", "images", f"comp-{i}.jpg"), "rb") as f:
                got = f.read()
            assert got == blob, (i, len(got), len(blob))
            with open(os.path.join(root, "train", "labels", f"comp-{i}.txt")) as f:
                assert f.read() == text, i
        return want

    written = dc.generate_stage_char_compositions("train", 5, root, sprites, stages, seed=3, batch=2)
    assert [os.path.basename(p) for p in written] == [f"comp-{i}.jpg" for i in range(5)]
    want = check(0, 5, 3, 2)
    assert any(t for _, t in want) and len({b for b, _ in want}) == 5
    sizes = {Image.open(io.BytesIO(b)).size for b, _ in want}
    assert sizes == {(200, 150), (131, 77)}, sizes                     # both stages were drawn
    # a second call continues the numbering
    written = dc.generate_stage_char_compositions("train", 2, root, sprites, stages, seed=3, batch=2)
    assert [os.path.basename(p) for p in written] == ["comp-5.jpg", "comp-6.jpg"]
    check(5, 2, 3, 2)
    assert len(os.listdir(os.path.join(root, "train", "images"))) == len(os.listdir(os.path.join(root, "train", "labels"))) == 7
    # overwrite restarts it
    written = dc.generate_stage_char_compositions("train", 1, root, sprites, stages, seed=4, batch=2, overwrite=True)
    assert [os.path.basename(p) for p in written] == ["comp-0.jpg"]
    again = check(0, 1, 4, 1)
    assert again[0][0] != want[0][0] and len(os.listdir(os.path.join(root, "train", "images"))) == 7
    with pytest.raises(NotImplementedError):
        dc.generate_stage_char_compositions("train", 1, root, sprites, stages, bbox_overlay=True)
    sprites.close()
    stages.close()
