"""The detector's output as the reference's cache directory (rows a2 / a3 of SURVEY.md section 8).

``AIRunner.run_yolo`` (``playaid/ai_runner.py:191-224``) shells out to ``detect.py --save-txt --save-conf --save-crop`` and
treats what that leaves in ``<AI_CACHE>/<exp>`` as its boundary: it returns at once when ``crops/`` exists (``:192-194``),
and everything behind it reads ``labels/<video>_<n>.txt`` and ``crops/<Fighter>/<video>_<n>.jpg`` (``:291-295``).
``write_detector_cache`` writes that state from a detection table in HBM -- the label text of ``detect.py``, the crop
pixels of ``pa_save_one_box_crops`` and their JPEG FILES from the device's encoder (``jpeg_encode.JpegEncoder``: quality
95, 4:4:4, byte for byte what YOLOv5's ``Image.save`` writes) -- so a second run over the same video skips the detector,
and the reference (or ``ClipSource.from_cache`` here) can continue from it. The repair state ``clean_yolo_crops`` adds later
(empty label files, interpolated and copied crops) is not written: both consumers repair on load.
"""
from __future__ import annotations

import os
from typing import Dict, List, Sequence, Tuple

import numpy as np

from . import constants
from .detect import label_lines

CROP_QUALITY = 95       # utils/plots.py::save_one_box: Image.fromarray(crop[..., ::-1]).save(f, quality=95, subsampling=0)
CROP_SUBSAMPLING = 0


def label_path(video_name: str, frame_num: int) -> str:
    """``labels/<video>_<n>.txt``, n 1-based (``ai_runner.py:291-292``)."""
    return os.path.join("labels", f"{video_name}_{frame_num}.txt")


def crop_path(fighter: str, video_name: str, frame_num: int, occurrence: int = 0) -> str:
    """``crops/<Fighter>/<video>_<n>.jpg`` (``ai_runner.py:294-295``). ``occurrence`` k > 0: the k-th FURTHER detection of
    that class in the frame, which finds the name taken and gets YOLOv5's ``increment_path`` name -- the stem with 2, 3, ...
    appended (the files "with another number attached at the end" of ``ai_runner.py:247-257``)."""
    stem = f"{video_name}_{frame_num}"
    return os.path.join("crops", fighter, (stem if occurrence == 0 else f"{stem}{occurrence + 1}") + ".jpg")


def cache_layout(dets: np.ndarray, counts: np.ndarray, video_name: str,
                 names: Sequence[str] = constants.CHAR_LIST) -> Tuple[List[Tuple[str, str]], List[Tuple[int, int, str]]]:
    """Host bookkeeping of the cache, no pixels: ``dets`` float32[n, max_det, 6] label rows (cls cx cy w h conf) in
    label-file order, ``counts`` int32[n] -> (label files: (relative path, text) for every frame with detections -- a
    frame without has no file --, crop files: (frame index, detection index, relative path) in the order ``detect.py``
    saves them)."""
    labels, crops = [], []
    for i in range(dets.shape[0]):
        k = int(counts[i])
        if k <= 0:
            continue
        labels.append((label_path(video_name, i + 1), label_lines(dets[i, :k])))
        seen: Dict[int, int] = {}
        for j in range(k):
            cls = int(dets[i, j, 0])
            if not 0 <= cls < len(names):
                raise ValueError(f"frame {i + 1}: class id {cls} has no name")
            crops.append((i, j, crop_path(names[cls], video_name, i + 1, seen.get(cls, 0))))
            seen[cls] = seen.get(cls, 0) + 1
    return labels, crops


def write_detector_cache(engine, encoder, frames_dev, dets, counts, out_dir: str, video_name: str,
                         names: Sequence[str] = constants.CHAR_LIST) -> Dict[str, int]:
    """frames uint8[n, H, W, 3] BGR (device), ``dets`` float32[n, max_det, 6] / ``counts`` int32[n] (device, as
    ``Engine.detect_postprocess`` writes them) -> ``out_dir/labels`` and ``out_dir/crops`` as ``detect.py --save-txt
    --save-conf --save-crop`` leaves them. The crops are cut (``pa_save_one_box_crops``, raw) and encoded
    (``encoder``: a ``JpegEncoder`` whose ``max_images`` is at least the engine's fighters) on the device; per chunk of
    frames one device -> host copy of the files. -> {"labels": files written, "crops": files written}."""
    import torch

    n, h, w, _ = frames_dev.shape
    F = engine.F
    max_det = dets.shape[1]
    d_host, c_host = dets.cpu().numpy(), counts.cpu().numpy()
    label_files, crop_files = cache_layout(d_host[:n], c_host[:n], video_name, names)
    for rel, text in label_files:
        path = os.path.join(out_dir, rel)
        os.makedirs(os.path.dirname(path), exist_ok=True)
        with open(path, "w") as f:
            f.write(text)
    os.makedirs(os.path.join(out_dir, "crops"), exist_ok=True)
    where = {(i, j): rel for i, j, rel in crop_files}
    step = min(engine.max_batch_frames, encoder.max_images // F)
    if step < 1:
        raise ValueError(f"write_detector_cache: the encoder takes {encoder.max_images} images per call, a frame has {F}")
    written = 0
    for j0 in range(0, max_det, F):   # detections j0 .. j0 + F - 1 of every frame: one crop slot per DETECTION
        for f0 in range(0, n, step):
            cnt = min(step, n - f0)
            idx = np.full((cnt, F), -1, np.int32)
            for s in range(F):
                idx[:, s] = np.where(j0 + s < c_host[f0:f0 + cnt], j0 + s, -1)
            if (idx < 0).all():
                continue
            images, desc = engine.save_one_box_crops(frames_dev[f0:f0 + cnt], dets[f0:f0 + cnt], counts[f0:f0 + cnt], det_index=idx,
                                                     jpeg_quality=0)
            files, rec = encoder.encode_images(images, desc, h, w, quality=CROP_QUALITY, subsampling=CROP_SUBSAMPLING, bgr=True)
            blobs = encoder.unpack_files(files, rec)
            engine.check_device_errors()
            for e, blob in enumerate(blobs):
                i, j = f0 + e // F, j0 + e % F
                if blob is None:
                    encoder.overflows()
                    raise ValueError(f"write_detector_cache: the crop of frame {i + 1}, detection {j} does not fit the encoder "
                                     "(max_blocks / scratch_bytes)")
                if not blob or (i, j) not in where:   # no detection, or an empty rectangle: no file
                    continue
                path = os.path.join(out_dir, where[(i, j)])
                os.makedirs(os.path.dirname(path), exist_ok=True)
                with open(path, "wb") as f:
                    f.write(blob)
                written += 1
    torch.cuda.synchronize(engine.device)
    return {"labels": len(label_files), "crops": written}
