"""The dataset-shaped input API of the action model over a decoded clip (``playaid/ult_action_dataset.py:233-371``).

The reference's ``UltActionRecogDataset.__getitem__`` hands the training / evaluation loop
``(frames[S, 3, H, W].float() / 255, tensor(char_id), tensor(action_ids[S]), meta)`` -- S crops around a middle frame picked by
``action_sample_from_frame_middle_out`` (``dataset_utils.py:109-138``), each ``cv2.imread`` + ``BGR2RGB`` +
``imutils.resize(width=crop_size)`` of a crop file, the action string of each of the S frames mapped through the animation
list, and a dict with the pieces. ``ClipWindowDataset`` yields the same 4-tuple for every (fighter, frame) of a clip the
runner has open, with the crops cut ON THE DEVICE by the engine's crop path (``pa_save_one_box_crops`` / ``pa_square_crops`` /
``pa_runner_inputs`` -- whatever ``AIRunner`` was configured with) instead of read from crop files, and the window indices from
the same sampler with the runner's own range (frames are 1-indexed crop files, ``ai_runner.py:438-439``). Its batches are what
``CNNActionDetector.forward`` takes (``cnn_action_detector.py:86-92``).

``synth_difficulty`` 1 or 2 passes every crop of an item through the reference's ``augment_char_crop`` at that level
(``ult_action_dataset.py:305-330``), on the device: ``augment.py``, DESIGN.md 5.14.

The synthetic windows of the reference's dataset (``get_synth``, ``simple_dataset``: character renders resized and pasted over
stage crops) are ``synth_dataset.SynthWindowDataset``, composed on the device from uploaded renders (``synth_dataset.py``,
DESIGN.md 5.15); ``augment_synth_char_crop``, the augmentation of the RGBA render BEFORE it is pasted that ``synth_difficulty``
1 / 2 adds to them, is ``sprite_augment.py``.

Not built, by scope (training only): the random choice of (fighter, action, frame), the frame-delta
choice, ``preceding_actions`` (the reference's own loop over them is empty: ``range(a, a)``,
``ult_action_dataset.py:284-286``).

For scoring (``metrics.py``, ``AIRunner.evaluate``): ``load_ground_truth_labels`` reads a hand-labelled clip's CSV as the
reference does (``ult_action_dataset.py:512-559``) and ``label_table`` turns action strings -- per-fighter lists or that CSV's
labels -- into the ``int32[max_frames - 1, F]`` table the device accumulator takes, ``-100`` where a frame has no ground truth.
"""
from __future__ import annotations

import csv
from collections import defaultdict
from typing import List, Optional, Sequence

import numpy as np
import torch

from . import augment, constants
from .anim_ontology import MOVE_TO_CLASS_ID
from .dataset_utils import action_sample_from_frame_middle_out


def _action_id(animations: Sequence[str], action: str) -> int:
    # ult_action_dataset.py:352-357 (an action outside the list maps to "Unknown", which must then be in the list)
    return animations.index(action) if action in animations else animations.index("Unknown")


def load_ground_truth_labels(csv_path: str, lines=None):
    """``UltActionRecogDataset.load_ground_truth_labels`` (``ult_action_dataset.py:512-559``) on ``csv_path``: rows
    ``frame_num, fighter, action, cx, cy, w, h``; line 1 (the header) is skipped, and with ``lines`` (a set of 1-based line
    numbers, the reference's train / validation split) only those lines are kept -- None keeps every line.
    -> ``(labels[fighter][frame_num] = (frame_num, fighter, action, cx, cy, w, h), action_to_frames[fighter][action] = [frame_num])``.
    ``frame_num`` is the frame's ``VideoCapture`` position (``:463``): 0 is the first frame."""
    labels = defaultdict(dict)
    action_to_frames = {}
    with open(csv_path, newline="") as f:
        reader = csv.reader(f)
        for row in reader:
            if reader.line_num == 1 or (lines is not None and reader.line_num not in lines):
                continue
            if not row:
                continue
            frame_num, fighter_name, action = int(row[0]), row[1], row[2]
            labels[fighter_name][frame_num] = (frame_num, fighter_name, action, float(row[3]), float(row[4]), float(row[5]), float(row[6]))
            if fighter_name not in action_to_frames:
                action_to_frames[fighter_name] = defaultdict(list)
            action_to_frames[fighter_name][action].append(frame_num)
    return dict(labels), dict(action_to_frames)


def label_table(runner_or_names, actions, animations: Optional[Sequence[str]] = None, n_rows: Optional[int] = None,
                first_frame: int = 0) -> np.ndarray:
    """-> ``int32[max_frames - 1, F]``: row i, column p = the action id of fighter slot p in the runner's frame i + 1 (the rows
    of ``Engine.evaluate_clip`` / ``infer_clip``'s ``logp``), ``-100`` (``metrics.IGNORE``) where there is no ground truth.

    ``runner_or_names``: an ``AIRunner`` (its ``fighters`` and ``max_frames``) or the fighter names in slot order (then ``n_rows``,
    or as many rows as the labels reach). ``actions``: per-fighter sequences ``actions[p][i]`` of action strings (the shape
    ``ClipWindowDataset`` takes; None = no ground truth), or ``load_ground_truth_labels``' ``labels[fighter][frame_num]`` mapping --
    frame_num ``first_frame + i`` is row i (the CSV counts ``VideoCapture`` positions, the runner's frame i + 1 is position i).
    Strings go through the dataset's rule: one outside ``animations`` (default: the ontology's 63) is ``"Unknown"``, which must
    then be in the list (ValueError otherwise, as in the reference)."""
    animations = list(animations) if animations is not None else list(MOVE_TO_CLASS_ID.keys())
    if hasattr(runner_or_names, "fighters"):
        names = list(runner_or_names.fighters)
        n_rows = runner_or_names.max_frames - 1 if n_rows is None else n_rows
    else:
        names = list(runner_or_names)
    by_name = isinstance(actions, dict)
    cols = []
    for p, name in enumerate(names):
        if by_name:
            cols.append({f - first_frame: rec[2] if isinstance(rec, (tuple, list)) else rec for f, rec in actions.get(name, {}).items()})
        else:
            cols.append({i: a for i, a in enumerate(actions[p]) if a is not None})
    if n_rows is None:
        n_rows = max([max(c) + 1 for c in cols if c] or [0])
    out = np.full((n_rows, len(names)), -100, dtype=np.int32)
    for p, col in enumerate(cols):
        for i, a in col.items():
            if 0 <= i < n_rows:
                out[i, p] = _action_id(animations, a)
    return out


class ClipWindowDataset:
    """Index i -> fighter ``i // (max_frames - 1)``, frame ``1 + i % (max_frames - 1)`` (the order of
    ``AIRunner.run_action_recognition``'s two loops, ``ai_runner.py:493-520``)."""

    def __init__(self, runner, actions: Optional[Sequence[Sequence[str]]] = None, animations: Optional[List[str]] = None,
                 crop_size: int = 128, synth_difficulty: int = 0, seed: int = 0):
        """``runner``: an ``AIRunner`` (its clip, label repair, crop mode and sampler settings are used as they are).
        ``actions[p][f - 1]``: the ground-truth action string of fighter slot p in frame f (what the reference reads from the
        frame's label file, ``ult_action_dataset.py:340-343``), or None: every frame is labelled ``Undefined``.
        ``animations``: the action list the ids index (default: the ontology's 63, ``anim_ontology.py:592-600``).
        ``crop_size`` (``UltActionRecogDataset(crop_size=...)``; 16..512): 128 hands out the runner's own crops, as ever. With
        any other size the S crops of an item are cut from the clip's FRAMES by ``Engine.square_crops(output_size=crop_size)``
        with the runner's repaired boxes at the engine's crop padding (RGB, no JPEG write / read: that stage is 128 x 128) --
        so the clip needs frames, and a clip that holds only crop files raises ValueError.
        ``synth_difficulty`` (``UltActionRecogDataset(synth_difficulty=...)``; 0, 1 or 2): with 1 or 2 the S crops of an item go
        through ``augment.augment_crops`` at that level, each with its own draw as in the reference's loop; the draw of item
        ``idx`` in epoch ``e`` (``set_epoch``) is a pure function of ``(seed, e, idx)``. The augmentation is the 128 x 128
        kernel: with another ``crop_size`` it raises ValueError (DESIGN.md 5.8c has the sized crops, 5.14 the augmentation). 0
        leaves every item as it is without the argument."""
        self.runner = runner
        self.animations = list(animations) if animations is not None else list(MOVE_TO_CLASS_ID.keys())
        self.characters = list(constants.CHAR_LIST)
        self.num_frames_per_sample = runner.num_frames_per_sample
        self.frame_delta = runner.frame_delta
        self.crop_size = int(crop_size)
        if self.crop_size != crop_size or not 16 <= self.crop_size <= 512:
            raise ValueError(f"crop_size must be an integer in 16..512, got {crop_size!r}")
        self._sized_boxes = None
        self.synth_difficulty = self._check_level(synth_difficulty)
        self.seed, self.epoch = int(seed), 0
        self._crops_dev = None   # (the clip's results it was made from, the crops as one device tensor [(max_frames - 1) * F, 128, 128, 3])
        if self.crop_size != 128 and (runner.clip.frames.shape[1] == 0 or runner.clip.frames.shape[2] == 0):
            raise ValueError(f"crop_size={self.crop_size}: crops of another size than 128 are cut from the clip's frames, and this "
                             "clip holds crop files only: frames are needed")
        self.actions = actions
        if actions is not None:
            if len(actions) != len(runner.fighters) or any(len(a) < runner.max_frames - 1 for a in actions):
                raise ValueError("actions: one list per fighter with an entry for every frame in [1, max_frames)")

    def __len__(self):
        return (self.runner.max_frames - 1) * len(self.runner.fighters)

    def _check_level(self, level) -> int:
        if level not in range(augment.MAX_LEVEL + 1):
            raise ValueError(f"synth_difficulty is 0, 1 or {augment.MAX_LEVEL}, got {level!r}")
        if level and self.crop_size != 128:
            raise ValueError(f"synth_difficulty={level} with crop_size={self.crop_size}: the augmentation is built for 128 x 128 crops only "
                             "(DESIGN.md 5.8c: crops of other sizes; 5.14: the augmentation)")
        return int(level)

    def set_epoch(self, epoch: int):
        """The epoch the augmentation's draws are keyed by (with ``seed`` and the item's index)."""
        self.epoch = int(epoch)

    def make_synth_more_challenging(self):
        """``UltActionRecogDataset.make_synth_more_challenging`` (``ult_action_dataset.py:561-564``): one level up, 2 at most."""
        if self.synth_difficulty < augment.MAX_LEVEL:
            self.synth_difficulty = self._check_level(self.synth_difficulty + 1)

    def _augmented(self, res, idx: int, p: int, frame_nums):
        """The item's S crops through ``augment_char_crop`` at the dataset's level: one launch, one read."""
        eng = self.runner._clip_engine
        if self._crops_dev is None or self._crops_dev[0] is not res:
            crops = np.ascontiguousarray(res["crops_rgb"][: self.runner.max_frames - 1])
            self._crops_dev = (res, torch.from_numpy(crops.reshape(-1, 128, 128, 3)).to(eng.device), crops.shape[1])
        _, crops_dev, F = self._crops_dev
        rng = np.random.default_rng([self.seed, self.epoch, idx])
        params = augment.sample_params(len(frame_nums), self.synth_difficulty, rng, src=[(f - 1) * F + p for f in frame_nums])
        return list(augment.augment_crops(eng, crops_dev, params, "uint8").cpu().numpy())

    def _action_id(self, action: str) -> int:
        return _action_id(self.animations, action)

    def __getitem__(self, idx: int):
        n_per = self.runner.max_frames - 1
        if not 0 <= idx < len(self):
            raise IndexError(idx)
        p, frame_num = idx // n_per, 1 + idx % n_per
        fighter_name = self.runner.fighters[p]
        frame_nums = action_sample_from_frame_middle_out(
            frame_num, num_frames_per_sample=self.num_frames_per_sample, frame_delta=self.frame_delta,
            max_frames=self.runner.max_frames, min_frame=1,
        )
        if self.crop_size == 128:
            res = self.runner._run_clip()  # the clip's crops, cut once on the device and cached by the runner
            if self.synth_difficulty:
                frames = self._augmented(res, idx, p, frame_nums)
            else:
                frames = [res["crops_rgb"][f - 1, p] for f in frame_nums]
        else:
            frames = self._cut_sized(p, frame_nums)
        actions = [self.actions[p][f - 1] if self.actions is not None else "Undefined" for f in frame_nums]
        input_frames = torch.tensor(np.array(frames)).permute(0, 3, 1, 2)
        anim_label = [self._action_id(a) for a in actions]
        return (
            input_frames.float() / 255.0,
            torch.tensor(self.characters.index(fighter_name)),
            torch.tensor(anim_label),
            {
                "char": fighter_name,
                "frames": [np.array(f) for f in frames],
                "frame_paths": [f"{self.runner.video_name}_{f}.jpg" for f in frame_nums],  # the crop files' names (ai_runner.py:440-444)
                "actions": actions,
                "frame_delta": self.frame_delta,
                "preceding_actions": [],
                "preceding_actions_tensor": torch.tensor([], dtype=torch.int64),
            },
        )

    def _cut_sized(self, p: int, frame_nums):
        """The crops of fighter slot p in the frames ``frame_nums`` at ``crop_size``: ``square_crop(frame, crop_size, padding)`` of
        the repaired box, from the decoded frame the repair names (``AIRunner._boxes``), RGB."""
        runner = self.runner
        if self._sized_boxes is None:
            self._sized_boxes = runner._boxes()
        boxes, src, missing = self._sized_boxes
        rows = [f - 1 for f in frame_nums]
        bad = [f for f in frame_nums if missing[f - 1, p]]
        assert not bad, f"Failed to get frame crops/{runner.fighters[p]}/{runner.video_name}_{bad[0]}.jpg"  # as _run_clip
        eng = runner.model.engine
        clip_frames = runner.clip.frames
        h, w = int(clip_frames.shape[1]), int(clip_frames.shape[2])
        if h > eng.cfg.max_frame_height or w > eng.cfg.max_frame_width or len(rows) > eng.max_batch_frames:
            raise ValueError(f"the model's engine takes {eng.max_batch_frames} frames of {eng.cfg.max_frame_height} x {eng.cfg.max_frame_width} "
                             f"at most; the clip's are {h} x {w}")
        sel = [int(src[r, p]) for r in rows]
        if isinstance(clip_frames, torch.Tensor):
            fsel = clip_frames[torch.as_tensor(sel, device=clip_frames.device)]
        else:
            fsel = np.ascontiguousarray(clip_frames[sel])
        bsel = np.ascontiguousarray(np.repeat(boxes[rows, p][:, None, :], eng.F, axis=1), dtype=np.float64)
        crops, status = eng.square_crops(fsel, bsel, padding=eng.cfg.crop_padding, swap_rb=True, output_size=self.crop_size)
        bad = np.nonzero(status[:, 0])[0]
        assert len(bad) == 0, f"Failed to get square crop from frame {frame_nums[bad[0]]}"  # ai_runner.py:418
        return [crops[i, 0] for i in range(len(rows))]

    def batches(self, batch_size: int):
        """(x[B, S, 3, crop_size, crop_size], char_ids[B], action_ids[B, S], metas) in index order -- ``torch.utils.data.DataLoader``'s
        default collation without its worker processes (the crops live in one engine)."""
        for i0 in range(0, len(self), batch_size):
            items = [self[i] for i in range(i0, min(i0 + batch_size, len(self)))]
            yield (torch.stack([it[0] for it in items]), torch.stack([it[1] for it in items]), torch.stack([it[2] for it in items]),
                   [it[3] for it in items])
