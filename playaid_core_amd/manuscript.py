"""``manuscript`` CLI plumbing (config 0 of BASELINE.json): game log + optional
``ai_output.yaml`` -> timeline -> per-frame fighter records, and -- with
``--output-video-path`` -- the annotated video the reference's product is.

Keeps the reference's entry point and flags (``playaid/manuscript.py:293-385``:
``--video-path --log-path --ai-output-path --frames --skip-graphs
--skip-summaries --show-timer``; ``log_offset`` forced to 5 for ``--video-path``
runs, ``:377``). Without an output path the loop walks the timeline on the CPU
and emits the records that rendering would consume, plus a small summary, so
the hand-off between the MI355X inference path (``ai_runner.py`` ->
``ai_output.yaml``) and the product CLI can be exercised end to end without a
display, ffmpeg or a GPU.

With an output path ``Manuscript.render`` does what the reference does per frame
(``:111-244``) on the MI355X: the input clip (Motion-JPEG, ``video.VideoCapture``)
is decoded in chunks into HBM, every fighter's label (``frame_labels`` below:
``:165-227`` as a pure function) is drawn at its box by ``annotator.Annotator``
(``csrc/annotate.hip``), the frames are encoded by ``jpeg_encode.JpegEncoder``
(quality 95, 4:2:0) and the files written as a Motion-JPEG ``.avi``
(``video.write_avi_mjpeg``) -- no frame visits the host. Still out of scope
(SURVEY.md section 2 rows 10-12): the matplotlib / bokeh charts (the 400-pixel
padding they would fill stays black unless ``--skip-graphs``), ``mp4v`` output
and the ffmpeg audio pass.

Like the reference, this CLI never calls ``AIRunner`` itself (the ``run_ai``
argument is accepted and ignored there, ``manuscript.py:49,371``); pass
``--run-ai`` to produce ``ai_output.yaml`` first (needs the MI355X).
"""
from __future__ import annotations

import json
import os
from collections import Counter
from typing import Dict, List, Optional, Tuple

import click

from . import anim_ontology
from .fighter import Fighter
from .timeline import load_ground_truth_from_path, load_timeline_from_ai_output


FighterRecord = Fighter  # round-1 name of the per-fighter record


def update_fighters_from_timeline(frame_number: int, ground_truth: List[Dict], fighters: List[Fighter]):
    """``timeline.py:186-201``: construct on the first call / frame 0, ``Fighter.update`` afterwards."""
    by_id = sorted(ground_truth, key=lambda d: d["fighter_id"])
    if fighters and frame_number != 0:
        for fighter, row in zip(fighters, by_id):
            fighter.update(frame_number, row)
    else:
        fighters.extend(Fighter(frame_num=frame_number, data=row) for row in by_id)
    return fighters


# label background by fighter_id (manuscript.py:115-124), and the one of a fighter in hitstun (:200-202)
LABEL_COLORS = {0: (25, 58, 115), 1: (201, 99, 48), 2: (201, 99, 48), 3: (201, 99, 48), 4: (201, 99, 48), 5: (201, 99, 48),
                6: (201, 99, 48), 7: (201, 99, 48)}
HITSTUN_COLOR = (55, 55, 55)
TIMER_BOX = (980, 80, 1200, 60)
RENDER_LINE_WIDTH = 4  # set_frame(..., line_width=4), manuscript.py:158 (no box is outlined: draw_box=False throughout)


def fighter_label(fighter) -> str:
    """``manuscript.py:169-179``: the action (nothing for ``Undefined`` / empty), ``| #<animation frame>``, ``| <anim_state>``."""
    label = f"{fighter.action}" if fighter.action != "Undefined" and fighter.action != "" else ""
    label += f" | #{fighter.animation_frame_num}"
    if fighter.anim_state:
        label += f" | {fighter.anim_state}"
    return label


def frame_labels(frame_number: int, fighters: List[Fighter], width: int, height: int, log_offset: int = 0,
                 show_timer: bool = False) -> List[Tuple[Tuple[int, int, int, int], str, Tuple[int, int, int]]]:
    """The ``box_label`` calls of one rendered frame (``manuscript.py:165-227``), as (box, label, colour); every one is made
    with ``draw_box=False``. A negative ``log_offset`` skips the fighters' labels of the first ``-log_offset`` frames. The
    timer takes the colour of the LAST fighter the loop touched, hitstun or not (the reference reads its loop variable
    after the loop); with no fighters the reference would fail there, here the timer is left out."""
    calls = []
    fighter = None
    for fighter in fighters:
        if log_offset < 0 and frame_number < abs(log_offset):
            break
        color = HITSTUN_COLOR if fighter.hitstun_left else LABEL_COLORS[fighter.fighter_id]
        calls.append((tuple(fighter.crop.xyxy_pixels(width, height)), fighter_label(fighter), color))
    if show_timer and fighter is not None:
        calls.append((TIMER_BOX, f"Frame #{max(frame_number + log_offset, 0)}", LABEL_COLORS[fighter.fighter_id]))
    return calls


class Manuscript:
    def __init__(self, input_video_path: str, ground_truth_path: str = None, ai_output_path: str = None,
                 start_frame: int = 0, max_frames: int = -1, log_offset: int = 0, run_ai: bool = False, **_ignored):
        self.input_video_path = input_video_path
        self.start_frame = start_frame
        self.log_offset = log_offset
        self.timeline = []
        if ground_truth_path:
            self.timeline = load_ground_truth_from_path(ground_truth_path, log_offset=log_offset)
        if ai_output_path:  # overrides, as manuscript.py:101-102
            self.timeline = load_timeline_from_ai_output(ai_output_path)
        self.max_frames = len(self.timeline) if max_frames < 0 else min(max_frames, len(self.timeline))

    def render(self, output_video_path: Optional[str] = None, skip_graphs: bool = False, show_timer: bool = False,
               chunk_frames: int = 32) -> Dict:
        """Walks the timeline and returns the summary. With ``output_video_path`` it also renders the annotated clip
        there (Motion-JPEG ``.avi``; needs the MI355X): the frames are decoded, drawn on and encoded on the device,
        ``chunk_frames`` at a time with one wait per chunk. ``skip_graphs=False`` pads the frames for the reference's
        charts (400 / 400 / 400, black: the charts are not drawn)."""
        fighters: List[Fighter] = []
        actions = [Counter(), Counter()]
        moves = [0, 0]
        writer = _VideoRenderer(self.input_video_path, output_video_path, self.start_frame, self.max_frames, not skip_graphs,
                                chunk_frames) if output_video_path else None
        for i in range(self.start_frame, self.max_frames):
            fighters = update_fighters_from_timeline(i, self.timeline[i], fighters)
            for p, f in enumerate(fighters):
                actions[p][f.action] += 1
                moves[p] = f.move_counter
            if writer:
                writer.add(i, frame_labels(i, fighters, writer.width, writer.height, self.log_offset, show_timer))
        if writer:
            writer.finish()
        return {
            "frames": max(self.max_frames - self.start_frame, 0),
            "fighters": [
                {"fighter_id": f.fighter_id, "fighter_name": f.fighter_name, "moves": moves[p],
                 "actions": dict(actions[p]), "last_crop": str(f.crop) if f.crop else None}
                for p, f in enumerate(fighters)
            ],
        }


class _VideoRenderer:
    """The device side of ``Manuscript.render``: collects the draw lists of ``chunk_frames`` frames, then decode ->
    annotate -> encode for the chunk (all enqueued; the one wait is the copy of the JPEG files to the host)."""

    def __init__(self, input_video_path: str, output_video_path: str, start_frame: int, end_frame: int, show_stats: bool, chunk_frames: int):
        from . import video
        from .annotator import Annotator
        from .jpeg_encode import JpegEncoder

        self.path = output_video_path
        self.cap = video.VideoCapture(input_video_path, batch_frames=chunk_frames)
        if not self.cap.isOpened():
            raise video.VideoError(f"{input_video_path}: not a Motion-JPEG clip (.avi with MJPG frames, .mjpeg, or a directory of .jpg)")
        if end_frame > self.cap.frame_count():
            raise video.VideoError(f"{input_video_path}: {self.cap.frame_count()} frames, the timeline asks for {end_frame}")
        self.width, self.height, self.fps = self.cap.width, self.cap.height, self.cap.fps
        self.chunk = max(1, min(int(chunk_frames), max(end_frame - start_frame, 1)))
        self.annotator = Annotator(int(self.fps), self.width, self.height, show_stats=show_stats, max_frames=self.chunk)
        self.encoder = JpegEncoder.for_frames(self.chunk, self.annotator.output_height, self.annotator.output_width, subsampling=2)
        self.files: List[bytes] = []
        self.pending: List[Tuple[int, list]] = []

    def add(self, frame_number: int, calls):
        self.pending.append((frame_number, calls))
        if len(self.pending) == self.chunk:
            self.flush()

    def flush(self):
        import torch

        from . import video

        if not self.pending:
            return
        j0, n = self.pending[0][0], len(self.pending)
        status = torch.zeros(n, dtype=torch.int32, device=self.annotator.device_name)
        for exact in (False, True):  # (a frame whose entropy decode has not settled in the enqueued passes is decoded again, exactly)
            status.zero_()
            frames = self.cap.read_frames(j0, n, status=status, exact=exact)
            self.annotator.set_frames(frames, line_width=RENDER_LINE_WIDTH)
            for k, (_, calls) in enumerate(self.pending):
                for box, label, color in calls:
                    self.annotator.box_label(k, box, label=label, color=color, draw_box=False)
            files = self.encoder.encode_frames(self.annotator.result(), quality=95, subsampling=2)
            bits = status.cpu().numpy()
            if not bits.any():
                break
            if exact or (bits & ~8).any():
                raise video.VideoError(f"frames {j0}..{j0 + n - 1} of the input clip do not decode (status {bits.tolist()})")
        self.files += files
        self.pending = []

    def finish(self):
        from . import video

        self.flush()
        video.write_avi_mjpeg(self.path, self.files, self.fps, self.annotator.output_width, self.annotator.output_height)
        self.encoder.close()
        self.annotator.close()
        self.cap.release()


@click.command()
@click.option("--frames", "-f", default=None, help="Frames in the format start,end. If empty, will use entire video.")
@click.option("--skip-graphs", "-s", is_flag=True, help="No 400-pixel chart padding in the rendered clip (the charts themselves are out of scope)")
@click.option("--skip-summaries", "-c", is_flag=True, help="Accepted for compatibility")
@click.option("--show-timer", "-t", is_flag=True, help="Draw 'Frame #<n>' in the rendered clip")
@click.option("--video-path", "-p", default=None, help="Path to the input clip (.npz: frames + labels)")
@click.option("--log-path", default=None, help="Path to the input log (JSON lines)")
@click.option("--ai-output-path", "-ai", default=None, help="Path to cached ai output")
@click.option("--run-ai", is_flag=True, help="Run AIRunner on the MI355X first and use its ai_output.yaml")
@click.option("--checkpoint", default=None, help="CNNActionDetector .ckpt for --run-ai")
@click.option("--summary-json", default=None, help="Where to write the summary (default: stdout only)")
@click.option("--output-video-path", "-o", default=None,
              help="Render the annotated clip there (Motion-JPEG .avi; needs the MI355X and a Motion-JPEG --video-path)")
@click.option("--params-labels", default=None,
              help="params_labels.csv (motion_kind hex -> param string); default $PLAYAID_PARAMS_LABELS. "
                   "Without it log-derived actions are 'Undefined', as for any hex the table lacks")
def run_manuscript(frames, skip_graphs, skip_summaries, show_timer, video_path, log_path, ai_output_path, run_ai,
                   checkpoint, summary_json, output_video_path, params_labels):
    """Entrypoint to Manuscript"""
    if params_labels or os.environ.get("PLAYAID_PARAMS_LABELS"):
        anim_ontology.load_hex_to_action(params_labels)
    if not video_path:
        print("Must specify --video-path")
        return
    start_frame, end_frame = 0, -1
    if frames:
        start_frame, end_frame = map(int, frames[1:].split(",") if frames[0] == "=" else frames.split(","))
    if run_ai:
        from .ai_runner import AIRunner  # needs the HIP library and a GPU

        runner = AIRunner(video_path, checkpoint_path=checkpoint)
        runner.run_action_recognition()
        runner.write_output()
        ai_output_path = runner.ai_output_file
    m = Manuscript(input_video_path=video_path, ground_truth_path=log_path, ai_output_path=ai_output_path,
                   start_frame=start_frame, max_frames=end_frame, log_offset=5 if log_path else 0, run_ai=run_ai)
    summary = m.render(output_video_path=output_video_path, skip_graphs=skip_graphs, show_timer=show_timer)
    text = json.dumps(summary, indent=1, sort_keys=True)
    if summary_json:
        os.makedirs(os.path.dirname(os.path.abspath(summary_json)), exist_ok=True)
        with open(summary_json, "w") as f:
            f.write(text)
    print(text)
    print("COMPLETED")


if __name__ == "__main__":
    run_manuscript()
