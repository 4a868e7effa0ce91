"""How far the non-default arithmetics move the ANSWERS: agreement of ``compute_dtype="bf16"`` and ``"emulated_f32"`` with
``"f32"`` on a synthetic clip, scored on the device (``Engine.agreement``: run A's ``action_id`` read in place as the labels
of run B, ``pa_eval_update`` with ``label_stride=4``).

    python scripts/eval_agreement.py [--frames 64] [--height 720] [--width 1280] [--out profiles/eval_agreement.txt]

Prints, per arithmetic: the fraction of (frame, fighter) labels that agree with the fp32 run, the flips (fp32 action ->
other action: count), B's NLL of A's labels, mean confidence and max |delta logp|. A record, not a gate: synthetic frames and
seeded weights say nothing about a trained checkpoint on real footage -- run it on labelled clips with ``AIRunner.evaluate``.
"""
import argparse
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd.anim_ontology import ACTIONS  # noqa: E402
from playaid_core_amd.engine import Engine  # noqa: E402


def run(sd, dtype, frames, boxes):
    eng = Engine(sd, max_batch_frames=64, max_clip_frames=max(64, frames.shape[0]), max_frame_height=frames.shape[1],
                 max_frame_width=frames.shape[2], compute_dtype=dtype)
    n = frames.shape[0]
    records, logp = eng.alloc_records(n - 1), eng.alloc_logp(n - 1)
    eng.infer_clip_device(torch.from_numpy(frames).to(eng.device), torch.from_numpy(boxes).double().to(eng.device), records, logp)
    torch.cuda.synchronize()
    return eng, records, logp


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--frames", type=int, default=64)
    ap.add_argument("--height", type=int, default=720)
    ap.add_argument("--width", type=int, default=1280)
    ap.add_argument("--seed", type=int, default=1234)
    ap.add_argument("--out", default=None)
    args = ap.parse_args()
    sd = synth.make_state_dict(seed=args.seed)
    frames = synth.make_frames(args.frames, args.height, args.width)
    boxes = synth.make_boxes(args.frames, args.height, args.width)
    lines = [f"eval_agreement: {args.frames} frames {args.height}x{args.width} synthetic, seeded weights (seed {args.seed}), "
             f"{(args.frames - 1) * 2} (frame, fighter) rows, labels = the f32 run's action_id"]
    ref, rec_a, logp_a = run(sd, "f32", frames, boxes)
    own = ref.agreement(rec_a, logp_a)
    lines.append(f"f32 vs f32: agreement {own['accuracy']:.6f} (must be 1), classes predicted {int((np.diag(own['confusion']) > 0).sum())}")
    for dtype in ("emulated_f32", "bf16"):
        eng, _, logp_b = run(sd, dtype, frames, boxes)
        out = ref.agreement(rec_a, logp_b)
        cm = out["confusion"]
        flips = [(ACTIONS[a], ACTIONS[b], int(cm[a, b])) for a, b in zip(*np.nonzero(cm - np.diag(np.diag(cm))))]
        dmax = float((logp_b - logp_a).abs().max())
        lines.append(f"{dtype} vs f32: agreement {out['accuracy']:.6f} ({out['rows'] - int(np.trace(cm))} of {out['rows']} labels flip), "
                     f"nll of f32's labels {out['loss']:.6f} (f32's own {own['loss']:.6f}), mean confidence {out['mean_confidence']:.4f}% "
                     f"(f32 {own['mean_confidence']:.4f}%), max |dlogp| {dmax:.3e}")
        lines.append(f"{dtype} flips (f32 action -> {dtype} action: rows): " + (", ".join(f"{a} -> {b}: {c}" for a, b, c in flips) or "none"))
        eng.close()
    ref.close()
    text = "\n".join(lines) + "\n"
    print(text, end="")
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
