"""Child of tests/test_detector_bf16.py: runs the bf16 per-row float64 walk (tests/helpers/detector_layers_bf16.py) under the
A/B knob its environment sets (knobs are read once per process) at 384 x 640 and 64 x 96 with three frames, and prints the
forms and worst ratios as one JSON line. Any failure exits non-zero with the fault named."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import detector_layers_bf16 as dlb  # noqa: E402
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd.yolov5 import YoloV5Detector  # noqa: E402


def main():
    sd = synth.make_yolov5s_state_dict()
    forms, ratios = set(), {}
    for net, (fh, fw) in (((384, 640), (720, 1280)), ((64, 96), (270, 480))):
        det = YoloV5Detector(sd, 6, net, max_images=4, compute_dtype="bf16")
        try:
            r = dlb.check_detector(det, synth.make_frames(3, fh, fw, seed=fh), f"bf16 net {net[0]}x{net[1]} n=3/4", log=print)
        finally:
            det.close()
        forms |= set(r["forms"])
        for f, v in r["ratios"].items():
            ratios[f] = max(ratios.get(f, 0.0), v)
        print(f"bf16 net {net}: " + ", ".join(f"{k} {v:.3f}" for k, v in sorted(r["ratios"].items())) + f"; decode {r['decode']:.3f}")
    print(json.dumps({"forms": sorted(forms), "ratios": ratios}))


if __name__ == "__main__":
    main()
