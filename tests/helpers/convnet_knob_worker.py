"""Child of tests/test_convnet_layers.py: runs the per-row float64 walk (tests/helpers/convnet_layers.py) under the knob its
environment sets (PA_CONVNET_WINO is read once per process) for the dtypes named in argv[1] at max_crops 64, n 37, and
prints the forms and worst ratios as one JSON line. Any failure exits non-zero with the row named."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import convnet_layers as cl  # noqa: E402
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd.resnet_transformer_detector import ConvNet, build_resnet50_table  # noqa: E402


def main():
    res = {}
    descs, bufs, weights, dim = build_resnet50_table(synth.make_resformer_state_dict(seed=2468))
    for dtype in sys.argv[1].split(","):
        net = ConvNet(descs, bufs, weights, dim, max_crops=64, compute_dtype=dtype)
        try:
            res[dtype] = cl.check_table(net, descs, weights, 37, 5, f"{dtype} knob n=37/64")
        finally:
            net.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
