"""Child of tests/test_convnet_bf16.py: runs the bf16 per-row float64 walk (tests/helpers/convnet_layers_bf16.py) under the knob its
environment sets (PA_CONVNET_BG_SPLIT is read once per process) at max_crops 64 for the crop counts in argv[1], and prints the
forms and worst ratios as one JSON line. Any failure exits non-zero with the row named."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import convnet_layers_bf16 as clb  # noqa: E402
from playaid_core_amd import synth  # noqa: E402
from playaid_core_amd.resnet_transformer_detector import ConvNet, build_resnet50_table  # noqa: E402


def main():
    res = {}
    descs, bufs, weights, dim = build_resnet50_table(synth.make_resformer_state_dict(seed=2468))
    for n in (int(v) for v in sys.argv[1].split(",")):
        net = ConvNet(descs, bufs, weights, dim, max_crops=64, compute_dtype="bf16")
        try:
            res[str(n)] = clb.check_table(net, descs, weights, n, 5, f"bf16 knob n={n}/64")
        finally:
            net.close()
    print(json.dumps(res))


if __name__ == "__main__":
    main()
