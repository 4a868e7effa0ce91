"""Child of tests/test_lstm_head.py: runs the float64 comparison of tests/helpers/lstm_head.py under the knob its
environment sets (PA_LSTM_* are read once per process) for the cases named in argv[1], and prints each case's forms and
worst ratio to the bar as one JSON line. Any failure exits non-zero with the case named."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import lstm_head as lh  # noqa: E402


def main():
    res = {}
    for name in sys.argv[1].split(","):
        r, forms, _ = lh.run_case(name)
        print(f"{name}: {r:.3f} of the bar, forms {forms}")
        res[name] = {"ratio": r, "forms": forms}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
