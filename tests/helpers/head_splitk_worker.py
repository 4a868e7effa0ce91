"""Child of tests/test_head_windows.py: runs the float64 comparison of tests/helpers/head_windows.py on the served head (S = 7,
A = 63, both fighters) and on an S = 1 / A = 5 / one-fighter engine under the ``PA_HEAD_SPLITK`` its environment sets (the knob
is read when an engine is created), and prints each engine's worst figures and the sha256 of its log-probabilities' bytes as one
JSON line. Any failure exits non-zero with the case named."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

from helpers import head_windows as hw  # noqa: E402


def main():
    knob = os.environ.get("PA_HEAD_SPLITK", "unset")
    res = {}
    for name, case in (("S7", hw.GRID[hw.SERVED]), ("S1", hw.SPLITK_S1)):
        ms, sha = hw.run_case(case, what=f"PA_HEAD_SPLITK={knob} ")
        res[name] = {"err": max(m["err"] for m in ms), "prob_err": max(m["prob_err"] for m in ms),
                     "skipped": max(m["skipped"] for m in ms), "windows": sum(m["windows"] for m in ms), "sha256": sha}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
