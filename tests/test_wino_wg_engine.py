"""Layers 1 and 2 of the exact engine under every launch width ``PA_WINO_WG`` can force on their Winograd launches
(csrc/wino_shape.h: 32 = four-wave workgroups of 32 channels on the 64-channel filter layout, 64 = the eight-wave workgroups), one
child process per value -- the knob is read once per process -- and one with the knob unset. An engine of 16 crops, traced at 16 and
at 5 crops.

An engine this small lays its filters out for 32-channel workgroups by itself, which leaves the width nothing to choose; so every
child runs under ``PA_WINO_BN=64 PA_WINO_KS=1``: 64-channel layouts and no K split, the state layers 1 and 2 have in the headline's
engines of 128 crops, where the width is open (``tests/test_wino_wg_rule.py`` pins that it is, under these very knobs). The width
never changes a bit: every stage of layers 1 and 2 and the log-probabilities are identical across the three processes."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WIDTHS = {"unset": None, "wg32": "32", "wg64": "64"}
STAGES = (2, 3, 4, 5, 6, 7, 8, 9)


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("wino_wg")
    res = {}
    for tag, v in WIDTHS.items():
        env = {k: val for k, val in os.environ.items() if not k.startswith("PA_WINO_")}
        env.update(PA_WINO_BN="64", PA_WINO_KS="1")
        if v is not None:
            env["PA_WINO_WG"] = v
        path = str(d / f"{tag}.npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "wino_wg_worker.py"), path], capture_output=True, text=True,
                           env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = dict(np.load(path))
    return res


@pytest.mark.gpu
@pytest.mark.parametrize("n", [16, 5])
def test_every_stage_of_layers_1_and_2_is_bit_identical_across_the_widths(traces, n):
    for s in STAGES:
        a = traces["wg64"][f"n{n}_s{s}"]
        assert a.any(), (n, s)
        for tag in ("wg32", "unset"):
            assert np.array_equal(traces[tag][f"n{n}_s{s}"], a), (tag, n, s)
    for tag in ("wg32", "unset"):
        assert np.array_equal(traces[tag][f"n{n}_aux7"], traces["wg64"][f"n{n}_aux7"]), (tag, n)
        assert np.array_equal(traces[tag][f"n{n}_s1"], traces["wg64"][f"n{n}_s1"]), (tag, n)


@pytest.mark.gpu
def test_the_log_probabilities_are_identical_across_the_widths(traces):
    a = traces["wg64"]["logp"]
    assert a.shape[0] == 2 and np.isfinite(a).all() and a.any()
    for tag in ("wg32", "unset"):
        assert np.array_equal(traces[tag]["logp"], a), tag


@pytest.mark.gpu
def test_layer_1_stages_against_float64(traces, state_dict):
    """The traced stages are real results, not equal garbage: layer 1 under width 32, each stage within 2e-5 of the stage's largest
    value of a float64 reference computed from the previous stage's stored output (tests/test_backbone_layers.py's own functions)."""
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_backbone_layers as bl

    wts = bl.folded_weights(state_dict, bf16=False)
    t = traces["wg32"]
    rows = {row[0]: row for row in bl.conv_table() if row[0] in (2, 3, 4, 5)}
    for n in (16, 5):
        for s in (2, 3, 4, 5):
            _, name, ci, co, stride, src, resid = rows[s]
            w, b = wts[s]
            r = bl.interior(t[f"n{n}_s{resid}"]).astype(np.float64) if resid is not None else None
            ref = bl.ref_conv(t[f"n{n}_s{src}"], w, b, stride, r)
            ratio = bl.f32_ratio(bl.interior(t[f"n{n}_s{s}"]), ref)
            print(f"n={n} stage {s} {name}: max|err| = {ratio:.3f} x the 2e-5 bar")
            assert ratio <= 1.0, (n, name, ratio)
