"""Layer 3 of the exact engine under every form ``PA_WINO_L3_SHAPE`` can force on its Winograd launches (csrc/wino_shape.h: 0 split K,
1 unsplit eight waves, 2 unsplit four waves of 32 channels, 3 unsplit 2 x 2 waves), one child process per value -- the knob is read
once per process -- and one with the knob unset. An engine of 16 crops, traced at 16 and at 5 crops.

Every form: each layer-3 stage within 2e-5 of the stage's largest value of a float64 reference computed from the PREVIOUS stage's
stored output with the engine's folded weights, as tests/test_backbone_layers.py builds its own (its functions are used here). The
unsplit eight-wave form and the 2 x 2 form agree bit for bit: the same 64-channel filter layout, the same sums per lane."""
import os
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FORMS = {"unset": None, "split": "0", "unsplit8": "1", "unsplit4": "2", "tg2": "3"}
STAGES = (10, 11, 12, 13)


@pytest.fixture(scope="module")
def traces(tmp_path_factory):
    import torch

    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = tmp_path_factory.mktemp("wino_l3")
    res = {}
    for tag, v in FORMS.items():
        env = {k: val for k, val in os.environ.items() if k != "PA_WINO_L3_SHAPE"}
        if v is not None:
            env["PA_WINO_L3_SHAPE"] = v
        path = str(d / f"{tag}.npz")
        r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "helpers", "wino_l3_worker.py"), path], capture_output=True, text=True,
                           env=env, timeout=600)
        assert r.returncode == 0, r.stderr[-2000:]
        res[tag] = dict(np.load(path))
    return res


@pytest.fixture(scope="module")
def folded(state_dict):
    sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
    import test_backbone_layers as bl

    return bl, bl.folded_weights(state_dict, bf16=False)


@pytest.mark.gpu
@pytest.mark.parametrize("form", list(FORMS))
@pytest.mark.parametrize("n", [16, 5])
def test_layer3_stages_against_float64(traces, folded, form, n):
    bl, wts = folded
    t = traces[form]
    rows = {s: row for row in bl.conv_table() for s in [row[0]] if s in STAGES}
    for s in STAGES:
        _, name, ci, co, stride, src, resid = rows[s]
        got = t[f"n{n}_s{s}"]
        assert bl.border_is_zero(got, 1), (form, n, name)
        w, b = wts[s]
        r = None
        if resid == "branch":
            a = t[f"n{n}_aux{s}"]
            assert bl.f32_ratio(bl.interior(a), bl.ref_branch(t[f"n{n}_s{s - 2}"], wts[("ds", s)][0])) <= 1.0, (form, n, name, "branch")
            r = bl.interior(a).astype(np.float64)
        elif resid is not None:
            r = bl.interior(t[f"n{n}_s{resid}"]).astype(np.float64)
        ref = bl.ref_conv(t[f"n{n}_s{src}"], w, b, stride, r)
        assert (ref != 0).mean() > 0.2, (form, n, name)
        ratio = bl.f32_ratio(bl.interior(got), ref)
        print(f"{form} n={n} stage {s} {name}: max|err| = {ratio:.3f} x the 2e-5 bar")
        assert ratio <= 1.0, (form, n, name, ratio)


@pytest.mark.gpu
def test_unsplit_eight_wave_and_2x2_forms_agree_bit_for_bit(traces):
    a, b = traces["unsplit8"], traces["tg2"]
    for key in a:
        assert a[key].any() and np.array_equal(a[key], b[key]), key


@pytest.mark.gpu
def test_the_knob_leaves_the_stages_in_front_of_layer3_alone_and_small_engines_on_the_split(traces):
    """Stage 9 (layer2.1.conv2) and the stride-2 opener (stage 10) are no layer-3 Winograd launches: the same bits in every process.
    An engine of 16 crops is below the default's threshold: unset = split, bit for bit."""
    for tag in FORMS:
        for n in (16, 5):
            for s in (9, 10):
                assert np.array_equal(traces[tag][f"n{n}_s{s}"], traces["split"][f"n{n}_s{s}"]), (tag, n, s)
    for key in traces["unset"]:
        assert np.array_equal(traces["unset"][key], traces["split"][key]), key
