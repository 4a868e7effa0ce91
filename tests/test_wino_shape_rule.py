"""How the ResNet-18 engine shapes the launches of its Winograd layers (csrc/wino_shape.h, csrc/engine_plan.h's wino_layer_shape),
without a GPU: tests/helpers/wino_shape_table.cpp prints, over the table ``pa_create`` itself builds, the shape and the channels per
workgroup each of the sixteen 3x3 layers gets. Compiled with the host C++ compiler alone ($CXX, else g++).

The expected values are written out by hand from the rules: a stride-2 opener is no Winograd layer; a layer under "split" gets the
workgroup width of ``wino_pick_bn`` with split-K scratch (64-channel workgroups times the largest power-of-two split that keeps eight
chunks per split and at most 256 workgroups; under 192 of them: 32 channels); the unsplit shapes fix the width themselves (64, 32,
64). Only the 8 x 8 maps -- layer 3 -- are open to ``PA_WINO_L3_SHAPE``, and to the default (unsplit four-wave workgroups of 16
sub-blocks x 32 channels) where the split would hold the whole chip -- 256 workgroups -- and the default has 256 of its own: 125 to
128 crops."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(ROOT, "tests", "helpers", "wino_shape_table.cpp")

OPENERS = ["layer2.0.conv1", "layer3.0.conv1", "layer4.0.conv1"]
ALL3X3 = [f"layer{l}.{b}.conv{c}" for l in (1, 2, 3, 4) for b in (0, 1) for c in (1, 2)]
LAYER3 = ["layer3.0.conv2", "layer3.1.conv1", "layer3.1.conv2"]
DTYPES = ("f32", "emulated_f32")
SHAPES = {0: ("split", None), 1: ("unsplit8", 64), 2: ("unsplit4", 32), 3: ("tg2", 64)}

# Under "split", by hand (sub-blocks = crops x (map / 4)^2; chunks = cin / 8):
#   128 crops: layer 1 512 workgroups of 64 channels; layer 2 256; layer 3 128 x 2 splits = 256; layer 4 64 x 4 = 256: all 64
#   16 crops: layer 1 64 (8 chunks: no split); layer 2 32 x 2; layer 3 16 x 4; layer 4 8 x 8: all under 192 -> 32
#   1 crop: 4; 2 x 2; 4 x 4; 8 x 8 -> 32
SPLIT_BN = {128: 64, 16: 32, 1: 32}
# what layer 3 gets with the knob unset, at 128 crops (the headline's engines)
LAYER3_DEFAULT_AT_128 = ("unsplit4", 32)


@pytest.fixture(scope="module")
def table(tmp_path_factory):
    cxx = os.environ.get("CXX") or "g++"
    if not shutil.which(cxx.split()[0]):
        pytest.skip(f"no host C++ compiler ({cxx})")
    exe = str(tmp_path_factory.mktemp("wino_shape") / "wino_shape_table")
    subprocess.run(cxx.split() + ["-std=c++17", "-O1", "-o", exe, SRC], check=True)

    def run(cases, *knobs):
        env = {k: v for k, v in os.environ.items() if not k.startswith("PA_")}
        out = subprocess.run([exe, *knobs, *cases], check=True, capture_output=True, text=True, env=env).stdout
        rows, head = {}, None
        for line in out.splitlines():
            kind, *fields = line.split()
            f = dict(x.split("=", 1) for x in fields)
            if kind == "knobs":
                head = f
            else:
                rows[(f["dtype"], int(f["max_crops"]), f["layer"])] = (f["shape"], int(f["bn"]))
        return head, rows

    return run


CASES = [f"{dt}:{nc}" for dt in DTYPES for nc in (128, 16, 1)]


def _expected(dt, nc, layer, knob=None):
    if layer in OPENERS:
        return ("none", 0)
    if layer in LAYER3:
        if knob is not None and knob != 0:
            return SHAPES[knob]
        if knob is None and nc == 128:
            return LAYER3_DEFAULT_AT_128
    return ("split", SPLIT_BN[nc])


def test_default_shapes_of_the_sixteen_layers(table):
    head, rows = table(CASES)
    assert head["wino_l3_shape"] == "-1" and head["min_wg"] == "256"
    assert head["default"] == LAYER3_DEFAULT_AT_128[0]
    assert len(rows) == len(CASES) * 16
    for dt in DTYPES:
        for nc in (128, 16, 1):
            for layer in ALL3X3:
                assert rows[(dt, nc, layer)] == _expected(dt, nc, layer), (dt, nc, layer)


def test_layers_1_2_4_get_what_they_got_before_the_rule(table):
    """... which is ``wino_pick_bn(cout, sub-blocks, cin)`` with the split-K scratch, under every value of the knob."""
    for knob in (None, 0, 1, 2, 3):
        _, rows = table(CASES, *([f"PA_WINO_L3_SHAPE={knob}"] if knob is not None else []))
        for (dt, nc, layer), got in rows.items():
            if layer in LAYER3:
                continue
            assert got == (("none", 0) if layer in OPENERS else ("split", SPLIT_BN[nc])), (knob, dt, nc, layer)


@pytest.mark.parametrize("knob", [0, 1, 2, 3])
def test_the_knob_moves_layer_3_and_nothing_else(table, knob):
    head, rows = table(CASES, f"PA_WINO_L3_SHAPE={knob}")
    assert head["wino_l3_shape"] == str(knob)
    for (dt, nc, layer), got in rows.items():
        assert got == _expected(dt, nc, layer, knob), (dt, nc, layer)
    # every engine size: a forced shape does not look at max_crops
    for dt in DTYPES:
        for nc in (128, 16, 1):
            assert {rows[(dt, nc, layer)] for layer in LAYER3} == {SHAPES[knob] if knob else ("split", SPLIT_BN[nc])}


def test_the_default_applies_where_the_split_would_fill_the_chip(table):
    """Layer 3 has 4 sub-blocks per crop, pixel tiles of 16 sub-blocks, 4 channel tiles of 64 (8 of 32). 124 crops: 31 pixel tiles, 124
    workgroups x 2 splits = 248 < 256 -> split. 125..128 crops: 32 pixel tiles, 128 x 2 = 256 split workgroups, 256 of the default's
    -> the default. 129 crops: 33 pixel tiles, 132 x 2 > 256: no split possible, which is what the layer had before (32-channel
    workgroups, nothing to split). 256 crops: 256 workgroups of 64 channels, no split, as before."""
    _, rows = table(["f32:124", "f32:125", "f32:127", "f32:129", "f32:256", "f32:64", "f32:96"])
    assert rows[("f32", 124, "layer3.1.conv1")] == ("split", 64)
    assert rows[("f32", 125, "layer3.1.conv1")] == LAYER3_DEFAULT_AT_128
    assert rows[("f32", 127, "layer3.0.conv2")] == LAYER3_DEFAULT_AT_128
    assert rows[("f32", 129, "layer3.1.conv1")] == ("split", 32)
    assert rows[("f32", 256, "layer3.1.conv1")] == ("split", 64)
    # 64 crops: 64 workgroups x 4 splits fill the chip, but the default would have 128 workgroups; 96 crops: 96 x 2 = 192
    assert rows[("f32", 64, "layer3.1.conv2")] == ("split", 64) and rows[("f32", 96, "layer3.1.conv2")] == ("split", 64)
    for nc in (124, 125, 256):
        assert rows[("f32", nc, "layer1.0.conv1")][0] == "split" and rows[("f32", nc, "layer4.1.conv2")][0] == "split"


def test_unknown_knob_values_leave_the_rule_alone(table):
    for v in ("4", "-2", "99"):
        _, rows = table(["f32:128"], f"PA_WINO_L3_SHAPE={v}")
        assert rows[("f32", 128, "layer3.1.conv1")] == LAYER3_DEFAULT_AT_128
